// The observation table is shared with the host mirrors and lives under include/, like view_info.h; the kernels take it from
// here, with the C ABI's checks of its arguments.
#pragma once
#include <climits>
#include "../../include/se2lam_amd/obs_table.h"
#include "common.h"

namespace se2gpu {

// d_counts, cap, nframes of a call named `who`; the capacity refusal comes last
inline int check_frame_slots(const char* who, const void* d_counts, int cap, int nframes) {
    SE2_NEED(d_counts);
    SE2_REQUIRE(cap >= 1, SE2GPU_ERR_INVALID, "%s: cap = %d is below 1", who, cap);
    SE2_REQUIRE(nframes >= 1, SE2GPU_ERR_INVALID, "%s: nframes = %d is below 1", who, nframes);
    SE2_REQUIRE((long long)nframes * cap <= INT_MAX, SE2GPU_ERR_CAPACITY, "%s: nframes * cap = %lld exceeds the limit %d", who,
                (long long)nframes * cap, INT_MAX);
    return SE2GPU_OK;
}

// d_mp_ptr, d_obs_frame, d_obs_ftr, m, nobs; without observations their arrays may be absent
inline int check_obs_csr(const char* who, const void* d_mp_ptr, const void* d_obs_frame, const void* d_obs_ftr, int m, int nobs) {
    SE2_NEED(d_mp_ptr);
    SE2_REQUIRE(m >= 0, SE2GPU_ERR_INVALID, "%s: m = %d is negative", who, m);
    SE2_REQUIRE(nobs >= 0, SE2GPU_ERR_INVALID, "%s: nobs = %d is negative", who, nobs);
    SE2_NEED_IF(nobs > 0, d_obs_frame); SE2_NEED_IF(nobs > 0, d_obs_ftr);
    return SE2GPU_OK;
}

}  // namespace se2gpu
