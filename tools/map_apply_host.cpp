// The host mirror of the map update (include/se2lam_amd/MapUpdate.h, applyObservations) behind one C function, for
// tools/map_apply_bench.py: the arguments of se2gpu_map_apply_batch_device without the handle and the work space, on HOST memory.
//   g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC -I include tools/map_apply_host.cpp -o libmap_apply_host.so
#include "se2lam_amd/MapUpdate.h"

extern "C" int map_apply_host(const int32_t* counts, int cap, int nframes, const uint8_t* frame_null, const int32_t* mp_ptr,
                              const int32_t* obs_frame, const int32_t* obs_ftr, const float* obs_view, const float* obs_info,
                              const int32_t* sizes_in, int m_cap, int nobs_cap, const int32_t* job_prev, const int32_t* job_new, int B,
                              const uint8_t* kind, const int32_t* src, const float* view, const float* info, const float* new_pos_w,
                              const float* info_prev, const float* local_pos, const uint8_t* good_prl_row, int kinds,
                              const int32_t* parallax_status, float* pos, uint8_t* good_prl, uint8_t* mp_null, float* mp_normal,
                              int32_t* ftr_mp, uint8_t* kf_observed, float* view_pos, float* view_info, int32_t* mp_ptr_new,
                              int32_t* obs_frame_new, int32_t* obs_ftr_new, float* obs_view_new, float* obs_info_new,
                              int32_t* new_frame, int32_t* sizes_out, int32_t* job_counts) {
    se2lam_amd::MapApplyTables t;
    t.counts = counts; t.cap = cap; t.nframes = nframes; t.frameNull = frame_null;
    t.mpPtr = mp_ptr; t.obsFrame = obs_frame; t.obsFtr = obs_ftr; t.obsView = obs_view; t.obsInfo = obs_info;
    t.sizesIn = sizes_in; t.mCap = m_cap; t.nobsCap = nobs_cap;
    t.B = B; t.jobPrev = job_prev; t.jobNew = job_new; t.kind = kind; t.src = src; t.view = view; t.info = info;
    t.newPosW = new_pos_w; t.infoPrev = info_prev; t.localPos = local_pos; t.goodPrlRow = good_prl_row; t.kinds = kinds;
    t.parallaxStatus = parallax_status;
    t.pos = pos; t.goodPrl = good_prl; t.mpNull = mp_null; t.mpNormal = mp_normal;
    t.ftrMP = ftr_mp; t.kfObserved = kf_observed; t.viewPos = view_pos; t.viewInfo = view_info;
    t.mpPtrNew = mp_ptr_new; t.obsFrameNew = obs_frame_new; t.obsFtrNew = obs_ftr_new; t.obsViewNew = obs_view_new;
    t.obsInfoNew = obs_info_new; t.newFrame = new_frame; t.sizesOut = sizes_out; t.jobCounts = job_counts;
    return se2lam_amd::applyObservations(t);
}
