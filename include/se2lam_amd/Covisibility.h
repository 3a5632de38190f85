// Covisibility - header-only mirror, C++17, of
//   Point2f Map::compareViewMPs(pKF1, pKF2, spMPs)              src/Map.cpp:354-369    compareViewMPs(view, a, b, common)
//   double  Map::compareViewMPs(pKFNow, spKFsRef, spMPsRet, k)  src/Map.cpp:373-400    compareViewMPs(view, kf, refs, common, k)
//   Map::updateCovisibility                                     src/Map.cpp:785-799    updateCovisibility(view, newKF, localKFs)
//   the redundancy test of Map::pruneRedundantKF                src/Map.cpp:193-196    isRedundant(view, kf, covisKFs)
// on tables in HOST memory: the CPU stand-in where no device copy exists and the baseline tools/covis_bench.py times.  They are
// written as the reference writes them - a sorted container of points per key frame, one look-up per point and key frame -
// and share nothing with the kernels' bit matrix.
//   CovisibilityTable   the same for batches in device memory (se2gpu_covis_build_device / _pairs_device / _refset_device)
// Key frames are slots 0..nframes-1, map points indices 0..m-1; the observation CSR is read by obs_table.h's entry and segment
// rule (null key frames are not skipped) and must describe the key frame's side (se2gpu.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../se2gpu.h"
#include "ORBmatcher.h"
#include "obs_table.h"
#include "types.h"

namespace se2lam_amd {

// The tables in host memory with KeyFrame::mObservations rebuilt from them: index() once after the tables change.
struct CovisHostView {
    int nframes = 0, cap = 0, m = 0, nobs = 0;
    const int32_t* counts = nullptr;     // nframes
    const int32_t* mpPtr = nullptr;      // m + 1
    const int32_t* obsFrame = nullptr;   // nobs
    const int32_t* obsFtr = nullptr;     // nobs
    const uint8_t* mpNull = nullptr;     // m or null: MapPoint::isNull()
    const uint8_t* goodPrl = nullptr;    // m or null: MapPoint::isGoodPrl()
    std::vector<std::vector<int32_t>> observations;   // per key frame: the points it observes, ascending, each once

    void index() {
        observations.assign(nframes, std::vector<int32_t>());
        const se2gpu::FrameSlots slots{counts, nullptr, cap, nframes};
        const se2gpu::ObsCsr csr{mpPtr, obsFrame, obsFtr, m, nobs};
        for (int p = 0, s, n; p < m; ++p) {
            se2gpu::point_segment(csr, p, s, n);
            for (int i = s; i < s + n; ++i) {
                if (!se2gpu::entry_valid(slots, obsFrame[i], obsFtr[i])) continue;
                std::vector<int32_t>& o = observations[obsFrame[i]];
                if (o.empty() || o.back() != p) o.push_back(p);      // points come in ascending order: a repeat is the last one
            }
        }
    }
    bool isNull(int p) const { return mpNull && mpNull[p]; }
    bool isGoodPrl(int p) const { return !goodPrl || goodPrl[p]; }
    bool hasObservation(int f, int p) const {                        // KeyFrame::hasObservation(pMP)
        return std::binary_search(observations[f].begin(), observations[f].end(), p);
    }
    int getSizeObsMP(int f) const { return (int)observations[f].size(); }   // KeyFrame.cpp:122-125: null points included
};

// Map.cpp:354-369.  common = spMPs, ascending.  Returns (nSameMP / size of a, nSameMP / size of b) in float; 0 / 0 is NaN.
inline Point2f compareViewMPs(const CovisHostView& view, int a, int b, std::vector<int>& common) {
    int nSameMP = 0;
    common.clear();
    for (int32_t p : view.observations[a]) {
        if (view.isNull(p)) continue;                                // getAllObsMPs(false), KeyFrame.cpp:152
        if (view.hasObservation(b, p)) {
            common.push_back(p);
            nSameMP++;
        }
    }
    Point2f r;
    r.x = (float)nSameMP / (float)view.getSizeObsMP(a);
    r.y = (float)nSameMP / (float)view.getSizeObsMP(b);
    return r;
}

// Map.cpp:373-400.  refs as the caller lists them (slots out of range are skipped, a slot listed twice counts twice: a
// std::set has no duplicates).  common = spMPsRet, ascending.  Returns the ratio, -1 when the key frame has no good point.
inline double compareViewMPs(const CovisHostView& view, int kf, const std::vector<int>& refs, std::vector<int>& common, int k) {
    common.clear();
    size_t nAll = 0;
    for (int32_t p : view.observations[kf]) {
        if (view.isNull(p) || !view.isGoodPrl(p)) continue;          // getAllObsMPs(): checkParallax = true (KeyFrame.h:69)
        ++nAll;
        int count = 0;
        for (int f : refs)
            if (f >= 0 && f < view.nframes && view.hasObservation(f, p)) count++;
        if (count >= k) common.push_back(p);
    }
    if (nAll == 0) return -1;
    return common.size() * 1.0 / nAll;
}

// Map.cpp:785-799: the slots of localKFs that newKF becomes covisible with (addCovisibleKF both ways is the caller's)
inline std::vector<int> updateCovisibility(const CovisHostView& view, int newKF, const std::vector<int>& localKFs) {
    std::vector<int> connect, spMPs;
    for (int kfi : localKFs) {
        compareViewMPs(view, newKF, kfi, spMPs);
        if (spMPs.size() > 0.3f * view.getSizeObsMP(newKF)) connect.push_back(kfi);   // :794, in float
    }
    return connect;
}

// Map.cpp:193-196
inline bool isRedundant(const CovisHostView& view, int kf, const std::vector<int>& covisKFs) {
    std::vector<int> spMPs;
    const double ratio = compareViewMPs(view, kf, covisKFs, spMPs, 2);
    return ratio >= 0.8;
}

// d_pair_out / d_job_out of the C ABI
struct CovisPair {
    int32_t nSame, sizeA, sizeB, flags;      // flags bit 0: Map.cpp:794 with ratioF, bit 1: Localizer.cpp:683 with ratioD
};
struct CovisJob {
    int32_t count, all, redundant;
};
struct CovisCommon {
    int32_t point, entryA, entryB;           // entries: indices into the CSR arrays (d_obs_view / d_obs_info rows)
};
static_assert(sizeof(CovisPair) == 16 && sizeof(CovisJob) == 12 && sizeof(CovisCommon) == 12, "the ints of the C ABI");

// The tables in device memory.  The caller owns every array; bits holds bitsWords() 64-bit words.
struct CovisibilityTable {
    int nframes = 0, cap = 0, M = 0, nobs = 0;
    const int32_t* counts = nullptr;
    const int32_t* mpPtr = nullptr;
    const int32_t* obsFrame = nullptr;
    const int32_t* obsFtr = nullptr;
    const uint8_t* mpNull = nullptr;         // may be null
    const uint8_t* goodPrl = nullptr;        // may be null
    uint64_t* bits = nullptr;                // work space: the observation sets as a bit matrix
    int32_t* sizeObs = nullptr;              // nframes: KeyFrame::getSizeObsMP()

    long long bitsWords() const { return se2gpu_covis_bits_words(nframes, M); }

    // Asynchronous on the matcher's stream, like the two calls below; matcher.sync() before outputs are read on the host.
    void build(ORBmatcher& matcher) {
        check(se2gpu_covis_build_device(matcher.handle(), counts, cap, nframes, mpPtr, obsFrame, obsFtr, M, nobs, mpNull, goodPrl,
                                        bits, sizeObs),
              "CovisibilityTable::build");
    }
    // compareViewMPs(pairA[p], pairB[p], spMPs) for npairs pairs; ratios: npairs x 2 floats; common (npairs x listCap, may be
    // null): the first listCap points of spMPs with their CSR entries, the input of FeatEdgeView
    void pairsBatchDevice(ORBmatcher& matcher, const int32_t* pairA, const int32_t* pairB, int npairs, float ratioF, double ratioD,
                          CovisPair* out, float* ratios, CovisCommon* common = nullptr, int listCap = 0) {
        check(se2gpu_covis_pairs_device(matcher.handle(), bits, nframes, M, pairA, pairB, npairs, ratioF, ratioD,
                                        reinterpret_cast<int32_t*>(out), ratios, reinterpret_cast<int32_t*>(common), listCap, counts,
                                        cap, mpPtr, obsFrame, obsFtr, nobs),
              "CovisibilityTable::pairsBatchDevice");
    }
    // compareViewMPs(jobKF[j], {refIdx[refPtr[j]] ..}, spMPsRet, k) for njobs jobs; redundant = ratio >= thresh
    void refsetBatchDevice(ORBmatcher& matcher, const int32_t* jobKF, const int32_t* refPtr, const int32_t* refIdx, int nref,
                           int njobs, int k, double thresh, CovisJob* out, double* ratios) {
        check(se2gpu_covis_refset_device(matcher.handle(), bits, nframes, M, jobKF, refPtr, refIdx, nref, njobs, k, thresh,
                                         reinterpret_cast<int32_t*>(out), ratios),
              "CovisibilityTable::refsetBatchDevice");
    }
};

}  // namespace se2lam_amd
