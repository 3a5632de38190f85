// The observation table of mappoint.hip, new_kf.hip and covis.hip (through csrc/obs_table.h) and of their host mirrors
// MapPointMain.h, FindCorrespd.h and Covisibility.h: a CSR over map points laid over a set of frame slots.  The same text
// compiles for the device and for the host, so the two rules have one definition:
//   the entry rule    (f, k) counts when f lies in 0..nframes-1, the frame is not null and k lies in 0..min(counts[f], cap)-1
//   the segment rule  mp_ptr[p] and mp_ptr[p + 1] are clamped to 0..nobs, and a descending segment is empty
// so nothing is indexed outside the arrays whatever they hold.  Self-contained: <cstdint> only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SE2_OT_FN __host__ __device__ __forceinline__
#else
#define SE2_OT_FN inline
#endif

namespace se2gpu {

struct FrameSlots {
    const int32_t* counts;       // nframes: features of a frame (a count beyond cap means cap)
    const uint8_t* frame_null;   // nframes, may be null: frames whose observations do not count
    int cap, nframes;
};

SE2_OT_FN int ot_min(int a, int b) { return a < b ? a : b; }
SE2_OT_FN int ot_max(int a, int b) { return a > b ? a : b; }

// the features of frame f that exist; f must lie in 0..nframes-1
SE2_OT_FN int feature_count(const FrameSlots& fs, int f) { return ot_min(fs.counts[f], fs.cap); }

// The entry rule.  frame_null is set by updateMainKFandDescriptor alone, which skips null key frames as the reference does
// (MapPoint.cpp:242); updateParallax and compareViewMPs do not, and pass nullptr.
SE2_OT_FN bool entry_valid(const FrameSlots& fs, int f, int k) {
    if ((unsigned)f >= (unsigned)fs.nframes) return false;
    if (fs.frame_null && fs.frame_null[f]) return false;
    const int c = feature_count(fs, f);   // read before k is looked at: this load does not wait for the one k came from
    return k >= 0 && k < c;
}

// feature index f * cap + k of a valid entry, -1 of one to skip; an int on the host too: nframes * cap <= INT_MAX is the C ABI's
// condition (check_frame_slots), and the host mirrors read the same arrays under it
SE2_OT_FN int feature_offset(const FrameSlots& fs, int f, int k) { return entry_valid(fs, f, k) ? f * fs.cap + k : -1; }

struct ObsCsr {
    const int32_t* mp_ptr;      // m + 1
    const int32_t* obs_frame;   // nobs, container order within a point
    const int32_t* obs_ftr;     // nobs
    int m, nobs;
};

// feature_offset of the entry at place i of the observation arrays
SE2_OT_FN int entry_offset(const FrameSlots& fs, const ObsCsr& c, int i) { return feature_offset(fs, c.obs_frame[i], c.obs_ftr[i]); }

// The segment rule: the entries s..e-1 of point p, both ends clamped to the arrays; e <= s is an empty list.
SE2_OT_FN void point_range(const ObsCsr& c, int p, int& s, int& e) {
    s = ot_min(ot_max(c.mp_ptr[p], 0), c.nobs);
    e = ot_min(ot_max(c.mp_ptr[p + 1], 0), c.nobs);
}

// the same as n entries from s, for a caller that deals the places 0..n-1 of a list to its lanes
SE2_OT_FN void point_segment(const ObsCsr& c, int p, int& s, int& n) {
    int e;
    point_range(c, p, s, e);
    n = ot_max(e - s, 0);
}

}  // namespace se2gpu
