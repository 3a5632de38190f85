// The 7-point samples of cv::findFundamentalMat's registrators (PointSetRegistrator::getSubset, ptsetreg.cpp): 7 distinct
// indices in 0..n-1 by rejection, cv::RNG(-1), one generator for the whole run.  They depend on the point count alone.
//
// The generator is a multiply-with-carry whose raw 32-bit stream does not depend on n; only the reduction `raw % n` and the
// accept scan do.  So the first kFmRawTable raw values are data (fm_raw_fill, uploaded once per handle); past the table's
// end the walk continues the recurrence from the state after the table.  A draw walks the stream a window of 128 values
// at a time, and what is serial in it is short:
//   reduce   the values mod n: the whole table once, up front; behind it a window at a time, two values per lane
//   scan     every lane runs getSubset's accept scan for a sample that would START at its stream position: the 7 indices
//            and where the sample after it would start.  No lane knows yet whether a sample really starts there.
//   chase    the true starts are the orbit of the window's first position under "start of the next sample": a walk of about
//            64 / 7 hops over one register per lane.  The lanes on the orbit store their samples.
// The next window starts where the chase stopped.  A sample that does not end inside its window (more than 57 rejections
// among its draws; not seen for any n, but nothing rules it out) goes through the plain serial scan, which carries a
// half-drawn sample from window to window, and the lanes take over again behind it.
//
// One function for both sides: plain C++ for the host compiler, where the "lanes" are a loop (tests/cpp_fm_subsets.cpp),
// __host__ __device__ under hipcc, where one wave of 64 calls it together (ransac.hip).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FM_HD __host__ __device__
#else
#define FM_HD
#endif

namespace se2gpu {

// raw values held as a table: 1000 samples take 7,000 raw values without a rejection and about 9,000 at n = 15; the
// remainder of a long draw (small n) is generated on the fly
constexpr int kFmRawTable = 8192;
constexpr int kFmModelPoints = 7;
constexpr int kFmWindow = 128;                  // stream values per round; samples start in its first 64
constexpr uint64_t kFmRngSeed = ~(uint64_t)0;   // cv::RNG(-1)

// cv::RNG::next: the new state; its low word is the value drawn
FM_HD inline uint64_t fm_rng_step(uint64_t s) { return (uint64_t)(uint32_t)s * 4164903690u + (uint32_t)(s >> 32); }

// the first `len` raw values of cv::RNG(-1) -> the generator state after them
inline uint64_t fm_raw_fill(uint32_t* table, int len) {
    uint64_t s = kFmRngSeed;
    for (int i = 0; i < len; ++i) {
        s = fm_rng_step(s);
        table[i] = (uint32_t)s;
    }
    return s;
}

// getSubset's accept step: v joins idx[0..have-1] unless it is among them
FM_HD inline void fm_accept(int idx[kFmModelPoints], int& have, int v) {
    bool seen = false;
    for (int q = 0; q < kFmModelPoints; ++q) seen = seen || (q < have && idx[q] == v);
    if (seen) return;
    for (int q = 0; q < kFmModelPoints; ++q)
        if (q == have) idx[q] = v;
    ++have;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define FM_SLOTS 1                        // a thread holds the state of its own lane
#define FM_LANE_OF(slot) lane
#define FM_SYNC() __syncthreads()         // the caller is a workgroup of one wave
#else
#define FM_SLOTS 64                       // the host holds all 64 and loops
#define FM_LANE_OF(slot) (slot)
#define FM_SYNC() ((void)0)
#endif

// subsets[it * 7 + 0..6] for it < niters, exactly what `niters` calls of getSubset on one cv::RNG(-1) give for n points.
// table[0..len-1] = the raw stream's head, state_after = the generator state behind it (fm_raw_fill).
// On the device the 64 threads of a one-wave workgroup call this together with the same arguments and their own `lane`;
// the host calls it once (lane is ignored).  serial_only takes every window through the serial scan (for tests).
// n < 7 has no sample: nothing is written.
FM_HD inline void fm_draw_subsets(const uint32_t* table, int len, uint64_t state_after, int n, int niters, int* subsets,
                                  int lane, bool serial_only = false) {
    if (n < kFmModelPoints) return;
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ int red[kFmRawTable], win[kFmWindow];
#else
    int red[kFmRawTable], win[kFmWindow];
#endif
    // reduce, for the table: red[p] = table[p] % n, once, with all loads in flight together
    const int pre = len < kFmRawTable ? len : kFmRawTable;
    for (int s = 0; s < FM_SLOTS; ++s)
        for (int p = FM_LANE_OF(s); p < pre; p += 64) red[p] = (int)(table[p] % (uint32_t)n);
    int carry[kFmModelPoints] = {0, 0, 0, 0, 0, 0, 0};   // a sample the serial scan has begun (uniform)
    int have = 0, it = 0;
    int base = 0;                 // stream position of the window's first value
    uint64_t state = state_after; // generator state in front of position max(base, len)
    while (it < niters) {
        const int* src = red + base;
        FM_SYNC();
        if (base + kFmWindow > pre) {
            // reduce, behind the table: win[k] = raw(base + k) % n
            const int in_table = len - base < 0 ? 0 : (len - base > kFmWindow ? kFmWindow : len - base);
            for (int s = 0; s < FM_SLOTS; ++s) {
                const int l = FM_LANE_OF(s);
                uint32_t r0 = l < in_table ? table[base + l] : 0u, r1 = l + 64 < in_table ? table[base + l + 64] : 0u;
                uint64_t g = state;
                for (int k = in_table; k < kFmWindow; ++k) {
                    g = fm_rng_step(g);
                    if (k == l) r0 = (uint32_t)g;
                    if (k == l + 64) r1 = (uint32_t)g;
                }
                win[l] = (int)(r0 % (uint32_t)n);
                win[l + 64] = (int)(r1 % (uint32_t)n);
            }
            src = win;
            FM_SYNC();
        }
        int advance = 0;
        if (have == 0 && !serial_only) {
            // scan: the sample that would start at base + l
            int idx[FM_SLOTS][kFmModelPoints], next[FM_SLOTS];
            uint64_t complete = 0;
            for (int s = 0; s < FM_SLOTS; ++s) {
                const int l = FM_LANE_OF(s);
                int h = 0, k = l + kFmModelPoints, first[kFmModelPoints];
                for (int q = 0; q < kFmModelPoints; ++q) idx[s][q] = 0;
                for (int q = 0; q < kFmModelPoints; ++q) first[q] = src[l + q];   // a sample takes 7 values at least
                for (int q = 0; q < kFmModelPoints; ++q) fm_accept(idx[s], h, first[q]);
                while (h < kFmModelPoints && k < kFmWindow) fm_accept(idx[s], h, src[k++]);
                next[s] = k;
#if defined(__HIP_DEVICE_COMPILE__)
                complete = __ballot(h == kFmModelPoints);
#else
                complete |= (uint64_t)(h == kFmModelPoints) << l;
#endif
            }
            // chase: the starts of the samples it, it + 1, .. among the window's first 64 positions
            uint64_t starts = 0;
            int count = 0;
            while (advance < 64 && ((complete >> advance) & 1) && it + count < niters) {
                starts |= (uint64_t)1 << advance;
                ++count;
#if defined(__HIP_DEVICE_COMPILE__)
                advance = __builtin_amdgcn_readlane(next[0], advance);
#else
                advance = next[advance];
#endif
            }
            for (int s = 0; s < FM_SLOTS; ++s) {
                const int l = FM_LANE_OF(s);
                if (!((starts >> l) & 1)) continue;
                int rank = 0;   // samples that start in front of this one
                for (uint64_t m = starts & (((uint64_t)1 << l) - 1); m; m &= m - 1) ++rank;
                for (int q = 0; q < kFmModelPoints; ++q) subsets[(it + rank) * kFmModelPoints + q] = idx[s][q];
            }
            it += count;
        }
        if (advance == 0) {
            // serial: one accept scan from the window's start (every lane runs it, lane 0 stores)
            int k = 0;
            while (k < kFmWindow && it < niters) {
                fm_accept(carry, have, src[k++]);
                if (have < kFmModelPoints) continue;
                if (FM_LANE_OF(0) == 0)
                    for (int q = 0; q < kFmModelPoints; ++q) subsets[it * kFmModelPoints + q] = carry[q];
                have = 0;
                ++it;
                if (!serial_only) break;   // the next window starts behind this sample and is scanned by the lanes again
            }
            advance = k;
        }
        // the generator state follows the window's base
        const int from = base > len ? base : len;
        for (int p = from; p < base + advance; ++p) state = fm_rng_step(state);
        base += advance;
    }
}

#undef FM_SLOTS
#undef FM_LANE_OF
#undef FM_SYNC

}  // namespace se2gpu
