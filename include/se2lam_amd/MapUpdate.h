// The map's observation table under a new key frame and under a pruned one - header-only mirror, C++17, of
//   LocalMapper::findCorrespd's bookkeeping   src/LocalMapper.cpp:95-168   addObservation / setViewMP / insertMP
//   MapPoint::addObservation                  src/MapPoint.cpp:104-122     the normal vector (:115-117)
//   KeyFrame::setNull, MapPoint::eraseObservation, MapPoint::setNull   src/KeyFrame.cpp:100-113, src/MapPoint.cpp:54-101
//   applyObservations(tables)       the rules of se2gpu_map_apply_batch_device (include/se2gpu.h) on tables in HOST memory, on
//                                   one thread: the stand-in where no device copy exists and the baseline
//                                   tools/map_apply_bench.py times
//   MapObservationTable             the same tables in device memory: applyBatchDevice(matcher, ws, wsBytes)
// The normal vector is map_normal.h's text, which the kernel runs too; compile with -ffp-contract=off to get its roundings.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "../se2gpu.h"
#include "ORBmatcher.h"
#include "map_normal.h"
#include "obs_table.h"
#include "types.h"

namespace se2lam_amd {

// Every array of one call; the layouts are those of se2gpu_map_apply_batch_device.  Host pointers for applyObservations,
// device pointers for MapObservationTable.
struct MapApplyTables {
    // the frame slots
    const int32_t* counts = nullptr;
    int cap = 0, nframes = 0;
    const uint8_t* frameNull = nullptr;       // nframes, may be null: KeyFrame::isNull()
    // the table before the call, capacities mCap / nobsCap
    const int32_t* mpPtr = nullptr;           // mCap + 1
    const int32_t* obsFrame = nullptr;        // nobsCap
    const int32_t* obsFtr = nullptr;
    const float* obsView = nullptr;           // nobsCap x 3, may be null (then obsInfo and the two new ones are too)
    const float* obsInfo = nullptr;           // nobsCap x 9
    const int32_t* sizesIn = nullptr;         // {m_old, nobs_old}
    int mCap = 0, nobsCap = 0;
    // the jobs and the rows se2gpu_kf_correspd_batch_device left
    int B = 0;
    const int32_t* jobPrev = nullptr;
    const int32_t* jobNew = nullptr;
    const uint8_t* kind = nullptr;            // B * cap
    const int32_t* src = nullptr;
    const float* view = nullptr;              // x 3
    const float* info = nullptr;              // x 9
    const float* newPosW = nullptr;           // x 3, kind 3
    const float* infoPrev = nullptr;          // x 9, kind 3
    const float* localPos = nullptr;          // x 3, by the previous key frame's feature
    const uint8_t* goodPrlRow = nullptr;      // B * cap, by the previous key frame's feature
    int kinds = 14;                           // bit k: apply the rows of kind k
    const int32_t* parallaxStatus = nullptr;  // mCap, may be null: 2 = abandoned by MapPoint::updateParallax
    // in place, per point
    float* pos = nullptr;
    uint8_t* goodPrl = nullptr;
    uint8_t* mpNull = nullptr;
    float* mpNormal = nullptr;
    // in place, per feature
    int32_t* ftrMP = nullptr;                 // mDualObservations: the point's slot or -1
    uint8_t* kfObserved = nullptr;
    float* viewPos = nullptr;
    float* viewInfo = nullptr;
    // out
    int32_t* mpPtrNew = nullptr;
    int32_t* obsFrameNew = nullptr;
    int32_t* obsFtrNew = nullptr;
    float* obsViewNew = nullptr;
    float* obsInfoNew = nullptr;
    int32_t* newFrame = nullptr;              // mCap
    int32_t* sizesOut = nullptr;              // 9: SE2GPU_MAP_APPLY_* of se2gpu.h
    int32_t* jobCounts = nullptr;             // B x 6
};

// The rules of se2gpu_map_apply_batch_device on host tables; returns sizesOut[0].
inline int applyObservations(const MapApplyTables& t) {
    using namespace se2gpu;
    const int cap = t.cap, B = t.B;
    const FrameSlots fs{t.counts, nullptr, cap, t.nframes};       // the range half of the entry rule; null frames are erased, below
    const int mOld = ot_min(ot_max(t.sizesIn[0], 0), t.mCap), nobsOld = ot_min(ot_max(t.sizesIn[1], 0), t.nobsCap);
    const ObsCsr old{t.mpPtr, t.obsFrame, t.obsFtr, mOld, nobsOld};
    auto fnull = [&](int f) { return t.frameNull && t.frameNull[f]; };
    auto dead = [&](int p) { return t.mpNull[p] || (t.parallaxStatus && t.parallaxStatus[p] == 2); };
    long long st[SE2GPU_MAP_APPLY_NSIZES] = {0};
    for (int i = 0; i < 6 * B; ++i) t.jobCounts[i] = 0;

    // what is needed, without a write in place
    std::vector<int32_t> len(mOld, 0);                             // entries kept, then with those appended
    std::vector<uint8_t> nullAfter(mOld, 0);
    for (int p = 0; p < mOld; ++p) {
        int s, e, ok = 0, kept = 0;
        point_range(old, p, s, e);
        for (int i = s; i < e; ++i) {
            if (entry_offset(fs, old, i) < 0) continue;
            ++ok;
            if (!fnull(t.obsFrame[i])) ++kept;
        }
        if (dead(p)) kept = 0;
        st[SE2GPU_MAP_APPLY_ERASED] += ot_max(e - s, 0) - kept;
        nullAfter[p] = kept == 0;
        if (kept == 0 && !t.mpNull[p]) ++st[SE2GPU_MAP_APPLY_NULLED];
        len[p] = kept;
    }
    struct Row { int key, j; };                                    // key: the point (kinds 1, 2) or src (kind 3)
    std::vector<std::vector<Row>> add(B), born(B);
    std::vector<std::pair<int, int>> skipped;                      // (job, j)
    auto skip = [&](int b, int j, bool dup) {
        skipped.push_back({b, j});
        ++st[SE2GPU_MAP_APPLY_SKIPPED];
        ++t.jobCounts[6 * b + 4];
        if (dup) { ++st[SE2GPU_MAP_APPLY_DUP]; ++t.jobCounts[6 * b + 5]; }
    };
    auto winners = [&](int b, std::vector<Row>& rows) {            // the greatest j of a key wins; ascending keys
        std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& c) { return a.key != c.key ? a.key < c.key : a.j > c.j; });
        size_t n = 0;
        for (size_t i = 0; i < rows.size(); ++i) {
            if (i && rows[i].key == rows[i - 1].key) { skip(b, rows[i].j, true); continue; }
            rows[n++] = rows[i];
        }
        rows.resize(n);
    };
    for (int b = 0; b < B; ++b) {
        const int fp = t.jobPrev[b], fn = t.jobNew[b];
        if ((unsigned)fp >= (unsigned)t.nframes || (unsigned)fn >= (unsigned)t.nframes || fp == fn || fnull(fp) || fnull(fn)) {
            t.jobCounts[6 * b] = 1;
            continue;
        }
        const size_t row = (size_t)b * cap;
        const int nNew = feature_count(fs, fn), nPrev = feature_count(fs, fp);
        for (int j = 0; j < nNew; ++j) {
            const int k = t.kind[row + j], i = t.src[row + j];
            if (k < 1 || k > 3 || !((t.kinds >> k) & 1)) continue;
            if (k == 3) {
                if (i >= 0 && i < nPrev) born[b].push_back({i, j}); else skip(b, j, false);
                continue;
            }
            const int p = k == 2 ? i : (i >= 0 && i < nPrev ? t.ftrMP[(size_t)fp * cap + i] : -1);   // getObservation(i) (:97)
            if (p >= 0 && p < mOld) add[b].push_back({p, j}); else skip(b, j, false);
        }
        winners(b, add[b]);
        winners(b, born[b]);
        size_t n = 0;
        for (const Row& r : add[b]) {
            bool refuse = nullAfter[r.key];                        // KeyFrame::addObservation returns on a null point (:197)
            int s, e;
            point_range(old, r.key, s, e);
            for (int i = s; i < e && !refuse; ++i)                 // std::map::insert keeps the old entry (:108)
                refuse = entry_offset(fs, old, i) >= 0 && t.obsFrame[i] == fn;
            if (refuse) { skip(b, r.j, false); continue; }
            add[b][n++] = r;
            ++len[r.key];
            ++t.jobCounts[6 * b + t.kind[row + r.j]];
        }
        add[b].resize(n);
        t.jobCounts[6 * b + 3] = (int32_t)born[b].size();
        st[SE2GPU_MAP_APPLY_ADDED] += (long long)n + 2 * (long long)born[b].size();
        st[SE2GPU_MAP_APPLY_CREATED] += (long long)born[b].size();
    }
    long long mNew = mOld + st[SE2GPU_MAP_APPLY_CREATED], nobsNew = 2 * st[SE2GPU_MAP_APPLY_CREATED];
    for (int p = 0; p < mOld; ++p) nobsNew += len[p];
    st[SE2GPU_MAP_APPLY_M_NEW] = mNew;
    st[SE2GPU_MAP_APPLY_NOBS_NEW] = nobsNew;
    st[SE2GPU_MAP_APPLY_STATUS] = mNew > t.mCap || nobsNew > t.nobsCap ? 2 : 0;
    for (int i = 0; i < SE2GPU_MAP_APPLY_NSIZES; ++i) t.sizesOut[i] = (int32_t)st[i];
    if (st[SE2GPU_MAP_APPLY_STATUS]) return 2;                     // nothing in place has been modified

    // the writes.  KeyFrame::setNull clears the key frame's own containers (KeyFrame.cpp:110-111)
    const bool rows = t.obsView && t.obsInfo && t.obsViewNew && t.obsInfoNew;
    for (int f = 0; f < t.nframes; ++f)
        if (fnull(f))
            for (size_t o = (size_t)f * cap; o < (size_t)(f + 1) * cap; ++o) { t.ftrMP[o] = -1; t.kfObserved[o] = 0; }
    std::vector<int32_t> cursor(mOld);
    int32_t at = 0;
    for (int p = 0; p < mOld; ++p) {
        t.mpPtrNew[p] = cursor[p] = at;
        at += len[p];
        t.newFrame[p] = -1;
        int s, e, size = 0;
        point_range(old, p, s, e);
        const bool gone = dead(p);
        for (int i = s; i < e; ++i) size += entry_offset(fs, old, i) >= 0;
        for (int i = s; i < e; ++i) {
            const int o = entry_offset(fs, old, i);
            if (o < 0) continue;
            if (gone) {                                            // MapPoint::setNull -> pKF->eraseObservation(idx) (:73-74)
                t.ftrMP[o] = -1;
                t.kfObserved[o] = 0;
            } else if (fnull(t.obsFrame[i])) {                     // MapPoint::eraseObservation (:86-101)
                if (--size > 0) normal_erase(t.mpNormal + 3 * (size_t)p, t.viewPos + 3 * (size_t)o, size);
            } else {
                const int32_t d = cursor[p]++;
                t.obsFrameNew[d] = t.obsFrame[i];
                t.obsFtrNew[d] = t.obsFtr[i];
                if (rows) {
                    std::copy(t.obsView + 3 * (size_t)i, t.obsView + 3 * (size_t)i + 3, t.obsViewNew + 3 * (size_t)d);
                    std::copy(t.obsInfo + 9 * (size_t)i, t.obsInfo + 9 * (size_t)i + 9, t.obsInfoNew + 9 * (size_t)d);
                }
            }
        }
        if (nullAfter[p]) { t.mpNull[p] = 1; t.goodPrl[p] = 0; }   // :56-57, :93-94
    }
    auto entry = [&](int32_t d, int f, int k, const float* v, const float* I) {
        t.obsFrameNew[d] = f;
        t.obsFtrNew[d] = k;
        if (rows) {
            std::copy(v, v + 3, t.obsViewNew + 3 * (size_t)d);
            std::copy(I, I + 9, t.obsInfoNew + 9 * (size_t)d);
        }
    };
    auto feature = [&](int f, int k, int p, const float* v, const float* I) {   // setViewMP and KeyFrame::addObservation
        const size_t o = (size_t)f * cap + k;
        std::copy(v, v + 3, t.viewPos + 3 * o);
        std::copy(I, I + 9, t.viewInfo + 9 * o);
        t.ftrMP[o] = p;
        t.kfObserved[o] = 1;
    };
    int32_t slot = mOld;
    for (int b = 0; b < B; ++b) {
        const int fp = t.jobPrev[b], fn = t.jobNew[b];
        const size_t row = (size_t)b * cap;
        for (const Row& r : add[b]) {                              // :103-105, :138-140
            const int p = r.key;
            const int32_t d = cursor[p]++;
            const float *v = t.view + 3 * (row + r.j), *I = t.info + 9 * (row + r.j);
            normal_add(t.mpNormal + 3 * (size_t)p, v, d - t.mpPtrNew[p]);
            entry(d, fn, r.j, v, I);
            feature(fn, r.j, p, v, I);
            t.newFrame[p] = fn;
        }
        for (const Row& r : born[b]) {                             // :150-165, in the order of the previous key frame's features
            const int p = slot++, i = r.key;
            const float *v = t.view + 3 * (row + r.j), *I = t.info + 9 * (row + r.j);
            const float *lp = t.localPos + 3 * (row + i), *Ip = t.infoPrev + 9 * (row + r.j);
            t.mpPtrNew[p] = at;
            std::copy(t.newPosW + 3 * (row + r.j), t.newPosW + 3 * (row + r.j) + 3, t.pos + 3 * (size_t)p);
            t.goodPrl[p] = t.goodPrlRow[row + i] ? 1 : 0;
            t.mpNull[p] = 0;
            float* nv = t.mpNormal + 3 * (size_t)p;
            nv[0] = nv[1] = nv[2] = 0.f;
            normal_add(nv, lp, 0);
            normal_add(nv, v, 1);
            entry(at, fp, i, lp, Ip);
            entry(at + 1, fn, r.j, v, I);
            feature(fp, i, p, lp, Ip);
            feature(fn, r.j, p, v, I);
            t.newFrame[p] = fn;
            at += 2;
        }
    }
    for (const auto& s : skipped) t.kfObserved[(size_t)t.jobNew[s.first] * cap + s.second] = 0;
    for (int p = slot; p <= t.mCap; ++p) {                         // padding: empty segments, null points
        t.mpPtrNew[p] = at;
        if (p < t.mCap) { t.mpNull[p] = 1; t.goodPrl[p] = 0; t.newFrame[p] = -1; }
    }
    return 0;
}

// The tables in device memory.  ws: se2gpu_map_apply_ws_bytes(B, cap, mCap, nobsCap) bytes, 16-byte aligned.
struct MapObservationTable : MapApplyTables {
    static long long workspaceBytes(int B, int cap, int mCap, int nobsCap) { return se2gpu_map_apply_ws_bytes(B, cap, mCap, nobsCap); }

    // asynchronous on the matcher's stream; sizesOut + 1 can be the next call's sizesIn
    void applyBatchDevice(ORBmatcher& matcher, void* ws, long long wsBytes) {
        check(se2gpu_map_apply_batch_device(matcher.handle(), counts, cap, nframes, frameNull, mpPtr, obsFrame, obsFtr, obsView,
                                            obsInfo, sizesIn, mCap, nobsCap, jobPrev, jobNew, B, kind, src, view, info, newPosW,
                                            infoPrev, localPos, goodPrlRow, kinds, parallaxStatus, pos, goodPrl, mpNull, mpNormal,
                                            ftrMP, kfObserved, viewPos, viewInfo, mpPtrNew, obsFrameNew, obsFtrNew, obsViewNew,
                                            obsInfoNew, newFrame, sizesOut, jobCounts, ws, wsBytes),
              "MapObservationTable::applyBatchDevice");
    }
};

}  // namespace se2lam_amd
