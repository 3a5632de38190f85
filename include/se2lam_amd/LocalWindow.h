// Local window - header-only mirror, C++17, of
//   KeyFrame::addCovisibleKF in both directions   LocalMapper.cpp:66-67, Map.cpp:233-234, :337-338, :794-797   connect(view, a, b)
//   the covisibility part of KeyFrame::setNull     src/KeyFrame.cpp:106-114                                      disconnect(view, s)
//   Map::updateLocalGraph                          src/Map.cpp:285-331                                           updateLocalGraph(view, cur, ...)
// on sets in HOST memory, written as the reference writes them - one std::set per key frame and per map point, the sets of
// the window ordered by id - and sharing nothing with the kernels' bit matrices: the CPU stand-in where no device copy exists.
//   LocalWindowTable   the same for batches in device memory, next to CovisibilityTable (se2gpu_covis_connect_device /
//                      _disconnect_device, se2gpu_local_window_batch_device)
// Key frames are slots 0..nframes-1, map points indices 0..m-1.
#pragma once
#include <cstdint>
#include <set>
#include <vector>

#include "../se2gpu.h"
#include "Covisibility.h"
#include "ORBmatcher.h"

namespace se2lam_amd {

struct LocalWindowHostView {
    std::vector<int> kfId;                           // KeyFrame::mIdKF per slot
    std::vector<int> mpId;                           // MapPoint::mId per point
    std::vector<std::set<int>> covisibleKFs;         // KeyFrame::mCovisibleKFs per slot
    std::vector<std::set<int>> kfObservations;       // KeyFrame::mObservations per slot: points
    std::vector<std::set<int>> mpObservations;       // MapPoint::mObservations per point: slots
    std::vector<uint8_t> kfNull, mpNull;             // isNull(); empty = none is null

    bool isNullKF(int f) const { return !kfNull.empty() && kfNull[f]; }
    bool isNullMP(int p) const { return !mpNull.empty() && mpNull[p]; }
    // KeyFrame::getAllObsMPs(false), KeyFrame.cpp:146-158
    std::set<int> getAllObsMPs(int f) const {
        std::set<int> r;
        for (int p : kfObservations[f])
            if (!isNullMP(p)) r.insert(p);
        return r;
    }
    // MapPoint::getObservations(), MapPoint.cpp:211-220
    std::set<int> getObservations(int p) const {
        std::set<int> r;
        for (int f : mpObservations[p])
            if (!isNullKF(f)) r.insert(f);
        return r;
    }
};

inline void connect(LocalWindowHostView& view, int a, int b) {
    view.covisibleKFs[a].insert(b);                  // pKFa->addCovisibleKF(pKFb)
    view.covisibleKFs[b].insert(a);                  // pKFb->addCovisibleKF(pKFa)
}

// KeyFrame.cpp:106-114
inline void disconnect(LocalWindowHostView& view, int s) {
    for (int b : view.covisibleKFs[s]) {
        if (b != s) view.covisibleKFs[b].erase(s);   // pKF->eraseCovisibleKF(shared_from_this()); the own entry goes with clear()
    }
    view.covisibleKFs[s].clear();
}

// Map.cpp:285-331 with mCurrentKF = cur.  The three vectors are mLocalGraphKFs, mRefKFs and mLocalGraphMPs as slots / points,
// in IdLessThan order.  Returns the number of EdgeSE2XYZ Map::loadLocalGraph would create from them (:1005-1051).
inline int updateLocalGraph(const LocalWindowHostView& view, int cur, std::vector<int>& localKFs, std::vector<int>& refKFs,
                            std::vector<int>& localMPs, int searchLevel = 3) {
    struct IdLess {
        const std::vector<int>* id;
        bool operator()(int a, int b) const { return (*id)[a] < (*id)[b]; }
    };
    std::set<int, IdLess> setLocalKFs(IdLess{&view.kfId}), setRefKFs(IdLess{&view.kfId});
    std::set<int, IdLess> setLocalMPs(IdLess{&view.mpId});

    setLocalKFs.insert(cur);

    while (searchLevel > 0) {
        std::set<int, IdLess> currentLocalKFs = setLocalKFs;
        for (auto i = currentLocalKFs.begin(), iend = currentLocalKFs.end(); i != iend; i++) {
            const std::set<int>& pKFs = view.covisibleKFs[*i];
            setLocalKFs.insert(pKFs.begin(), pKFs.end());
        }
        searchLevel--;
    }

    for (auto i = setLocalKFs.begin(), iend = setLocalKFs.end(); i != iend; i++) {
        std::set<int> pMPs = view.getAllObsMPs(*i);
        setLocalMPs.insert(pMPs.begin(), pMPs.end());
    }

    int nObs = 0;
    for (auto i = setLocalMPs.begin(), iend = setLocalMPs.end(); i != iend; i++) {
        std::set<int> pKFs = view.getObservations(*i);
        nObs += (int)pKFs.size();                    // every observer ends in one of the two sets
        for (auto j = pKFs.begin(), jend = pKFs.end(); j != jend; j++) {
            if (setLocalKFs.find(*j) != setLocalKFs.end() || setRefKFs.find(*j) != setRefKFs.end()) continue;
            setRefKFs.insert(*j);
        }
    }

    localKFs.assign(setLocalKFs.begin(), setLocalKFs.end());
    refKFs.assign(setRefKFs.begin(), setRefKFs.end());
    localMPs.assign(setLocalMPs.begin(), setLocalMPs.end());
    return nObs;
}

// d_win_out of the C ABI
struct LocalWindowCounts {
    int32_t nLocal, nRef, nMP, nObs;
};
static_assert(sizeof(LocalWindowCounts) == 16, "the ints of the C ABI");

// The covisibility graph in device memory next to the observation bits of a CovisibilityTable.  The caller owns every array:
// adj holds adjWords() 64-bit words and is zeroed by the caller once.
struct LocalWindowTable {
    int nframes = 0, M = 0;
    uint64_t* adj = nullptr;                 // KeyFrame::mCovisibleKFs as a bit matrix, directed
    const uint64_t* bitsKF = nullptr;        // CovisibilityTable::bits built from the key frame's side
    const uint64_t* bitsMP = nullptr;        // the same from MapPoint::mObservations; where the sides agree, = bitsKF
    const uint8_t* frameNull = nullptr;      // may be null
    const int32_t* kfOrder = nullptr;        // slots by ascending mIdKF, may be null (index order)
    const int32_t* mpOrder = nullptr;        // points by ascending mId, may be null

    long long adjWords() const { return se2gpu_covis_adj_words(nframes); }
    void attach(const CovisibilityTable& t) {
        nframes = t.nframes; M = t.M; bitsKF = t.bits; bitsMP = t.bits;
    }

    // Asynchronous on the matcher's stream; matcher.sync() before outputs are read on the host.
    // addCovisibleKF both ways; pairOut null: every pair, else those CovisibilityTable::pairsBatchDevice flagged with flagMask
    void connect(ORBmatcher& matcher, const int32_t* pairA, const int32_t* pairB, int npairs, const CovisPair* pairOut = nullptr,
                 int flagMask = 1) {
        check(se2gpu_covis_connect_device(matcher.handle(), adj, nframes, pairA, pairB, npairs,
                                          reinterpret_cast<const int32_t*>(pairOut), flagMask),
              "LocalWindowTable::connect");
    }
    void disconnect(ORBmatcher& matcher, const int32_t* slots, int nslots) {
        check(se2gpu_covis_disconnect_device(matcher.handle(), adj, nframes, slots, nslots), "LocalWindowTable::disconnect");
    }
    // Map::updateLocalGraph for njobs current key frames; winKF: njobs x 2 x ceil(nframes / 64) words, winMP: njobs x
    // ceil(M / 64); the lists (may be null) hold kfListCap / mpListCap ints per job
    void updateLocalGraphBatchDevice(ORBmatcher& matcher, const int32_t* jobKF, int njobs, int searchLevel, uint64_t* winKF,
                                     uint64_t* winMP, LocalWindowCounts* out, int32_t* localList = nullptr,
                                     int32_t* refList = nullptr, int kfListCap = 0, int32_t* mpList = nullptr, int mpListCap = 0) {
        check(se2gpu_local_window_batch_device(matcher.handle(), bitsKF, bitsMP, nframes, M, adj, frameNull, jobKF, njobs,
                                               searchLevel, kfOrder, mpOrder, winKF, winMP, reinterpret_cast<int32_t*>(out),
                                               localList, refList, kfListCap, mpList, mpListCap),
              "LocalWindowTable::updateLocalGraphBatchDevice");
    }
};

}  // namespace se2lam_amd
