"""The specification of the local-window calls (se2gpu_covis_connect_device, se2gpu_covis_disconnect_device,
se2gpu_local_window_batch_device, include/se2gpu.h) as Python sets: KeyFrame::mCovisibleKFs as one set of slots per key frame,
KeyFrame::mObservations and MapPoint::mObservations as sets built from the two observation CSRs by the validity rule
(tests/covis_model.py), and Map::updateLocalGraph (src/Map.cpp:298-326 of the reference) restated on them as it is written.
No bit matrix and no bit tricks: rows are only packed at the end, for the comparison with the device's words."""
import numpy as np

import covis_model as cm

ISENT = cm.ISENT
WSENT = 0xA5A5A5A5A5A5A5A5


def pack(sets, n):
    """sets of indices -> (len(sets), ceil(n / 64)) uint64 rows, for comparisons only"""
    WN = (n + 63) // 64
    rows = np.zeros((len(sets), WN * 64), np.uint8)
    for r, s in enumerate(sets):
        rows[r, sorted(s)] = 1
    return np.packbits(rows, axis=1, bitorder="little").view(np.uint64).reshape(len(sets), WN)


def connect(adj, pair_a, pair_b, pair_out=None, flag_mask=1):
    """addCovisibleKF both ways on adj (a list of sets, changed in place); pairs out of range are skipped"""
    n = len(adj)
    for p, (a, b) in enumerate(zip(pair_a, pair_b)):
        if not (0 <= a < n and 0 <= b < n):
            continue
        if pair_out is not None and not (int(pair_out[p][3]) & flag_mask):
            continue
        adj[a].add(int(b))
        adj[b].add(int(a))
    return adj


def disconnect(adj, slots):
    """KeyFrame::setNull's covisibility part (KeyFrame.cpp:106-114), one call after the other in the order listed"""
    n = len(adj)
    for s in slots:
        if not 0 <= s < n:
            continue
        for b in list(adj[s]):
            adj[b].discard(s)          # pKF->eraseCovisibleKF(shared_from_this())
        adj[s].clear()                 # mCovisibleKFs.clear()
    return adj


class Model:
    """kf_obs[f]: the points of key frame slot f's mObservations (the key frame's side); mp_obs[p]: the key frame slots of point
    p's mObservations (the point's side, None = the same CSR); adj[f]: mCovisibleKFs of slot f"""

    def __init__(self, tables_kf, adj, tables_mp=None, frame_null=None):
        kf = cm.Model(*tables_kf)
        mp = kf if tables_mp is None else cm.Model(*tables_mp)
        self.nframes, self.m = kf.nframes, kf.m
        assert (mp.nframes, mp.m) == (kf.nframes, kf.m) and len(adj) == kf.nframes
        self.kf_obs = kf.sets
        self.notnull = kf.notnull
        self.mp_obs = [set() for _ in range(self.m)]
        for f, pts in enumerate(mp.sets):
            for p in pts:
                self.mp_obs[p].add(f)
        self.adj = [set(int(b) for b in a if 0 <= b < self.nframes) for a in adj]
        self.frame_null = [False] * self.nframes if frame_null is None else [bool(x) for x in frame_null]
        self._memo = {}                                             # (cur, search_level) -> the answer, computed once

    def update_local_graph(self, cur, search_level=3):
        """Map.cpp:298-326 -> (setLocalKFs, setRefKFs, setLocalMPs, the number of EdgeSE2XYZ of Map.cpp:1005-1051)"""
        if (cur, search_level) in self._memo:
            return self._memo[(cur, search_level)]
        local = {cur}                                               # :297
        level = search_level
        while level > 0:                                            # :300
            current = set(local)                                    # :301, the copy
            for kf in current:                                      # :302
                local |= self.adj[kf]                               # :304-305
            level -= 1
        mps = set()
        for kf in local:                                            # :310
            mps |= {p for p in self.kf_obs[kf] if p in self.notnull}   # getAllObsMPs(false), KeyFrame.cpp:152
        refs = set()
        for p in mps:                                               # :318
            for kf in self.mp_obs[p]:                               # getObservations()
                if self.frame_null[kf]:                             # MapPoint.cpp:216
                    continue
                if kf in local or kf in refs:                       # :322
                    continue
                refs.add(kf)                                        # :324
        n_obs = sum(1 for p in mps for kf in self.mp_obs[p] if not self.frame_null[kf] and (kf in local or kf in refs))
        self._memo[(cur, search_level)] = (local, refs, mps, n_obs)
        return local, refs, mps, n_obs

    def window(self, job_kf, search_level=3, kf_order=None, mp_order=None, kf_list_cap=None, mp_list_cap=None):
        """what se2gpu_local_window_batch_device leaves in its sentinel-filled outputs"""
        n, WF, W = len(job_kf), (self.nframes + 63) // 64, (self.m + 63) // 64
        win_kf, win_mp = np.full((n, 2, WF), WSENT, np.uint64), np.full((n, W), WSENT, np.uint64)
        out = np.full((n, 4), ISENT, np.int32)
        mk = lambda cap: None if cap is None else np.full((n, cap), ISENT, np.int32)  # noqa: E731
        local_list, ref_list, mp_list = mk(kf_list_cap), mk(kf_list_cap), mk(mp_list_cap)
        ko = range(self.nframes) if kf_order is None else [int(x) for x in kf_order]
        mo = range(self.m) if mp_order is None else [int(x) for x in mp_order]
        for j, cur in enumerate(job_kf):
            if not 0 <= cur < self.nframes:
                out[j] = (-1, 0, 0, 0)
                continue
            local, refs, mps, n_obs = self.update_local_graph(int(cur), search_level)
            win_kf[j] = pack([local, refs], self.nframes)
            win_mp[j] = pack([mps], self.m)[0]
            out[j] = (len(local), len(refs), len(mps), n_obs)
            for arr, members, order, cap in ((local_list, local, ko, kf_list_cap), (ref_list, refs, ko, kf_list_cap),
                                             (mp_list, mps, mo, mp_list_cap)):
                if arr is not None:
                    lst = [s for s in order if s in members][:cap]
                    arr[j, :len(lst)] = lst
        return dict(win_kf=win_kf, win_mp=win_mp, out=out, local_list=local_list, ref_list=ref_list, mp_list=mp_list)


def same_window(got, want):
    """every word, count and list, the sentinels of what a call leaves alone included; returns the first difference or None"""
    for k in ("win_kf", "win_mp", "out", "local_list", "ref_list", "mp_list"):
        if (got[k] is None) != (want[k] is None) or (want[k] is not None and not np.array_equal(got[k], want[k])):
            return k
    return None
