"""An independent model of the covisibility calls (se2gpu_covis_*_device, include/se2gpu.h): Python sets per key frame built
from the observation CSR by the validity rule, and Map::compareViewMPs (src/Map.cpp:354-400 of the reference) restated on them.
No bit tricks: the bit matrix is only packed at the end, for the comparison with d_bits.  The threshold tests spell out every
conversion: np.float32 for Map.cpp:794, Python float (IEEE double) for Localizer.cpp:683 and Map.cpp:196, :398."""
import numpy as np

SENT, ISENT = -7.0, -9


class Model:
    """sets[f]: the points key frame slot f observes (KeyFrame::mObservations); first[(f, p)]: the CSR index of the first valid
    entry of frame f in point p's list; notnull / good: the points getAllObsMPs(false) / getAllObsMPs() keep"""

    def __init__(self, counts, cap, mp_ptr, obs_frame, obs_ftr, mp_null=None, good_prl=None):
        self.nframes, self.m, self.nobs = len(counts), len(mp_ptr) - 1, len(obs_frame)
        self.sets = [set() for _ in range(self.nframes)]
        self.first = {}
        for p in range(self.m):
            s, e = (min(max(int(mp_ptr[p + i]), 0), self.nobs) for i in (0, 1))
            for i in range(s, e):                               # a descending segment is an empty range
                f, k = int(obs_frame[i]), int(obs_ftr[i])
                if not 0 <= f < self.nframes or not 0 <= k < min(int(counts[f]), cap):
                    continue
                self.sets[f].add(p)
                self.first.setdefault((f, p), i)
        self.notnull = {p for p in range(self.m) if mp_null is None or not mp_null[p]}
        self.good = {p for p in self.notnull if good_prl is None or good_prl[p]}

    def size_obs(self):
        return np.array([len(s) for s in self.sets], np.int32)      # KeyFrame::getSizeObsMP: null points included

    def bits(self):
        W = (self.m + 63) // 64
        rows = np.zeros((self.nframes + 2, W * 64), np.uint8)
        for r, s in enumerate(self.sets + [self.notnull, self.good]):
            rows[r, sorted(s)] = 1
        return np.packbits(rows, axis=1, bitorder="little").view(np.uint64).reshape(self.nframes + 2, W)

    def common(self, a, b):
        """spMPs of compareViewMPs(pKF_a, pKF_b, spMPs), ascending"""
        return sorted(p for p in self.sets[a] if p in self.notnull and p in self.sets[b])

    def pairs(self, pair_a, pair_b, ratio_f=0.3, ratio_d=0.1, list_cap=None):
        n = len(pair_a)
        out, ratio = np.full((n, 4), ISENT, np.int32), np.full((n, 2), SENT, np.float32)
        common = None if list_cap is None else np.full((n, list_cap, 3), ISENT, np.int32)
        for i, (a, b) in enumerate(zip(pair_a, pair_b)):
            if not (0 <= a < self.nframes and 0 <= b < self.nframes):
                out[i] = (-1, 0, 0, 0)
                continue
            sp = self.common(a, b)
            n_same, size_a, size_b = len(sp), len(self.sets[a]), len(self.sets[b])
            flags = 0
            if np.float32(n_same) > np.float32(ratio_f) * np.float32(size_a):     # Map.cpp:794
                flags |= 1
            if float(n_same) > float(ratio_d) * float(size_a):                    # Localizer.cpp:683
                flags |= 2
            out[i] = (n_same, size_a, size_b, flags)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio[i] = (np.float32(n_same) / np.float32(size_a), np.float32(n_same) / np.float32(size_b))   # :367-368
            if common is not None:
                for j, p in enumerate(sp[:list_cap]):
                    common[i, j] = (p, self.first[(a, p)], self.first[(b, p)])
        return dict(out=out, ratio=ratio, common=common)

    def refset_points(self, kf, refs, k):
        """(spMPsRet, spMPsAll) of compareViewMPs(pKFNow, spKFsRef, spMPsRet, k): refs as listed, out-of-range ones skipped"""
        allp = sorted(p for p in self.sets[kf] if p in self.good)
        refs = [f for f in refs if 0 <= f < self.nframes]
        return [p for p in allp if sum(1 for f in refs if p in self.sets[f]) >= k], allp

    def refset(self, job_kf, ref_ptr, ref_idx, k=2, thresh=0.8):
        n, nref = len(job_kf), len(ref_idx)
        out, ratio = np.full((n, 3), ISENT, np.int32), np.full(n, SENT, np.float64)
        for j, kf in enumerate(job_kf):
            if not 0 <= kf < self.nframes:
                out[j] = (-1, 0, 0)
                continue
            s, e = (min(max(int(ref_ptr[j + i]), 0), nref) for i in (0, 1))
            ret, allp = self.refset_points(kf, [int(f) for f in ref_idx[s:e]] if e > s else [], k)
            r = -1.0 if not allp else float(len(ret)) * 1.0 / float(len(allp))    # :377-379, :398
            out[j] = (len(ret), len(allp), int(bool(allp) and r >= float(thresh)))   # :196
            ratio[j] = r
        return dict(out=out, ratio=ratio)


def same_floats(a, b):
    """equal to the bit, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
