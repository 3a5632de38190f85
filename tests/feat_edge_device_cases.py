"""Inputs of se2gpu_feat_edge_batch_device for the tests and tools/feat_edge_device_bench.py: worlds of
feat_edge_cases.make_pair laid out as the device tables of both routes (float, as the map keeps them), with the places where
invalid entries are planted.  World w owns the frame slots 2w (key frame 0) and 2w + 1, a run of the point table and, per
point, the two observation entries 2g and 2g + 1 (covisibility route) or one feature in each frame (match route)."""
import numpy as np

import feat_edge_cases as fc

ISENT = -9            # capi.ISENT: what se2gpu_covis_pairs_device leaves behind the list
CAP = 136             # features per frame in the match tables


class Tables:
    def __init__(self, shapes, outliers=None, spare_points=3, Tbc=None):
        """shapes: (N, seed) per world; outliers: {world: planted count}; Tbc (4x4): the worlds as a camera mounted there sees
        them (feat_edge_cases.with_camera) instead of synth.RBC / TBC"""
        outliers = outliers or {}
        self.cases = [fc.make_pair(N, seed, n_outliers=outliers.get(w, 0)) if N else fc.empty_pair(seed)
                      for w, (N, seed) in enumerate(shapes)]
        if Tbc is not None:
            self.cases = [fc.with_camera(c, Tbc) for c in self.cases]
        self.N = np.array([len(c["mp"]) for c in self.cases])
        self.off = np.concatenate([[0], np.cumsum(self.N)]).astype(int)
        W = len(shapes)
        self.nframes, self.m = 2 * W + 1, int(self.off[-1]) + spare_points     # a spare frame and spare points nobody names
        self.nobs = 2 * self.m
        self.Twc = np.zeros((self.nframes, 12), np.float32)
        self.Twc[:, [0, 5, 10]] = 1
        self.pos = np.zeros((self.m, 3), np.float32)
        self.obs_view, self.obs_info = np.zeros((self.nobs, 3), np.float32), np.zeros((self.nobs, 9), np.float32)
        self.counts = np.full(self.nframes, CAP, np.int32)
        self.ftr_mp = np.full((self.nframes, CAP), -1, np.int32)
        self.view_pos, self.view_info = np.zeros((self.nframes, CAP, 3), np.float32), np.zeros((self.nframes, CAP, 9), np.float32)
        self.view_info[...] = np.eye(3, dtype=np.float32).ravel()
        for w, c in enumerate(self.cases):
            n, o = self.N[w], self.off[w]
            for k in range(2):
                self.Twc[2 * w + k] = c["kf"][k][:3, :4].ravel()
            self.pos[o:o + n] = c["mp"]
            g = o + np.arange(n)
            for k in range(2):
                self.obs_view[2 * g + k] = c["z"][:, k]
                self.obs_info[2 * g + k] = c["info"][:, k].reshape(n, 9)
                ftr = self.ftr_of(w, k)
                self.ftr_mp[2 * w + k, ftr] = g
                self.view_pos[2 * w + k, ftr] = c["z"][:, k]
                self.view_info[2 * w + k, ftr] = c["info"][:, k].reshape(n, 9)

    def ftr_of(self, w, k):
        """the feature of key frame k that observes point j of world w: ascending in key frame 0 (the order the matches are
        walked in), descending in key frame 1"""
        j = np.arange(self.N[w])
        return j + 3 if k == 0 else (self.N[w] - 1 - j) + 2

    def case(self, w, keep=None):
        """world w as the device sees it - the float tables in double - restricted to the points `keep` (index array)"""
        n, o = self.N[w], self.off[w]
        keep = np.arange(n) if keep is None else np.asarray(keep, int)
        g = o + keep
        kf = np.zeros((2, 4, 4))
        kf[:, 3, 3] = 1
        kf[:, :3, :4] = self.Twc[2 * w:2 * w + 2].astype(np.float64).reshape(2, 3, 4)
        z = np.stack([self.obs_view[2 * g], self.obs_view[2 * g + 1]], 1).astype(np.float64)
        info = np.stack([self.obs_info[2 * g], self.obs_info[2 * g + 1]], 1).astype(np.float64).reshape(len(g), 2, 3, 3)
        return dict(kf=kf, mp=self.pos[g].astype(np.float64), z=z, info=info, planted=self.cases[w]["planted"][keep])

    def covis_inputs(self, worlds, list_cap, plant=()):
        """pair_a, pair_b, pair_out (n, 4), common (n, list_cap, 3) as se2gpu_covis_pairs_device leaves them for these worlds.
        plant: (pair, entry, column, value) replacements inside the lists"""
        n = len(worlds)
        pair_a, pair_b = np.array([2 * w for w in worlds], np.int32), np.array([2 * w + 1 for w in worlds], np.int32)
        pair_out = np.zeros((n, 4), np.int32)
        common = np.full((n, list_cap, 3), ISENT, np.int32)
        for p, w in enumerate(worlds):
            N = int(self.N[w])
            pair_out[p] = (N, N, N, 3)
            k = min(N, list_cap)
            g = self.off[w] + np.arange(k)
            common[p, :k] = np.stack([g, 2 * g, 2 * g + 1], 1)
        for p, i, col, v in plant:
            common[p, i, col] = v
        return pair_a, pair_b, pair_out, common

    def match_inputs(self, worlds, plant=()):
        """pair_a, pair_b, matches (n, CAP) in the layout of the verify call's d_matches_mp.  plant: (pair, feature, value)"""
        n = len(worlds)
        pair_a, pair_b = np.array([2 * w for w in worlds], np.int32), np.array([2 * w + 1 for w in worlds], np.int32)
        matches = np.full((n, CAP), -1, np.int32)
        for p, w in enumerate(worlds):
            matches[p, self.ftr_of(w, 0)] = self.ftr_of(w, 1)
        for p, i, v in plant:
            matches[p, i] = v
        return pair_a, pair_b, matches
