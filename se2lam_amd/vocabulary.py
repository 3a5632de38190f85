"""Python view of the device DBoW2 vocabulary over the C ABI (harness; C++ twin: include/se2lam_amd/ORBVocabularyDevice.h).

Reference interface: se2lam::ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>
    loadFromBinaryFile(path)                            OdoSLAM.cpp:45
    transform(features, BowVector, FeatureVector, 4)    KeyFrame.cpp:251, Localizer.cpp:195-205
    score(v1, v2) over every key frame                  GlobalMapper.cpp:201-254, Localizer.cpp:337-391
Three handles: Vocabulary (the tree on the device, immutable, shareable), BowContext (a thread's stream and scratch:
transform), BowDatabase (the key frames' BowVectors on the device: query).  Vocabulary.train makes a vocabulary from
descriptors (create).  All compute happens in libse2gpu.so (HIP).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
TF_IDF, TF, IDF, BINARY = range(4)


class Vocabulary:
    def __init__(self, k=None, L=None, scoring=None, weighting=None, parent=None, desc=None, weight=None, leaf=None, path=None):
        """either `path` (the file saveToBinaryFile writes) or the records: parent / desc (n x 32) / weight / leaf incl. the root"""
        self._h = C.c_void_p()
        if path is not None:
            capi.check(capi.lib().se2gpu_voc_load(str(path).encode(), C.byref(self._h)))
        else:
            parent = np.ascontiguousarray(parent, np.int32)
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1)
            weight = np.ascontiguousarray(weight, np.float64)
            leaf = np.ascontiguousarray(leaf, np.uint8)
            n = len(parent)
            assert len(desc) == 32 * n and len(weight) == n and len(leaf) == n
            capi.check(capi.lib().se2gpu_voc_create(int(k), int(L), int(scoring), int(weighting), n, parent.ctypes.data,
                                                    desc.ctypes.data, weight.ctypes.data, leaf.ctypes.data, C.byref(self._h)))
        self._read_header()

    def _read_header(self):
        l = capi.lib()
        self.k, self.L = l.se2gpu_voc_k(self._h), l.se2gpu_voc_L(self._h)
        self.scoring, self.weighting = l.se2gpu_voc_scoring(self._h), l.se2gpu_voc_weighting(self._h)
        self.words, self.nodes = l.se2gpu_voc_words(self._h), l.se2gpu_voc_nodes(self._h)

    @classmethod
    def load(cls, path):
        return cls(path=path)

    @classmethod
    def train(cls, desc, counts, k, L, weighting=TF_IDF, scoring=L1_NORM, seed=0, max_iters=0, cap=None, nframes=None):
        """TemplatedVocabulary::create on the device (se2gpu_voc_train; the algorithm: include/se2lam_amd/VocabularyTrain.h).
        desc (nframes, cap, 32) uint8 and counts (nframes,) as numpy arrays, or device pointers (capi.DeviceArray.ptr) with
        cap and nframes given.  The statistics of the run are left in `.train_stats` (a dict)."""
        on_device = cap is not None
        if not on_device:
            desc = np.ascontiguousarray(desc, np.uint8)
            assert desc.ndim == 3 and desc.shape[2] == 32
            nframes, cap = desc.shape[:2]
            counts = np.ascontiguousarray(counts, np.int32)
            assert len(counts) == nframes
            pd, pc = desc.ctypes.data, counts.ctypes.data
        else:
            pd, pc = desc, counts
        par = capi.VocTrainParams(int(k), int(L), int(scoring), int(weighting), int(max_iters), int(seed) & ((1 << 64) - 1))
        st = capi.VocTrainStats()
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        capi.check(capi.lib().se2gpu_voc_train(C.addressof(par), pd, pc, int(cap), int(nframes), int(on_device), C.byref(self._h), C.addressof(st)))
        self._read_header()
        self.train_stats = {n: int(getattr(st, n)) for n, _ in capi.VocTrainStats._fields_}
        return self

    def export(self):
        """-> parent (n,) int32, desc (n, 32) uint8, weight (n,) float64 (the file's floats widened), leaf (n,) bool; root at 0"""
        n = self.nodes
        parent, desc = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8)
        weight, leaf = np.zeros(n, np.float64), np.zeros(n, np.uint8)
        capi.check(capi.lib().se2gpu_voc_export(self._h, n, parent.ctypes.data, desc.ctypes.data, weight.ctypes.data, leaf.ctypes.data))
        return parent, desc, weight, leaf.astype(bool)

    def save(self, path):
        """the file saveToBinaryFile writes"""
        capi.check(capi.lib().se2gpu_voc_save(self._h, str(path).encode()))

    def __del__(self):
        try:
            if self._h:
                capi.lib().se2gpu_voc_destroy(self._h)
                self._h = None
        except Exception:
            pass


class BowContext:
    def __init__(self, voc: Vocabulary, max_features=4096, max_batch=1):
        self.voc = voc                      # keeps the tree alive
        self._h = C.c_void_p()
        capi.check(capi.lib().se2gpu_bow_create(voc._h, max_features, max_batch, C.byref(self._h)))

    def transform(self, desc, levelsup):
        """one frame, host buffers -> (words u32, values f64, (fv_nodes, fv_ptr, fv_idx) int32 CSR)"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        m = max(n, 1)
        word = np.zeros(m, np.uint32); val = np.zeros(m, np.float64)
        nodes = np.zeros(m, np.int32); ptr = np.zeros(m + 1, np.int32); idx = np.zeros(m, np.int32)
        nb, nn = C.c_int(0), C.c_int(0)
        capi.check(capi.lib().se2gpu_bow_transform(self._h, d.ctypes.data, n, int(levelsup), word.ctypes.data, val.ctypes.data,
                                                   C.byref(nb), nodes.ctypes.data, ptr.ctypes.data, idx.ctypes.data, C.byref(nn)))
        b, k = nb.value, nn.value
        return word[:b].copy(), val[:b].copy(), (nodes[:k].copy(), ptr[:k + 1].copy(), idx[:ptr[k]].copy())

    def transform_batch_device(self, d_desc, d_counts, cap, nframes, levelsup, d_bow_word, d_bow_value, d_bow_n, d_fv_nodes,
                               d_fv_ptr, d_fv_idx, d_fv_nn):
        """device pointers (capi.DeviceArray.ptr) in the layout of se2gpu.h; asynchronous on the context's stream"""
        capi.check(capi.lib().se2gpu_bow_transform_batch_device(self._h, d_desc, d_counts, cap, nframes, int(levelsup), d_bow_word,
                                                                d_bow_value, d_bow_n, d_fv_nodes, d_fv_ptr, d_fv_idx, d_fv_nn))

    def transform_batch(self, desc, counts, levelsup):
        """harness convenience: desc (nframes, cap, 32) and counts from host memory through the device-resident call ->
        per frame (words, values, (fv_nodes, fv_ptr, fv_idx))"""
        desc = np.ascontiguousarray(desc, np.uint8)
        nframes, cap = desc.shape[:2]
        counts = np.ascontiguousarray(counts, np.int32)
        D = capi.DeviceArray
        d_desc, d_cnt = D.from_numpy(desc), D.from_numpy(counts)
        bw, bv, bn = D(4 * nframes * cap), D(8 * nframes * cap), D(4 * nframes)
        fn, fp, fi, nn = D(4 * nframes * cap), D(4 * nframes * (cap + 1)), D(4 * nframes * cap), D(4 * nframes)
        self.transform_batch_device(d_desc.ptr, d_cnt.ptr, cap, nframes, levelsup, bw.ptr, bv.ptr, bn.ptr, fn.ptr, fp.ptr, fi.ptr, nn.ptr)
        self.sync()
        h_bw, h_bv, h_bn = bw.to_numpy(np.uint32, (nframes, cap)), bv.to_numpy(np.float64, (nframes, cap)), bn.to_numpy(np.int32, nframes)
        h_fn, h_fp = fn.to_numpy(np.int32, (nframes, cap)), fp.to_numpy(np.int32, (nframes, cap + 1))
        h_fi, h_nn = fi.to_numpy(np.int32, (nframes, cap)), nn.to_numpy(np.int32, nframes)
        out = []
        for f in range(nframes):
            b, k = int(h_bn[f]), int(h_nn[f])
            out.append((h_bw[f, :b].copy(), h_bv[f, :b].copy(), (h_fn[f, :k].copy(), h_fp[f, :k + 1].copy(), h_fi[f, :h_fp[f, k]].copy())))
        return out

    def sync(self):
        capi.check(capi.lib().se2gpu_bow_sync(self._h))

    def stream(self):
        return capi.lib().se2gpu_bow_stream(self._h)

    def set_stream(self, stream):
        capi.check(capi.lib().se2gpu_bow_set_stream(self._h, stream))

    def __del__(self):
        try:
            if self._h:
                capi.lib().se2gpu_bow_destroy(self._h)
                self._h = None
        except Exception:
            pass


class BowDatabase:
    def __init__(self, voc: Vocabulary):
        self.voc = voc
        self._h = C.c_void_p()
        capi.check(capi.lib().se2gpu_bowdb_create(voc._h, C.byref(self._h)))

    def __len__(self):
        return int(capi.lib().se2gpu_bowdb_size(self._h))

    def add(self, kf_id, word, value):
        word = np.ascontiguousarray(word, np.uint32); value = np.ascontiguousarray(value, np.float64)
        assert len(word) == len(value)
        capi.check(capi.lib().se2gpu_bowdb_add(self._h, int(kf_id), word.ctypes.data, value.ctypes.data, len(word)))

    def add_device(self, ctx: BowContext, kf_id, d_word, d_value, d_n, cap):
        capi.check(capi.lib().se2gpu_bowdb_add_device(self._h, ctx._h, int(kf_id), d_word, d_value, d_n, int(cap)))

    def remove(self, kf_id):
        capi.check(capi.lib().se2gpu_bowdb_remove(self._h, int(kf_id)))

    def query(self, ctx: BowContext, word, value, cur_kf_id=0, min_kfid_offset=0, n=None, want_scores=True):
        """-> (scores (size,) or None, best_entry, best_kf_id, best_score).  word / value: numpy arrays (host query), or device
        pointers with n given (device query)"""
        on_device = n is not None
        if not on_device:
            word = np.ascontiguousarray(word, np.uint32); value = np.ascontiguousarray(value, np.float64)
            n = len(word)
            pw, pv = word.ctypes.data, value.ctypes.data
        else:
            pw, pv = word, value
        scores = np.zeros(max(len(self), 1), np.float64) if want_scores else None
        be, bk, bs = C.c_int(-1), C.c_int(-1), C.c_double(0.0)
        capi.check(capi.lib().se2gpu_bowdb_query(self._h, ctx._h, pw, pv, int(n), int(on_device), int(cur_kf_id), int(min_kfid_offset),
                                                 None if scores is None else scores.ctypes.data, C.byref(be), C.byref(bk), C.byref(bs)))
        return (None if scores is None else scores[:len(self)]), be.value, bk.value, bs.value

    def __del__(self):
        try:
            if self._h:
                capi.lib().se2gpu_bowdb_destroy(self._h)
                self._h = None
        except Exception:
            pass


# ---- synthetic vocabularies (tests, tools/bow_bench.py): the reference ships no vocabulary file ----------------------------
def synthetic_vocabulary(seed, k, L, weighting=TF_IDF, full=True, early_leaf=0.0, stop_frac=0.05, tie_frac=0.0):
    """A random k-ary tree of depth L, generated level by level (vectorised; a full k = 10, L = 6 tree - the shape of ORBvoc,
    1.1 M nodes - takes seconds).  Nodes are numbered breadth first, so a parent precedes its children and siblings are
    consecutive.  full: every inner node has k children, otherwise 2 .. k.  early_leaf: share of the nodes above depth L that
    stay childless (leaves above depth L).  tie_frac: share of the inner nodes whose second child repeats the descriptor of
    the first (a tie at every distance).  stop_frac: share of the words with weight 0.
    -> parent (n,) int32, desc (n, 32) uint8, weight (n,) float32, leaf (n,) bool, all including the root at index 0."""
    rng = np.random.default_rng(seed)
    parent = [np.zeros(1, np.int32)]
    desc = [rng.integers(0, 256, (1, 32)).astype(np.uint8)]
    depth = [np.zeros(1, np.int32)]
    frontier = np.zeros(1, np.int64)
    frontier_desc = desc[0]
    nxt = 1
    for d in range(1, L + 1):
        if early_leaf > 0 and d > 1 and len(frontier) > 1:
            keep = rng.random(len(frontier)) >= early_leaf
            keep[0] = True
            if keep.all():                                                # a small level gets its early leaf too
                keep[-1] = False
            frontier, frontier_desc = frontier[keep], frontier_desc[keep]
        nch = np.full(len(frontier), k) if full else rng.integers(2, k + 1, len(frontier))
        par = np.repeat(frontier, nch)
        first = np.cumsum(nch) - nch                                      # position of every parent's first child
        flips = rng.random((len(par), 256)) < min(0.08 * (1 + d), 0.3)    # children resemble their parent, as cluster centres do
        dsc = np.repeat(frontier_desc, nch, axis=0) ^ np.packbits(flips, axis=1)
        if tie_frac > 0:
            t = first[(rng.random(len(frontier)) < tie_frac) & (nch >= 2)]
            dsc[t + 1] = dsc[t]
        parent.append(par.astype(np.int32)); desc.append(dsc); depth.append(np.full(len(par), d, np.int32))
        frontier = np.arange(nxt, nxt + len(par), dtype=np.int64)
        frontier_desc = dsc
        nxt += len(par)
    parent, desc, depth = np.concatenate(parent), np.concatenate(desc), np.concatenate(depth)
    n = len(parent)
    leaf = np.ones(n, bool)
    leaf[parent[1:]] = False
    leaf[0] = False
    weight = np.where(leaf, rng.uniform(0.1, 9.0, n), 0.0).astype(np.float32)
    weight[leaf & (rng.random(n) < stop_frac)] = 0.0
    if stop_frac > 0 and (weight[leaf] > 0).all():                        # a small tree gets its stopped word too
        weight[rng.choice(np.nonzero(leaf)[0])] = 0.0
    if weighting in (TF, BINARY):                                         # such vocabularies store 1
        weight[leaf & (weight > 0)] = 1.0
    return parent, desc, weight, leaf


def write_vocabulary_file(path, k, L, scoring, weighting, parent, desc, weight, leaf):
    """the layout of TemplatedVocabulary::saveToBinaryFile: 24-byte header, then 41 bytes per node 1 .. n-1"""
    n = len(parent)
    rec = np.zeros(n - 1, np.dtype([("parent", "<i4"), ("desc", "u1", 32), ("weight", "<f4"), ("leaf", "u1")]))
    assert rec.dtype.itemsize == 41
    rec["parent"], rec["desc"], rec["weight"], rec["leaf"] = parent[1:], desc[1:], weight[1:], leaf[1:]
    with open(path, "wb") as f:
        f.write(np.array([n, 41], "<u4").tobytes() + np.array([k, L, scoring, weighting], "<i4").tobytes())
        f.write(rec.tobytes())
