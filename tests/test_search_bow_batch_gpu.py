"""se2gpu_search_by_bow_batch_device (SearchByBoW over a batch of key-frame pairs that lie in HBM) against the CPU oracle:
match rows and counts are compared EXACTLY, the tail of every row is -1.

Frames: the oracle's extraction of synth.frame(0..5), 1,000 features each, packed with cap = 1024.  FeatureVectors: the
stand-in of tests/test_match_gpu.py (node = the first `nbits` descriptor bits).  What the sweep's shapes cover:
  nbits  0: 1 node of 1,000 features (16 chunks of 64)      nbits 3: 8 nodes of ~240 (four chunks)
  nbits  5: 32 nodes of 70-90 (two chunks, the second nearly empty)      nbits 7: ~126 nodes of ~30 (the reference's regime)
  nbits 10: ~500 nodes of 11-18; the node sets differ between frames and there are more node pairs than waves per pair"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 1024
PAIRS = [(0, 1), (1, 0), (0, 2), (2, 5), (3, 3), (0, 5), (4, 1)]


def _feature_vector(desc, nbits):
    """Stand-in for DBoW2::FeatureVector: node = the first `nbits` descriptor bits; CSR with ascending node ids."""
    node = (desc[:, 0].astype(np.int32) | (desc[:, 1].astype(np.int32) << 8)) & ((1 << nbits) - 1)
    order = np.argsort(node, kind="stable")
    nodes, counts = np.unique(node[order], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return nodes.astype(np.int32), ptr, order.astype(np.int32)


class FrameSet:
    """key frames (kps, desc) with their feature vectors and map-point flags, packed into the strided device layouts"""

    def __init__(self, frames, fvs, cap, has=None, counts=None, nn=None):
        from se2lam_amd import capi
        D = capi.DeviceArray
        B = len(frames)
        self.frames, self.fvs, self.cap, self.B = frames, fvs, cap, B
        self.has = has if has is not None else [np.ones(len(k), np.uint8) for k, _ in frames]
        kps, desc = np.zeros((B, cap), capi.KP_DTYPE), np.zeros((B, cap, 32), np.uint8)
        cnt = np.zeros(B, np.int32)
        nodes, ptr, idx = np.zeros((B, cap), np.int32), np.zeros((B, cap + 1), np.int32), np.zeros((B, cap), np.int32)
        nnodes, flags = np.zeros(B, np.int32), np.zeros((B, cap), np.uint8)
        for f, ((k, d), (fn, fp, fi)) in enumerate(zip(frames, fvs)):
            n = len(k)
            kps[f, :n], desc[f, :n], cnt[f] = k, d, n
            nodes[f, :len(fn)], ptr[f, :len(fp)], idx[f, :len(fi)], nnodes[f] = fn, fp, fi, len(fn)
            flags[f, :n] = self.has[f]
        if counts is not None:
            cnt[:] = counts
        if nn is not None:
            nnodes[:] = nn
        self.counts = cnt
        self.d = [D.from_numpy(a) for a in (kps, desc, cnt, nodes, ptr, idx, nnodes, flags)]

    def search(self, matcher, pairs, mp_only, check_ori, has_flags=True):
        """one batch call -> (matches12 (npairs, cap), nmatches (npairs,))"""
        from se2lam_amd import capi
        D = capi.DeviceArray
        kps, desc, cnt, nodes, ptr, idx, nnodes, flags = self.d
        pa, pb = D.from_numpy(np.array([p[0] for p in pairs], np.int32)), D.from_numpy(np.array([p[1] for p in pairs], np.int32))
        P = len(pairs)
        d_m, d_nm = D.from_numpy(np.full((P, self.cap), 7, np.int32)), D.from_numpy(np.full(P, 7, np.int32))
        matcher.search_by_bow_batch_device(kps.ptr, desc.ptr, cnt.ptr, self.cap, self.B, nodes.ptr, ptr.ptr, idx.ptr, nnodes.ptr,
                                           flags.ptr if has_flags else None, pa.ptr, pb.ptr, P, d_m.ptr, d_nm.ptr,
                                           bIfMPOnly=mp_only, checkOri=check_ori)
        matcher.sync()
        return d_m.to_numpy(np.int32, (P, self.cap)), d_nm.to_numpy(np.int32, (P,))


@pytest.fixture(scope="module")
def feats(oracle, synth):
    return [oracle.orb_extract(synth.frame(t)) for t in range(6)]


@pytest.fixture(scope="module")
def sets(feats):
    """the six frames on the device, once per nbits (and once with the map-point flags of the mp_only test)"""
    cache = {}

    def get(nbits, has=None):
        key = (nbits, has is not None)
        if key not in cache:
            cache[key] = FrameSet(feats, [_feature_vector(d, nbits) for _, d in feats], CAP, has)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def reference(oracle):
    """oracle.search_by_bow of one pair of a frame set, computed once and shared"""
    cache = {}

    def get(fs, tag, a, b, mp_only, ratio, check_ori):
        key = (tag, a, b, mp_only, ratio, check_ori)
        if key not in cache:
            (k1, d1), (k2, d2) = fs.frames[a], fs.frames[b]
            cache[key] = oracle.search_by_bow(k1, d1, fs.fvs[a], fs.has[a], k2, d2, fs.fvs[b], fs.has[b], mp_only, ratio, check_ori)
        return cache[key]
    return get


def _matcher(ratio, cap=CAP):
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher(ratio, max_features=min(cap, 8192), max_batch=8)


def _check_row(m12_row, nm, m_ref, nm_ref, n1):
    assert nm == nm_ref
    assert np.array_equal(m12_row[:n1], m_ref)
    assert (m12_row[n1:] == -1).all()


@pytest.mark.parametrize("ratio", [0.6, 0.9])
@pytest.mark.parametrize("nbits", [0, 3, 5, 7, 10])
def test_parity_sweep(sets, reference, nbits, ratio):
    fs = sets(nbits)
    mt = _matcher(ratio)
    counts = {}
    for check_ori in (True, False):
        m12, nm = fs.search(mt, PAIRS, False, check_ori, has_flags=False)
        for p, (a, b) in enumerate(PAIRS):
            m_ref, nm_ref = reference(fs, nbits, a, b, False, ratio, check_ori)
            print("nbits %d ratio %.1f ori %d pair %s: device %d oracle %d" % (nbits, ratio, check_ori, (a, b), nm[p], nm_ref))
            assert nm_ref >= 400
            counts[(p, check_ori)] = nm_ref
            _check_row(m12[p], nm[p], m_ref, nm_ref, len(fs.frames[a][0]))
    for p, (a, b) in enumerate(PAIRS):   # the orientation check removes matches, so the per-pair histogram is exercised
        if (a, b) != (3, 3):
            assert counts[(p, True)] < counts[(p, False)]


def test_mp_only(sets, feats, reference):
    from se2lam_amd import capi
    rng = np.random.default_rng(1)
    has = [(rng.random(len(k)) < 0.7).astype(np.uint8) for k, _ in feats]
    fs = sets(5, has)
    mt = _matcher(0.6)
    m12, nm = fs.search(mt, PAIRS, True, True)
    for p, (a, b) in enumerate(PAIRS):
        m_ref, nm_ref = reference(fs, "mp5", a, b, True, 0.6, True)
        print("mp_only pair %s: device %d oracle %d" % ((a, b), nm[p], nm_ref))
        assert nm_ref >= 200
        _check_row(m12[p], nm[p], m_ref, nm_ref, len(feats[a][0]))
    with pytest.raises(capi.Se2GpuError) as e:
        fs.search(mt, PAIRS, True, True, has_flags=False)
    assert e.value.code == capi.ERR_INVALID


def test_pairs_are_independent_and_the_scratch_reinitialises(sets, feats, reference):
    base = sets(5)
    # frames 0..5, frame 6 = frame 0 with counts = 0 (its feature vector kept), frame 7 = frame 1 with nn = 0
    frames = list(feats) + [feats[0], feats[1]]
    fvs = list(base.fvs) + [base.fvs[0], base.fvs[1]]
    counts = [len(k) for k, _ in frames]; counts[6] = 0
    nn = [len(fv[0]) for fv in fvs]; nn[7] = 0
    fs = FrameSet(frames, fvs, CAP, counts=counts, nn=nn)
    pairs = [(0, 1), (6, 1), (1, 0), (0, 1), (1, 6), (7, 1), (0, 1), (1, 7)]
    mt = _matcher(0.6)

    def check(pairs, m12, nm):
        for p, (a, b) in enumerate(pairs):
            if a >= 6 or b >= 6:
                assert nm[p] == 0 and (m12[p] == -1).all()
            else:
                m_ref, nm_ref = reference(base, 5, a, b, False, 0.6, True)
                assert nm_ref >= 400
                _check_row(m12[p], nm[p], m_ref, nm_ref, len(feats[a][0]))

    m12, nm = fs.search(mt, pairs, False, True)
    check(pairs, m12, nm)
    assert np.array_equal(m12[0], m12[3]) and np.array_equal(m12[0], m12[6]) and nm[0] == nm[3] == nm[6]
    m12_again, nm_again = fs.search(mt, pairs, False, True)          # the same handle: its scratch starts clean again
    assert np.array_equal(m12_again, m12) and np.array_equal(nm_again, nm)
    fewer = [(1, 0), (7, 1), (0, 1)]
    m12_f, nm_f = fs.search(mt, fewer, False, True)
    check(fewer, m12_f, nm_f)


def test_a_node_of_thousands(oracle, feats):
    """frames 0-2 against 3-5 as one key frame each: 3,000 features in one node, a random permutation as its index list"""
    rng = np.random.default_rng(11)
    frames = [(np.concatenate([feats[t][0] for t in ts]), np.concatenate([feats[t][1] for t in ts])) for ts in ((0, 1, 2), (3, 4, 5))]
    assert all(len(k) == 3000 for k, _ in frames)
    fvs = [(np.zeros(1, np.int32), np.array([0, len(k)], np.int32), rng.permutation(len(k)).astype(np.int32)) for k, _ in frames]
    fs = FrameSet(frames, fvs, 3072)
    m12, nm = fs.search(_matcher(0.9, 3072), [(0, 1)], False, True, has_flags=False)
    m_ref, nm_ref = oracle.search_by_bow(frames[0][0], frames[0][1], fvs[0], fs.has[0], frames[1][0], frames[1][1], fvs[1], fs.has[1],
                                         False, 0.9, True)
    print("node of thousands: device %d oracle %d" % (nm[0], nm_ref))
    assert nm_ref > 100
    _check_row(m12[0], nm[0], m_ref, nm_ref, 3000)


@pytest.mark.parametrize("ratio", [0.6, 0.9])
def test_equals_the_host_buffer_path(sets, ratio):
    fs = sets(7)
    mt = _matcher(ratio)
    m12, nm = fs.search(mt, PAIRS, False, True, has_flags=False)
    for p, (a, b) in enumerate(PAIRS):
        (k1, d1), (k2, d2) = fs.frames[a], fs.frames[b]
        nm_h, m12_h = mt.SearchByBoW(k1, d1, fs.fvs[a], fs.has[a], k2, d2, fs.fvs[b], fs.has[b], bIfMPOnly=False)
        assert nm[p] == nm_h and np.array_equal(m12[p, :len(k1)], m12_h) and (m12[p, len(k1):] == -1).all()


def _scene_tree(rng, k, L, d1):
    """a small vocabulary "trained" on the scene, as tests/test_bow_gpu.py builds it"""
    parent, depth, frontier = [0], [0], [0]
    for lv in range(1, L + 1):
        nxt = []
        for p in frontier:
            for _ in range(k):
                parent.append(p); depth.append(lv); nxt.append(len(parent) - 1)
        frontier = nxt
    n = len(parent)
    parent = np.array(parent, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    for i in range(1, n):
        if parent[i] == 0:
            desc[i] = d1[rng.integers(0, len(d1))]
        else:
            desc[i] = desc[parent[i]] ^ np.packbits(rng.random((32, 8)) < 0.05 * depth[i], axis=1).reshape(32)
    leaf = np.array(depth) == L
    return parent, desc, leaf, np.where(leaf, 1.0, 0.0).astype(np.float32)


def test_extract_transform_search_with_nothing_downloaded_in_between(oracle, synth, tmp_path):
    """se2gpu_orb_extract_batch_device -> se2gpu_bow_transform_batch_device -> se2gpu_search_by_bow_batch_device on the arrays
    where they lie, the matcher on the context's stream; downloads only after the last sync"""
    from se2lam_amd import capi, orb, vocabulary as V
    imgs = np.stack([synth.frame(0), synth.frame(1)])
    B, rows, cols = imgs.shape
    cap = 2000
    D = capi.DeviceArray
    ex = orb.ORBextractor(max_batch=2)
    d_img, d_kps, d_desc, d_cnt = D.from_numpy(imgs), D(B * cap * 28), D(B * cap * 32), D(B * 4)
    ex.extract_batch_device(d_img.ptr, B, rows, cols, d_kps.ptr, d_desc.ptr, d_cnt.ptr, cap)
    ex.sync()
    # the vocabulary is built from frame 0's descriptors: the one download, before the chain under test starts
    d0 = d_desc.to_numpy(np.uint8, (B, cap, 32))[0, :int(d_cnt.to_numpy(np.int32, (B,))[0])]
    k, L = 8, 3
    parent, desc_v, leaf, weight = _scene_tree(np.random.default_rng(4), k, L, d0)
    path = tmp_path / "scene_voc.bin"
    V.write_vocabulary_file(path, k, L, 0, 0, parent, desc_v, weight, leaf)
    ctx = V.BowContext(V.Vocabulary.load(path), cap, B)
    bw, bv, bn = D(4 * B * cap), D(8 * B * cap), D(4 * B)
    fn, fp, fi, nn = D(4 * B * cap), D(4 * B * (cap + 1)), D(4 * B * cap), D(4 * B)
    mt = _matcher(0.9, cap)
    mt.set_stream(ctx.stream())
    pairs = [(0, 1), (1, 0)]
    pa, pb = D.from_numpy(np.array([0, 1], np.int32)), D.from_numpy(np.array([1, 0], np.int32))
    d_m, d_nm = D(4 * len(pairs) * cap), D(4 * len(pairs))
    ctx.transform_batch_device(d_desc.ptr, d_cnt.ptr, cap, B, 2, bw.ptr, bv.ptr, bn.ptr, fn.ptr, fp.ptr, fi.ptr, nn.ptr)
    mt.search_by_bow_batch_device(d_kps.ptr, d_desc.ptr, d_cnt.ptr, cap, B, fn.ptr, fp.ptr, fi.ptr, nn.ptr, None, pa.ptr, pb.ptr,
                                  len(pairs), d_m.ptr, d_nm.ptr, bIfMPOnly=False)
    mt.sync()
    cnt = d_cnt.to_numpy(np.int32, (B,))
    kps, desc = d_kps.to_numpy(capi.KP_DTYPE, (B, cap)), d_desc.to_numpy(np.uint8, (B, cap, 32))
    h_nn = nn.to_numpy(np.int32, B)
    h_fn, h_fp, h_fi = fn.to_numpy(np.int32, (B, cap)), fp.to_numpy(np.int32, (B, cap + 1)), fi.to_numpy(np.int32, (B, cap))
    fvs = [(h_fn[f, :h_nn[f]], h_fp[f, :h_nn[f] + 1], h_fi[f, :h_fp[f, h_nn[f]]]) for f in range(B)]
    m12, nm = d_m.to_numpy(np.int32, (len(pairs), cap)), d_nm.to_numpy(np.int32, (len(pairs),))
    for p, (a, b) in enumerate(pairs):
        m_ref, nm_ref = oracle.search_by_bow(kps[a, :cnt[a]], desc[a, :cnt[a]], fvs[a], np.ones(cnt[a], np.uint8),
                                             kps[b, :cnt[b]], desc[b, :cnt[b]], fvs[b], np.ones(cnt[b], np.uint8), False, 0.9, True)
        _check_row(m12[p], nm[p], m_ref, nm_ref, cnt[a])
    assert nm[0] > 100
