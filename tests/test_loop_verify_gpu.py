"""se2gpu_track_loop_verify_batch_device (RemoveMatchOutlierRansac + RemoveKPMatch over a batch of key-frame pairs in HBM)
against tests/loop_verify_model.py: both output rows and all 8 info fields are compared EXACTLY.

Scene: 12 frames, cap = 512; frames 2k and 2k+1 hold the two views of synth.two_view_matches(seed k), each in a random feature
order of its own, the rest of the row up to cap filled with further points (counts decides what is a feature).  A match row
names a random subset of the correspondences, so it is a permutation with holes: the ascending feature order in which the
points have to be taken differs from the order of the correspondences and from the order of the matched indices."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_verify_model as lvm  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 512
NFRAMES = 12
N_POINTS = (400, 512, 333, 450, 512, 380)          # features of the two frames of view pair k
OUTLIERS = (0.0, 0.1, 0.3, 0.5, 0.2, 0.7)
SENTINEL = 7


class Scene:
    def __init__(self, synth, capi):
        rng = np.random.default_rng(2024)
        self.kps = np.zeros((NFRAMES, CAP), capi.KP_DTYPE)
        self.kps["x"] = rng.uniform(0, 640, (NFRAMES, CAP)).astype(np.float32)
        self.kps["y"] = rng.uniform(0, 480, (NFRAMES, CAP)).astype(np.float32)
        self.counts = np.zeros(NFRAMES, np.int32)
        self.where = []                              # where[k] = (position of correspondence j in frame 2k, in frame 2k+1)
        for k, (n, frac) in enumerate(zip(N_POINTS, OUTLIERS)):
            p1, p2, _ = synth.two_view_matches(100 + k, n, frac)
            wa, wb = rng.permutation(n), rng.permutation(n)
            for f, w, p in ((2 * k, wa, p1), (2 * k + 1, wb, p2)):
                self.kps["x"][f, w], self.kps["y"][f, w] = p[:, 0], p[:, 1]
                self.counts[f] = n
            self.where.append((wa, wb))
        self.has_mp = (rng.random((NFRAMES, CAP)) < 0.7).astype(np.uint8)
        self.num_mps = rng.integers(0, 400, NFRAMES).astype(np.int32)

    def row(self, k, n_raw):
        """a match row frame 2k -> frame 2k+1 with n_raw of the correspondences (the same ones for the same arguments)"""
        wa, wb = self.where[k]
        row = np.full(CAP, -1, np.int32)
        js = np.random.default_rng([k, n_raw]).choice(len(wa), n_raw, replace=False)
        row[wa[js]] = wb[js]
        return row


@pytest.fixture(scope="module")
def scene(synth):
    from se2lam_amd import capi
    return Scene(synth, capi)


def run_batch(track, kps, counts, pairs, rows, has_mp=None, num_mps=None, want_mp=True, sync=True):
    """one call -> (good (P, cap), mp (P, cap) or None, info (P, 8)); the outputs start as SENTINEL"""
    from se2lam_amd import capi
    D = capi.DeviceArray
    nframes, cap = kps.shape
    P = len(pairs)
    d_kps, d_cnt = D.from_numpy(kps), D.from_numpy(np.asarray(counts, np.int32))
    d_has = None if has_mp is None else D.from_numpy(has_mp)
    d_num = None if num_mps is None else D.from_numpy(num_mps)
    d_pa = D.from_numpy(np.array([p[0] for p in pairs], np.int32))
    d_pb = D.from_numpy(np.array([p[1] for p in pairs], np.int32))
    d_rows = D.from_numpy(np.stack(rows).astype(np.int32))
    d_good = D.from_numpy(np.full((P, cap), SENTINEL, np.int32))
    d_mp = D.from_numpy(np.full((P, cap), SENTINEL, np.int32)) if (want_mp and has_mp is not None) else None
    d_info = D.from_numpy(np.full((P, 8), SENTINEL, np.int32))
    track.loop_verify_batch_device(d_kps.ptr, d_cnt.ptr, cap, nframes, d_has and d_has.ptr, d_num and d_num.ptr, d_pa.ptr, d_pb.ptr,
                                   P, d_rows.ptr, d_good.ptr, d_mp and d_mp.ptr, d_info.ptr)
    track.sync()
    return (d_good.to_numpy(np.int32, (P, cap)), None if d_mp is None else d_mp.to_numpy(np.int32, (P, cap)),
            d_info.to_numpy(np.int32, (P, 8)))


def check_equal(got, want, pairs):
    (g_good, g_mp, g_info), (w_good, w_mp, w_info) = got, want
    for p, pair in enumerate(pairs):
        print("pair %d %s: device %s model %s" % (p, pair, g_info[p].tolist(), w_info[p].tolist()))
    for p, pair in enumerate(pairs):
        assert np.array_equal(g_info[p], w_info[p]), (p, pair)
        assert np.array_equal(g_good[p], w_good[p]), (p, pair)
        if w_mp is not None and g_mp is not None:
            assert np.array_equal(g_mp[p], w_mp[p]), (p, pair)


# ---- direct ---------------------------------------------------------------------------------------------------------------
RAW_COUNTS = (0, 9, 10, 14, 15, 16, 64, 65, 300)


@pytest.fixture(scope="module")
def direct(scene, oracle):
    """the batch of the direct test and its model (with has_mp and num_mps), shared with the single-pair test"""
    pairs, rows = [], []
    for p, n_raw in enumerate(RAW_COUNTS):
        k = p % 6
        pairs.append((2 * k, 2 * k + 1)); rows.append(scene.row(k, n_raw))
    pairs.append(pairs[8]); rows.append(rows[8])                 # a repeated pair (300 raw matches)
    pairs.append((2, 2)); rows.append(scene.row(1, 120))         # (f, f): frame 2 against itself, frame 3's indices fit its 512
    pairs.append((1, 0)); rows.append(scene.row(0, 200))   # the second view first; its row indexes frame 0 by chance only
    model = lvm.verify_batch(oracle, scene.kps, scene.counts, CAP, pairs, rows, scene.has_mp, scene.num_mps)
    return pairs, rows, model


def test_direct(scene, direct):
    from se2lam_amd.track import Track
    pairs, rows, model = direct
    w_good, w_mp, w_info = model
    assert w_info[:9, 0].tolist() == list(RAW_COUNTS)
    assert w_info[:9, 4].tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 2]
    assert (w_info[8, 1] > w_info[8, 2] > 0) and w_info[6, 1] >= 10 and w_info[7, 1] >= 10
    tr = Track()
    got = run_batch(tr, scene.kps, scene.counts, pairs, rows, scene.has_mp, scene.num_mps)
    check_equal(got, model, pairs)
    for p, (a, b) in enumerate(pairs):
        assert (got[0][p, scene.counts[a]:] == -1).all() and (got[1][p, scene.counts[a]:] == -1).all()
    assert np.array_equal(got[0][8], got[0][9]) and np.array_equal(got[2][8], got[2][9])
    # d_num_mps NULL: n_mps_a is the number of set flags among the features of frame a; everything else is unchanged
    got_n = run_batch(tr, scene.kps, scene.counts, pairs, rows, scene.has_mp, None)
    w_info_n = w_info.copy()
    w_info_n[:, 3] = [np.count_nonzero(scene.has_mp[a, :scene.counts[a]]) for a, _ in pairs]
    check_equal(got_n, (w_good, w_mp, w_info_n), pairs)
    # no flags at all: no map-point rows, n_good_mp = n_mps_a = 0
    got_0 = run_batch(tr, scene.kps, scene.counts, pairs, rows, None, None)
    w_info_0 = w_info.copy()
    w_info_0[:, 2] = 0; w_info_0[:, 3] = 0
    check_equal(got_0, (w_good, None, w_info_0), pairs)
    # flags without the map-point rows: the counts are still there
    got_c = run_batch(tr, scene.kps, scene.counts, pairs, rows, scene.has_mp, scene.num_mps, want_mp=False)
    check_equal(got_c, (w_good, None, w_info), pairs)


def test_equals_the_single_pair_path(scene, direct):
    """se2gpu_track_remove_outliers on the downloaded arrays keeps what the batch keeps (it clears everything below 10
    inliers, so the pairs are ones where the batch leaves at least 10)"""
    from se2lam_amd.track import Track
    pairs, rows, (w_good, _, w_info) = direct
    tr = Track()
    chosen = [6, 7, 8]
    got_good, _, got_info = run_batch(tr, scene.kps, scene.counts, [pairs[p] for p in chosen], [rows[p] for p in chosen])
    for q, p in enumerate(chosen):
        a, b = pairs[p]
        na, nb = scene.counts[a], scene.counts[b]
        assert w_info[p, 1] >= 10
        m = rows[p][:na].copy()
        ni = tr.removeOutliers(scene.kps[a, :na], scene.kps[b, :nb], m)
        print("pair %s: batch %d single %d survivors" % ((a, b), got_info[q, 1], ni))
        assert ni == got_info[q, 1] and np.array_equal(m, got_good[q, :na])
        last = tr.last_ransac()
        assert [last["sample"], last["model"], last["iterations"]] == got_info[q, 5:8].tolist()


# ---- hostile inputs --------------------------------------------------------------------------------------------------------
def test_hostile_inputs(scene, oracle):
    from se2lam_amd.track import Track
    kps, counts = scene.kps.copy(), scene.counts.copy()
    counts[2], counts[3], counts[6] = CAP + 1000, 2**31 - 1, -5
    kps["x"][10:12], kps["y"][10:12] = 0.0, 0.0                 # a degenerate pair, every point the same: no model exists
    kps["x"][8:10], kps["y"][8:10] = 100.0, 50.0                # the same away from the origin: a model, every point fits it
    counts[8:12] = 40
    normal = scene.row(0, 100)
    spiked = scene.row(2, 150)
    holes = np.flatnonzero(spiked < 0)
    spiked[holes[0]], spiked[holes[1]], spiked[holes[2]] = -5, counts[5], 1 << 30
    over = scene.row(1, 100)
    holes = np.flatnonzero(over < 0)                            # counts[2], counts[3] clamp to cap: CAP itself is no match
    over[holes[0]], over[holes[-1]], over[holes[5]] = CAP, 1 << 30, -5
    same = np.full(CAP, -1, np.int32)
    same[:40] = np.arange(40)
    pairs = [(0, 1), (-1, 1), (0, 1), (0, NFRAMES), (2, 3), (4, 5), (10, 11), (6, 1), (0, 1), (8, 9)]
    rows = [normal, normal, normal, normal, over, spiked, same, normal, normal, same]
    model = lvm.verify_batch(oracle, kps, counts, CAP, pairs, rows, scene.has_mp, None)
    w_good, w_mp, w_info = model
    skipped = [0, 0, 0, 0, 0, -1, -1, 0]
    assert w_info[1].tolist() == skipped and w_info[3].tolist() == skipped
    assert w_info[7].tolist() == skipped                                  # counts[6] = -5: a frame without features
    assert w_info[4, 0] == 100 and w_info[5, 0] == 150                    # the hostile values count as no match
    assert w_info[6].tolist() == [40, 0, 0, int(scene.has_mp[10, :40].sum()), 2, -1, -1, 1000]   # no model: an all-0 mask
    assert w_info[9].tolist()[:2] == [40, 40] and w_info[9, 5] == 0
    assert w_info[0, 1] >= 50
    got = run_batch(Track(), kps, counts, pairs, rows, scene.has_mp, None)
    check_equal(got, model, pairs)
    for p in (1, 3, 6, 7):
        assert (got[0][p] == -1).all() and (got[1][p] == -1).all()
    for p in (2, 8):                                                      # the neighbours of the refused pairs
        assert np.array_equal(got[0][p], got[0][0]) and np.array_equal(got[1][p], got[1][0]) and np.array_equal(got[2][p], got[2][0])


# ---- slicing ---------------------------------------------------------------------------------------------------------------
def test_a_batch_of_several_slices(scene, oracle):
    """The scratch of a call is capped at 64 MiB; a pair takes 1000 x (27 + 3) doubles, 1000 x (1 + 7) ints, 21 bytes per
    feature and 16 bytes = 282,768 bytes at cap = 512, so a slice holds 237 pairs at most and 250 pairs run as two slices
    (of 125).  They must come out as in two calls of 100 and 150 pairs, which fit a slice each; pairs either side of the
    boundaries are compared with the model as well."""
    from se2lam_amd.track import Track
    P = 250
    assert (64 << 20) // (1000 * (30 * 8 + 8 * 4) + CAP * 21 + 16) == 237 < P
    pairs = [(2 * (p % 6), 2 * (p % 6) + 1) for p in range(P)]
    rows = [scene.row(p % 6, 15 + p % 11) for p in range(P)]
    tr = Track()
    whole = run_batch(tr, scene.kps, scene.counts, pairs, rows, scene.has_mp, scene.num_mps)
    first = run_batch(tr, scene.kps, scene.counts, pairs[:100], rows[:100], scene.has_mp, scene.num_mps)
    second = run_batch(tr, scene.kps, scene.counts, pairs[100:], rows[100:], scene.has_mp, scene.num_mps)
    for i in range(3):
        assert np.array_equal(whole[i], np.concatenate([first[i], second[i]]))
    assert (whole[2][:, 0] == [15 + p % 11 for p in range(P)]).all() and (whole[2][:, 4] == 2).all()
    some = [0, 99, 100, 124, 125, 236, 237, 249]
    model = lvm.verify_batch(oracle, scene.kps, scene.counts, CAP, [pairs[p] for p in some], [rows[p] for p in some], scene.has_mp,
                             scene.num_mps)
    check_equal(tuple(x[some] for x in whole), model, [pairs[p] for p in some])


# ---- chain: SearchByBoW and the verification on one stream ------------------------------------------------------------------
CHAIN_CAP = 1024
CHAIN_PAIRS = [(0, 1), (1, 0), (0, 2), (2, 5), (3, 3), (0, 5), (4, 1)]


def _feature_vector(desc, nbits):
    """Stand-in for DBoW2::FeatureVector (tests/test_search_bow_batch_gpu.py): node = the first `nbits` descriptor bits; CSR
    with ascending node ids."""
    node = (desc[:, 0].astype(np.int32) | (desc[:, 1].astype(np.int32) << 8)) & ((1 << nbits) - 1)
    order = np.argsort(node, kind="stable")
    nodes, counts = np.unique(node[order], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return nodes.astype(np.int32), ptr, order.astype(np.int32)


def test_search_by_bow_then_verify_on_one_stream(oracle, synth):
    from se2lam_amd import capi
    from se2lam_amd.matcher import ORBmatcher
    from se2lam_amd.track import Track
    D = capi.DeviceArray
    feats = [oracle.orb_extract(synth.frame(t)) for t in range(6)]
    fvs = [_feature_vector(d, 7) for _, d in feats]
    B, cap, P = len(feats), CHAIN_CAP, len(CHAIN_PAIRS)
    rng = np.random.default_rng(5)
    kps, desc = np.zeros((B, cap), capi.KP_DTYPE), np.zeros((B, cap, 32), np.uint8)
    cnt, nnodes = np.zeros(B, np.int32), np.zeros(B, np.int32)
    nodes, ptr, idx = np.zeros((B, cap), np.int32), np.zeros((B, cap + 1), np.int32), np.zeros((B, cap), np.int32)
    for f, ((k, d), (fn, fp, fi)) in enumerate(zip(feats, fvs)):
        n = len(k)
        kps[f, :n], desc[f, :n], cnt[f] = k, d, n
        nodes[f, :len(fn)], ptr[f, :len(fp)], idx[f, :len(fi)], nnodes[f] = fn, fp, fi, len(fn)
    has_mp = (rng.random((B, cap)) < 0.6).astype(np.uint8)
    dev = [D.from_numpy(a) for a in (kps, desc, cnt, nodes, ptr, idx, nnodes, has_mp)]
    d_kps, d_desc, d_cnt, d_nodes, d_ptr, d_idx, d_nn, d_has = dev
    d_pa = D.from_numpy(np.array([p[0] for p in CHAIN_PAIRS], np.int32))
    d_pb = D.from_numpy(np.array([p[1] for p in CHAIN_PAIRS], np.int32))
    d_m, d_nm = D.from_numpy(np.full((P, cap), SENTINEL, np.int32)), D.from_numpy(np.full(P, SENTINEL, np.int32))
    d_good, d_mp = D.from_numpy(np.full((P, cap), SENTINEL, np.int32)), D.from_numpy(np.full((P, cap), SENTINEL, np.int32))
    d_info = D.from_numpy(np.full((P, 8), SENTINEL, np.int32))
    mt = ORBmatcher(0.6, max_features=cap, max_batch=8)
    tr = Track()
    tr.set_stream(mt.stream())
    mt.search_by_bow_batch_device(d_kps.ptr, d_desc.ptr, d_cnt.ptr, cap, B, d_nodes.ptr, d_ptr.ptr, d_idx.ptr, d_nn.ptr, None,
                                  d_pa.ptr, d_pb.ptr, P, d_m.ptr, d_nm.ptr, bIfMPOnly=False)
    tr.loop_verify_batch_device(d_kps.ptr, d_cnt.ptr, cap, B, d_has.ptr, None, d_pa.ptr, d_pb.ptr, P, d_m.ptr, d_good.ptr, d_mp.ptr,
                                d_info.ptr)
    tr.sync()                                                            # the one wait of the chain
    got = (d_good.to_numpy(np.int32, (P, cap)), d_mp.to_numpy(np.int32, (P, cap)), d_info.to_numpy(np.int32, (P, 8)))
    rows = []
    for a, b in CHAIN_PAIRS:
        (k1, d1), (k2, d2) = feats[a], feats[b]
        m_ref, nm_ref = oracle.search_by_bow(k1, d1, fvs[a], has_mp[a, :len(k1)], k2, d2, fvs[b], has_mp[b, :len(k2)], False, 0.6, True)
        assert nm_ref >= 400
        rows.append(np.concatenate([m_ref, np.full(cap - len(m_ref), -1, np.int32)]))
    assert np.array_equal(d_m.to_numpy(np.int32, (P, cap)), np.stack(rows))
    model = lvm.verify_batch(oracle, kps, cnt, cap, CHAIN_PAIRS, rows, has_mp, None)
    check_equal(got, model, CHAIN_PAIRS)
    assert (model[2][:, 1] >= 45).all() and (model[2][:, 2] > 0).all()    # every pair is a loop the Localizer would accept
    tr.set_stream(None)
