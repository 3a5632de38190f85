"""se2gpu_track_frames_batch_device (Track::removeOutliers + Track::doTriangulate over a batch of frame pairs in HBM) against
tests/track_frame_model.py: every output word - match rows, positions (compared as bit patterns), parallax flags and the 8 info
words - is compared EXACTLY.  The scenes and what each pair is there for: tests/track_frame_cases.py, whose properties
tests/test_track_frame_model.py asserts on the CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_frame_cases as tc  # noqa: E402
import track_frame_model as tfm  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = tc.SENTINEL


class DeviceScene:
    """the frame tables of a scene in device memory, uploaded once"""

    def __init__(self, sc):
        from se2lam_amd import capi
        D = capi.DeviceArray
        self.sc = sc
        self.kps, self.counts = D.from_numpy(sc.kps), D.from_numpy(sc.counts)
        self.obs, self.view = D.from_numpy(sc.kf_observed), D.from_numpy(sc.view_pos)


def run_batch(track, ds, batch, with_obs=True, sync=True, lower=tc.LOWER, upper=tc.UPPER, min_degree=tc.MIN_DEGREE):
    """one call -> (matched12 (P, cap), local_pos (P, cap, 3), good_prl (P, cap), info (P, 8)); the outputs start as SENTINEL"""
    from se2lam_amd import capi
    D = capi.DeviceArray
    sc, P = ds.sc, len(batch.pairs)
    cap = sc.cap
    d_pa = D.from_numpy(np.array([p[0] for p in batch.pairs], np.int32))
    d_pb = D.from_numpy(np.array([p[1] for p in batch.pairs], np.int32))
    d_Trc, d_P = D.from_numpy(np.stack(batch.Trc).astype(np.float32)), D.from_numpy(np.stack(batch.P).astype(np.float32))
    d_flags = D.from_numpy(np.array(batch.flags, np.uint8)) if any(batch.flags) else None
    d_rows = D.from_numpy(np.stack(batch.rows).astype(np.int32))
    d_m = D.from_numpy(np.full((P, cap), SENT, np.int32))
    d_pos = D.from_numpy(np.full((P, cap, 3), float(SENT), np.float32))
    d_good = D.from_numpy(np.full((P, cap), SENT, np.uint8))
    d_info = D.from_numpy(np.full((P, 8), SENT, np.int32))
    track.track_frames_batch_device(ds.kps.ptr, ds.counts.ptr, cap, sc.nframes, ds.obs.ptr if with_obs else None,
                                    ds.view.ptr if with_obs else None, d_pa.ptr, d_pb.ptr, P, d_Trc.ptr, d_P.ptr,
                                    d_flags and d_flags.ptr, tc.P_REF, d_rows.ptr, lower, upper, min_degree, d_m.ptr, d_pos.ptr,
                                    d_good.ptr, d_info.ptr)
    track.sync()
    return (d_m.to_numpy(np.int32, (P, cap)), d_pos.to_numpy(np.float32, (P, cap, 3)), d_good.to_numpy(np.uint8, (P, cap)),
            d_info.to_numpy(np.int32, (P, 8)))


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_equal(got, want, pairs):
    for p, pair in enumerate(pairs):
        print("pair %d %s: device %s model %s" % (p, pair, got[3][p].tolist(), want[3][p].tolist()))
    for p, pair in enumerate(pairs):
        assert np.array_equal(got[3][p], want[3][p]), (p, pair)
        assert np.array_equal(got[0][p], want[0][p]), (p, pair)
        assert same_bytes(got[1][p], want[1][p]), (p, pair, np.abs(got[1][p] - want[1][p]).max())
        assert np.array_equal(got[2][p], want[2][p]), (p, pair)


@pytest.fixture(scope="module")
def scene():
    return tc.main_scene()


@pytest.fixture(scope="module")
def dscene(scene):
    return DeviceScene(scene)


@pytest.fixture(scope="module")
def direct(scene, oracle):
    b, names = tc.direct_batch(scene)
    return b, names, b.model(tfm, oracle, scene), b.model(tfm, oracle, scene, with_obs=False)


# ---- direct ---------------------------------------------------------------------------------------------------------------
def test_direct(scene, dscene, direct):
    """Raw counts 0..300 on paths 0, 1 and 2, a repeated pair, (f, f), a flagged pair, two pairs out of range and one whose mask
    has fewer than 10 inliers; with the observation table (a third of the features observed) and without it.  The outputs
    start as a sentinel, so a word that is not written differs from the model."""
    from se2lam_amd.track import Track
    b, names, model, model_0 = direct
    tr = Track()
    got = run_batch(tr, dscene, b)
    check_equal(got, model, b.pairs)
    assert same_bytes(got[1][8], got[1][9]) and np.array_equal(got[3][8], got[3][9]) and np.array_equal(got[0][8], got[0][9])
    for p, (a, _) in enumerate(b.pairs):
        na = scene.counts[a] if 0 <= a < scene.nframes else 0
        assert (got[0][p, na:] == -1).all() and not got[1][p, na:].any() and not got[2][p, na:].any()
    got_0 = run_batch(tr, dscene, b, with_obs=False)
    check_equal(got_0, model_0, b.pairs)
    assert (got_0[3][:, 2] == 0).all() and (got_0[3][:, 4] == 0).all()


def test_other_parallax_thresholds_and_depth_bounds(scene, dscene, oracle):
    """min_degree 1 and 4 (the ends of cvu::checkParallax's table) and a narrower depth gate"""
    from se2lam_amd.track import Track
    b, _ = tc.direct_batch(scene)
    b = b.take([6, 7, 8])
    tr = Track()
    for mind, lo, hi in ((1, 500.0, 8000.0), (4, 1500.0, 4000.0)):
        want = tfm.track_batch(oracle, scene.kps, scene.counts, scene.cap, b.pairs, b.rows, b.Trc, b.P, tc.P_REF, lo, hi, mind,
                               scene.kf_observed, scene.view_pos, b.flags)
        check_equal(run_batch(tr, dscene, b, lower=lo, upper=hi, min_degree=mind), want, b.pairs)


def test_a_pair_gives_the_same_bytes_wherever_it_stands(scene, dscene, direct):
    """pair 8 (300 raw matches) and pair 7 alone, as pair 0, as pair 2 of 3, and in a second run"""
    from se2lam_amd.track import Track
    b, _, model, _ = direct
    tr = Track()
    for q in (8, 7):
        alone = run_batch(tr, dscene, b.take([q]))
        first = run_batch(tr, dscene, b.take([q, 5, 6]))
        third = run_batch(tr, dscene, b.take([5, 11, q]))
        again = run_batch(tr, dscene, b.take([5, 11, q]))
        for k in range(4):
            assert same_bytes(alone[k][0], first[k][0]) and same_bytes(alone[k][0], third[k][2])
            assert same_bytes(third[k], again[k])
        check_equal(alone, tuple(x[[q]] for x in model), [b.pairs[q]])


# ---- hostile inputs --------------------------------------------------------------------------------------------------------
def test_hostile_inputs(scene, oracle):
    """counts beyond cap and below 0 (clamped), match values below -1, at counts[b] and far beyond, values behind counts[a]"""
    from se2lam_amd.track import Track
    sc = tc.main_scene()
    sc.counts[2], sc.counts[3], sc.counts[6] = sc.cap + 1000, 2**31 - 1, -5
    b = tc.Batch()
    b.add((0, 1), sc.row(0, 100), sc.pose(0))
    over = sc.row(1, 100)
    holes = np.flatnonzero(over < 0)                            # counts[2], counts[3] clamp to cap: cap itself is no match
    over[holes[0]], over[holes[-1]], over[holes[5]] = sc.cap, 1 << 30, -5
    b.add((2, 3), over, sc.pose(1))
    spiked = sc.row(2, 150)
    holes = np.flatnonzero(spiked < 0)
    spiked[holes[0]], spiked[holes[1]], spiked[holes[2]] = -5, sc.counts[5], 1 << 30
    spiked[sc.counts[4]:] = 5
    b.add((4, 5), spiked, sc.pose(2))
    b.add((6, 1), sc.row(0, 100), sc.pose(0))                   # counts[6] = -5: a frame without features
    b.add((0, 1), sc.row(0, 100), sc.pose(0))
    want = b.model(tfm, oracle, sc)
    assert want[3][1, 0] == 100 and want[3][2, 0] == 150 and want[3][3].tolist() == [0, 0, 0, 0, 0, 0, 0, tfm.FEW_INLIERS]
    assert want[3][1, 4] == int(sc.kf_observed[2].sum())
    got = run_batch(Track(), DeviceScene(sc), b)
    check_equal(got, want, b.pairs)
    for k in range(4):
        assert same_bytes(got[k][0], got[k][4])


# ---- slicing ---------------------------------------------------------------------------------------------------------------
def test_a_batch_of_several_slices(oracle):
    """The filter's scratch is capped at 64 MiB; a pair takes 1000 x (27 + 3) doubles, 1000 x (1 + 7) ints, 21 bytes per feature
    and 16 bytes = 273,360 bytes at cap = 64, so a slice holds 245 pairs at most and 260 pairs run as two slices (of 130).  They
    must come out as in two calls of 100 and 160 pairs, which fit a slice each; the pairs with matches - among them those either
    side of the boundaries - are compared with the model, the others are empty rows."""
    from se2lam_amd.track import Track
    sc = tc.slice_scene()
    ds = DeviceScene(sc)
    b, busy = tc.slice_batch(sc)
    P = tc.SLICE_PAIRS
    assert (64 << 20) // (1000 * (30 * 8 + 8 * 4) + tc.SLICE_CAP * 21 + 16) == 245 < P
    tr = Track()
    whole = run_batch(tr, ds, b)
    first = run_batch(tr, ds, b.take(range(100)))
    second = run_batch(tr, ds, b.take(range(100, P)))
    for k in range(4):
        assert same_bytes(whole[k], np.concatenate([first[k], second[k]]))
    some = sorted(set(busy) | set(range(0, P, 13)))
    check_equal(tuple(x[some] for x in whole), b.take(some).model(tfm, oracle, sc), [b.pairs[p] for p in some])
    rest = [p for p in range(P) if p not in some]
    assert (whole[3][rest, 0] == [p % 10 for p in rest]).all() and (whole[3][rest, 7] == tfm.FEW_INLIERS).all()
    assert (whole[0][rest] == -1).all() and not whole[1][rest].any() and not whole[2][rest].any()


# ---- the single calls on the same handle ------------------------------------------------------------------------------------
def test_single_calls_on_the_handle_are_unchanged_by_a_batch_call(scene, dscene, direct, oracle):
    """se2gpu_track_remove_outliers, se2gpu_track_triangulate and se2gpu_track_loop_verify_batch_device give the same bytes
    before and after a batch call on the same handle - and the single calls on the downloaded arrays are the host route the
    batch call replaces: they give the batch's outputs for the pair."""
    import test_loop_verify_gpu as lv
    from se2lam_amd import capi
    from se2lam_amd.track import Track
    b, _, model, model_0 = direct
    tr = Track()
    q = 8
    (fa, fb), row = b.pairs[q], b.rows[q]
    na, nb = scene.counts[fa], scene.counts[fb]

    def singles():
        m = row[:na].copy()
        ni = tr.removeOutliers(scene.kps[fa, :na], scene.kps[fb, :nb], m)
        tri = tr.doTriangulate(scene.kps[fa, :na], scene.kps[fb, :nb], m, scene.kf_observed[fa, :na], tc.P_REF, b.P[q],
                               b.Trc[q][[3, 7, 11]], tc.LOWER, tc.UPPER, tc.MIN_DEGREE)
        return (m, ni) + tri

    def loop_verify():
        return lv.run_batch(tr, scene.kps, scene.counts, [b.pairs[p] for p in (5, 6, 8)], [b.rows[p] for p in (5, 6, 8)],
                            scene.kf_observed, None)

    before, lv_before = singles(), loop_verify()
    got = run_batch(tr, dscene, b)
    after, lv_after = singles(), loop_verify()
    for x, y in zip(before, after):
        assert same_bytes(np.asarray(x), np.asarray(y))
    for x, y in zip(lv_before, lv_after):
        assert same_bytes(x, y)
    check_equal(got, model, b.pairs)
    m_filtered, ni, pos, good, m_final, ng, nold = after
    assert [ni, nold, ng] == got[3][q, 1:4].tolist()
    assert np.array_equal(m_final, got[0][q, :na]) and np.array_equal(good, got[2][q, :na])
    old = (m_final >= 0) & (scene.kf_observed[fa, :na] != 0)
    pos = pos.copy()
    pos[old] = scene.view_pos[fa, :na][old]                      # the single call leaves the key frame's map points to the caller
    assert same_bytes(pos, got[1][q, :na])


# ---- chain: extract, MatchByWindow and this call on one stream --------------------------------------------------------------
def test_extract_match_track_on_one_stream(oracle, synth):
    """se2gpu_orb_extract_batch_device on four synthetic 640x480 frames -> se2gpu_match_window_batch_device -> this call, all on
    the extractor's stream with one wait.  It equals the same calls with a wait after each, the model, and the host route
    (download, then se2gpu_track_remove_outliers + se2gpu_track_triangulate per pair)."""
    from se2lam_amd import capi
    from se2lam_amd.matcher import ORBmatcher
    from se2lam_amd.orb import ORBextractor, KP_DTYPE
    from se2lam_amd.track import Track
    D = capi.DeviceArray
    B, cap = 4, 1024
    pairs = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0)]
    P = len(pairs)
    imgs = synth.frames(B)
    rng = np.random.default_rng(11)
    obs = (rng.random((B, cap)) < 1 / 3).astype(np.uint8)
    view = rng.uniform(-5000, 5000, (B, cap, 3)).astype(np.float32)
    sc = tc.main_scene()
    Trc = np.stack([sc.pose(p % 6)[0] for p in range(P)]); Pm = np.stack([sc.pose(p % 6)[1] for p in range(P)])
    flags = np.array([0, 0, 0, 0, 1], np.uint8)
    d_img, d_obs, d_view = D.from_numpy(imgs), D.from_numpy(obs), D.from_numpy(view)
    d_pa = D.from_numpy(np.array([p[0] for p in pairs], np.int32)); d_pb = D.from_numpy(np.array([p[1] for p in pairs], np.int32))
    d_Trc, d_P, d_flags = D.from_numpy(Trc), D.from_numpy(Pm), D.from_numpy(flags)
    ex = ORBextractor(max_batch=B)
    mt = ORBmatcher(0.9, max_features=cap, max_batch=max(B, P))
    tr = Track()

    def chain(wait_each):
        d_kps = D.from_numpy(np.zeros((B, cap), KP_DTYPE)); d_desc = D(B * cap * 32); d_cnt = D.from_numpy(np.zeros(B, np.int32))
        d_rows = D.from_numpy(np.full((P, cap), SENT, np.int32)); d_nm = D.from_numpy(np.full(P, SENT, np.int32))
        d_m = D.from_numpy(np.full((P, cap), SENT, np.int32)); d_pos = D.from_numpy(np.full((P, cap, 3), float(SENT), np.float32))
        d_good = D.from_numpy(np.full((P, cap), SENT, np.uint8)); d_info = D.from_numpy(np.full((P, 8), SENT, np.int32))
        ex.extract_batch_device(d_img.ptr, B, 480, 640, d_kps.ptr, d_desc.ptr, d_cnt.ptr, cap)
        if wait_each:
            ex.sync()
        mt.match_window_batch_device(d_kps.ptr, d_desc.ptr, d_cnt.ptr, cap, d_pa.ptr, d_pb.ptr, P, 20, d_rows.ptr, d_nm.ptr)
        if wait_each:
            mt.sync()
        tr.track_frames_batch_device(d_kps.ptr, d_cnt.ptr, cap, B, d_obs.ptr, d_view.ptr, d_pa.ptr, d_pb.ptr, P, d_Trc.ptr, d_P.ptr,
                                     d_flags.ptr, tc.P_REF, d_rows.ptr, tc.LOWER, tc.UPPER, tc.MIN_DEGREE, d_m.ptr, d_pos.ptr,
                                     d_good.ptr, d_info.ptr)
        tr.sync()                                                        # the one wait of the chain
        return (d_kps.to_numpy(KP_DTYPE, (B, cap)), d_cnt.to_numpy(np.int32, (B,)), d_rows.to_numpy(np.int32, (P, cap)),
                (d_m.to_numpy(np.int32, (P, cap)), d_pos.to_numpy(np.float32, (P, cap, 3)), d_good.to_numpy(np.uint8, (P, cap)),
                 d_info.to_numpy(np.int32, (P, 8))))

    mt.set_stream(ex.stream())
    tr.set_stream(ex.stream())
    kps, cnt, rows, got = chain(False)
    mt.set_stream(None)
    tr.set_stream(None)
    kps_w, cnt_w, rows_w, got_w = chain(True)
    assert same_bytes(kps, kps_w) and same_bytes(cnt, cnt_w) and same_bytes(rows, rows_w)
    for k in range(4):
        assert same_bytes(got[k], got_w[k])
    want = tfm.track_batch(oracle, kps, cnt, cap, pairs, list(rows), Trc, Pm, tc.P_REF, tc.LOWER, tc.UPPER, tc.MIN_DEGREE, obs, view,
                           flags)
    check_equal(got, want, pairs)
    assert (want[3][:, 0] >= 100).all() and want[3][4, 7] == tfm.SKIPPED
    for p, (a, b) in enumerate(pairs[:4]):                               # the host route, pair by pair
        na, nb = cnt[a], cnt[b]
        m = rows[p, :na].copy()
        ni = tr.removeOutliers(kps[a, :na], kps[b, :nb], m)
        pos, good, m2, ng, nold = tr.doTriangulate(kps[a, :na], kps[b, :nb], m, obs[a, :na], tc.P_REF, Pm[p], Trc[p][[3, 7, 11]],
                                                   tc.LOWER, tc.UPPER, tc.MIN_DEGREE)
        old = (m2 >= 0) & (obs[a, :na] != 0)
        pos = pos.copy(); pos[old] = view[a, :na][old]
        assert [ni, nold, ng] == got[3][p, 1:4].tolist()
        assert np.array_equal(m2, got[0][p, :na]) and np.array_equal(good, got[2][p, :na]) and same_bytes(pos, got[1][p, :na])
