"""tests/track_frame_model.py, the numpy statement of se2gpu_track_frames_batch_device, on the CPU: against the oracle's
removeOutliers + doTriangulate, against results of the compiled reference's Track::doTriangulate recorded in
tests/golden/track_frame_ref.npz (tools/gen_track_frame_golden.py), rule by rule on hand-stated cases, and the properties that
the cases of the GPU test (tests/track_frame_cases.py) are there for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_frame_cases as tc  # noqa: E402
import track_frame_model as tfm  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_frame_ref.npz")
GOLDEN_SCENES = ((600, 7), (1000, 11), (1, 3), (40, 5))      # (n, seed) of tests/test_triangulate.scene


def _frames(k1, k2, cap):
    kps = np.zeros((2, cap), tc.KP)
    kps[0, :len(k1)], kps[1, :len(k2)] = k1, k2
    return kps, np.array([len(k1), len(k2)], np.int32)


# ---- against the oracle's two member functions -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,frac", [(100, 400, 0.0), (101, 512, 0.3), (102, 333, 0.7), (103, 12, 0.0), (104, 9, 0.0)])
def test_model_equals_remove_outliers_then_triangulate(oracle, synth, seed, n, frac):
    """has_obs and the flag clear: the model is oracle.remove_outliers followed by oracle.triangulate"""
    p1, p2, _ = synth.two_view_matches(seed, n, frac)
    rng = np.random.default_rng(seed)
    k1, k2 = np.zeros(n, tc.KP), np.zeros(n, tc.KP)
    perm = rng.permutation(n)
    k1["x"], k1["y"] = p1[:, 0], p1[:, 1]
    k2["x"][perm], k2["y"][perm] = p2[:, 0], p2[:, 1]
    match = perm.astype(np.int32)
    match[::7] = -1
    cap = n + 5
    kps, counts = _frames(k1, k2, cap)
    row = np.concatenate([match, np.full(5, 3, np.int32)])              # entries from counts[a] on count as -1
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (-200.0, 0.0, 0.0)
    Trc = np.linalg.inv(T.astype(np.float64))[:3].astype(np.float32).reshape(-1)
    P = (tc.K @ T[:3]).astype(np.float32).reshape(-1)
    got = tfm.track_pair(oracle, kps, counts, cap, 0, 1, row, Trc, P, tc.P_REF, 500.0, 8000.0, 2)
    m, ni = oracle.remove_outliers(k1, k2, match)
    pos, good, m2, ng, nold = oracle.triangulate(k1, k2, m, None, tc.P_REF, P, Trc[[3, 7, 11]], 500.0, 8000.0, 2)
    assert got[3][1] == ni and got[3][2] == nold == 0 and got[3][3] == ng
    assert np.array_equal(got[0][:n], m2) and (got[0][n:] == -1).all()
    assert got[1][:n].tobytes() == pos.tobytes() and not got[1][n:].any()
    assert np.array_equal(got[2][:n], good) and not got[2][n:].any()
    assert got[3][0] == int((match >= 0).sum()) and got[3][6] == int(((m >= 0) & (m2 < 0)).sum())
    assert got[3][7] == (tfm.RUN if ni >= 10 else tfm.FEW_INLIERS)
    if n >= 300 and frac < 0.5:
        assert ni >= 100


# ---- against the compiled reference -----------------------------------------------------------------------------------------
def golden_case(n, seed):
    """the batch of one pair that states test_triangulate.scene(n, seed) for the model -> (arguments of track_pair, X, K, Tcr)"""
    from test_triangulate import scene
    k1, k2, match, has_obs, P1, P2, Ocam, X = scene(n, seed)
    th = 0.03
    Tcr = np.eye(4, dtype=np.float32)
    Tcr[:3, :3] = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float32)
    Tcr[:3, 3] = np.array([-150.0, 5.0, 20.0], np.float32)
    kps, counts = _frames(k1, k2, n)
    Trc = np.zeros(12, np.float32)
    Trc[[3, 7, 11]] = Ocam
    obs = np.stack([has_obs, np.zeros(n, np.uint8)])
    view = np.stack([X.astype(np.float32), np.zeros((n, 3), np.float32)])
    return dict(kps=kps, counts=counts, cap=n, a=0, b=1, row=match, Trc=Trc, P=P2.reshape(-1), P_ref=P1.reshape(-1), lower=500.0,
                upper=8000.0, min_degree=2, kf_observed=obs, view_pos=view), (k1, k2, match, has_obs, X.astype(np.float32), Tcr)


@pytest.mark.parametrize("n,seed", GOLDEN_SCENES)
def test_model_equals_the_compiled_do_triangulate(oracle, n, seed):
    """Positions, flags, updated matches and both counts of Track::doTriangulate as the reference's own sources compute them
    (recorded by tools/gen_track_frame_golden.py).  The scenes are exact projections, so with 10 matches or more the filter
    keeps every match and the model's triangulation sees the rows the reference saw; n = 1 is dropped by the filter, there the
    record is only checked to be the single match it is.  Matches, flags and counts are equal; positions agree to 1e-5 of the
    largest coordinate, what OpenCV's float Jacobi SVD and the FP64 one share (tests/test_ref_compiled.py uses the same bound);
    positions of observed features are the key frame's map points, bit for bit."""
    args, (k1, k2, match, has_obs, X, Tcr) = golden_case(n, seed)
    g = np.load(GOLDEN)
    tag = "n%d_s%d_" % (n, seed)
    pos, good, m, ng, nold = g[tag + "pos"], g[tag + "good"], g[tag + "match"], int(g[tag + "counts"][0]), int(g[tag + "counts"][1])
    got = tfm.track_pair(oracle, **args)
    if n < 10:
        assert got[3].tolist() == [int((match >= 0).sum()), 0, 0, 0, int(has_obs.sum()), 0, 0, tfm.FEW_INLIERS]
        assert len(m) == n
        return
    assert got[3][0] == got[3][1] == int((match >= 0).sum()) and got[3][7] == tfm.RUN
    assert (got[3][2], got[3][3]) == (nold, ng) and np.array_equal(got[0], m) and np.array_equal(got[2], good)
    seen = (match >= 0) & (has_obs == 1)
    assert got[1][seen].tobytes() == X[seen].tobytes() and np.array_equal(pos[seen], X[seen])
    acc = (match >= 0) & (has_obs == 0) & (m >= 0)
    assert acc.any() and np.abs(got[1][acc] - pos[acc]).max() <= 1e-5 * np.abs(pos[acc]).max()
    assert not got[1][~(seen | acc)].any() and (pos[~(seen | acc)] == -1).all()
    assert got[3][6] == int(((match >= 0) & (has_obs == 0) & (m < 0)).sum())


def test_the_compiled_reference_still_gives_the_golden_results():
    """where the compiled reference is present: it reproduces the recorded arrays"""
    from oracle import ref
    if not os.path.exists(ref.LIB_MAP):
        return
    g = np.load(GOLDEN)
    K = np.array([[400.0, 0, 320.0], [0, 400.0, 240.0], [0, 0, 1]], np.float32)
    for n, seed in GOLDEN_SCENES:
        _, (k1, k2, match, has_obs, X, Tcr) = golden_case(n, seed)
        pos, good, m, ng, nold = ref.track_triangulate(K, k1, k2, match, has_obs, X, Tcr, 500.0, 8000.0)
        tag = "n%d_s%d_" % (n, seed)
        assert np.array_equal(pos, g[tag + "pos"]) and np.array_equal(good, g[tag + "good"]) and np.array_equal(m, g[tag + "match"])
        assert [ng, nold] == g[tag + "counts"].tolist()


# ---- rule by rule -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return tc.main_scene()


def _pair(oracle, sc, a, b, row, k=0, with_obs=True, flag=0, counts=None, lower=tc.LOWER, upper=tc.UPPER, min_degree=2):
    Trc, P = sc.pose(k)
    return tfm.track_pair(oracle, sc.kps, sc.counts if counts is None else counts, sc.cap, a, b, row, Trc, P, tc.P_REF, lower, upper,
                          min_degree, sc.kf_observed if with_obs else None, sc.view_pos if with_obs else None, flag)


def test_rule_1_raw_matches(oracle, scene):
    """entries from counts[a] on, negative values and values from counts[b] on count as -1; counts are clamped to 0..cap"""
    row = scene.row(1, 100)
    base = _pair(oracle, scene, 2, 3, row, k=1)
    assert base[3][0] == 100 and base[3][7] == tfm.RUN
    hostile = row.copy()
    holes = np.flatnonzero(hostile[:scene.counts[2]] < 0)
    hostile[holes[0]], hostile[holes[1]], hostile[holes[2]] = -5, scene.counts[3], 1 << 30
    hostile[scene.counts[2]:] = 5
    got = _pair(oracle, scene, 2, 3, hostile, k=1)
    for x, y in zip(got, base):
        assert x.tobytes() == y.tobytes()
    counts = scene.counts.copy()
    counts[2], counts[3] = scene.cap + 1000, 2**31 - 1                  # clamp to cap: the filler features become features
    big = _pair(oracle, scene, 2, 3, row, k=1, counts=counts)
    assert big[3][0] == 100 and big[3][4] == int(scene.kf_observed[2].sum())
    counts[2] = -5
    assert _pair(oracle, scene, 2, 3, row, k=1, counts=counts)[3].tolist() == [0, 0, 0, 0, 0, 0, 0, tfm.FEW_INLIERS]


def test_rule_2_filter(oracle, scene):
    """fewer than 10 raw matches, or fewer than 10 inliers among more: rows of -1, zero positions and flags, inlier count 0;
    otherwise exactly the entries the oracle's mask keeps"""
    for n_raw, path in ((0, 0), (9, 0), (10, 1), (14, 1)):
        m, pos, good, info = _pair(oracle, scene, 4, 5, scene.row(2, n_raw), k=2)
        assert info[0] == n_raw and info[5] == path
        if info[1] == 0:
            assert info[7] == tfm.FEW_INLIERS and (m == -1).all() and not pos.any() and not good.any() and not info[[2, 3, 6]].any()
    row = scene.row(0, 200)
    m, pos, good, info = _pair(oracle, scene, 0, 1, row, with_obs=False, lower=-1e9, upper=1e9)   # no depth rejection
    src = np.flatnonzero(row[:scene.counts[0]] >= 0)
    p1 = np.stack([scene.kps["x"][0, src], scene.kps["y"][0, src]], 1)
    p2 = np.stack([scene.kps["x"][1, row[src]], scene.kps["y"][1, row[src]]], 1)
    mask, ni = oracle.fundamental_mask(p1, p2)
    assert 10 <= ni < 200 and info[1] == ni and info[6] == 0
    assert np.array_equal(np.flatnonzero(m >= 0), src[mask.astype(bool)]) and np.array_equal(m[m >= 0], row[src[mask.astype(bool)]])


def test_rule_3_triangulation(oracle, scene):
    row = scene.row(1, 250)
    na = scene.counts[2]
    m, pos, good, info = _pair(oracle, scene, 2, 3, row, k=1)
    m0, pos0, good0, info0 = _pair(oracle, scene, 2, 3, row, k=1, with_obs=False)
    obs = scene.kf_observed[2] != 0
    old = (m >= 0) & obs
    # observed features: the key frame's map point whatever its depth, never good parallax, counted
    assert info[2] == old.sum() > 0 and pos[old].tobytes() == scene.view_pos[2][old].tobytes() and not good[old].any()
    assert info[4] == obs[:na].sum() and info0[4] == 0 and info0[2] == 0
    # the others: as without the table
    new = ~obs
    assert np.array_equal(m[new], m0[new]) and pos[new].tobytes() == pos0[new].tobytes() and np.array_equal(good[new], good0[new])
    # depth gate: accepted positions lie inside, rejected matches are -1 with zero position, and they are counted
    acc = (m0 >= 0)
    assert ((pos0[acc, 2] >= tc.LOWER) & (pos0[acc, 2] <= tc.UPPER)).all() and not pos0[~acc].any() and not good0[~acc].any()
    wide = _pair(oracle, scene, 2, 3, row, k=1, with_obs=False, lower=-1e9, upper=1e9)
    assert wide[3][6] == 0 and info0[6] == (wide[0] >= 0).sum() - acc.sum() > 0
    gone = (wide[0] >= 0) & ~acc
    assert ((wide[1][gone, 2] < tc.LOWER) | (wide[1][gone, 2] > tc.UPPER)).all()
    # parallax: cos of the angle at the point between the two centres, against minCos[min_degree - 1]
    Ocam = scene.pose(1)[0][[3, 7, 11]].astype(np.float64)
    p = pos0[acc].astype(np.float64)
    cosp = np.abs((p * (p - Ocam)).sum(1)) / (np.linalg.norm(p, axis=1) * np.linalg.norm(p - Ocam, axis=1))
    for mind, mc in ((1, 0.9998), (2, 0.9994), (3, 0.9986), (4, 0.9976)):
        g = _pair(oracle, scene, 2, 3, row, k=1, with_obs=False, min_degree=mind)
        clear = np.abs(cosp - mc) > 1e-6
        assert np.array_equal(g[2][acc][clear] != 0, cosp[clear] < mc) and g[3][3] == g[2].sum()
    # flag bit 0: the filtered row, nothing else
    f = _pair(oracle, scene, 2, 3, row, k=1, flag=1)
    assert f[3].tolist() == [info[0], info[1], 0, 0, info[4], 2, 0, tfm.SKIPPED] and not f[1].any() and not f[2].any()
    assert np.array_equal(f[0], wide[0]) and (f[0] >= 0).sum() == info[1]
    for x, y in zip(_pair(oracle, scene, 2, 3, row, k=1, flag=2), (m, pos, good, info)):
        assert x.tobytes() == y.tobytes()


def test_rule_4_frames_out_of_range(oracle, scene):
    for a, b in ((-1, 1), (0, scene.nframes), (scene.nframes, -7)):
        m, pos, good, info = _pair(oracle, scene, a, b, scene.row(0, 200), flag=1)
        assert info.tolist() == [0, 0, 0, 0, 0, 0, 0, tfm.BAD_FRAME] and (m == -1).all() and not pos.any() and not good.any()


# ---- the cases of the GPU test have the properties they are there for --------------------------------------------------------
def test_the_direct_batch_has_its_properties(oracle, scene):
    b, names = tc.direct_batch(scene)
    m, pos, good, info = b.model(tfm, oracle, scene)
    assert scene.cap % 256 != 0 and scene.nframes == 12 and (scene.counts < scene.cap).all()
    assert 0.25 < scene.kf_observed.mean() < 0.42
    assert info[:9, 0].tolist() == list(tc.RAW_COUNTS) and info[:9, 5].tolist() == list(tc.PATHS)
    by = {v: k for k, v in names.items()}
    few = by["few inliers"]
    assert info[few, 0] >= 10 and info[few, 1] == 0 and info[few, 5] == 2 and info[few, 7] == tfm.FEW_INLIERS
    row = b.rows[few]
    src = np.flatnonzero(row >= 0)
    p1 = np.stack([scene.kps["x"][0, src], scene.kps["y"][0, src]], 1); p2 = np.stack([scene.kps["x"][3, row[src]], scene.kps["y"][3, row[src]]], 1)
    assert 0 < oracle.fundamental_mask(p1, p2)[1] < 10                    # a mask with inliers, too few of them
    for p in (6, 7, 8):
        acc = (m[p] >= 0) & (scene.kf_observed[b.pairs[p][0]] == 0)
        assert info[p, 7] == tfm.RUN and info[p, 6] >= 1 and info[p, 2] >= 1             # depth rejections, tracked old points
        assert good[p][acc].any() and not good[p][acc].all() and info[p, 3] == good[p].sum()   # both values of good_prl
    assert info[by["flagged"], 7] == tfm.SKIPPED and info[by["flagged"], 1] >= 10
    assert info[by["frame past the end"], 7] == info[by["negative frame"], 7] == tfm.BAD_FRAME
    assert b.pairs[by["(f, f)"]][0] == b.pairs[by["(f, f)"]][1] and info[by["(f, f)"], 7] == tfm.RUN
    assert info[by["repeat of 8"]].tolist() == info[8].tolist()
    assert info[by["flag without bit 0"], 7] == tfm.RUN
    assert sorted(set(info[:, 7].tolist())) == [0, 1, 2, 3]


def test_the_slice_batch_has_its_properties(oracle):
    sc = tc.slice_scene()
    b, busy = tc.slice_batch(sc)
    assert len(b.pairs) == tc.SLICE_PAIRS == 260
    n_raw = np.array([(r >= 0).sum() for r in b.rows])
    assert (n_raw < 10).sum() > 200                                       # most of them take path 0
    info = b.take(busy).model(tfm, oracle, sc)[3]
    assert (info[:, 7] == tfm.RUN).all() and (info[:, 1] >= 10).all() and {129, 130, 244, 245} <= set(busy)
