"""The numpy model of the new-key-frame calls (tests/new_kf_model.py) held to hand-worked cases, its float32 restatement
held to its FP64 layer, the cases' distance from every threshold, and the header's host functions
(include/se2lam_amd/FindCorrespd.h, through tests/cpp_find_correspd.cpp) held to the restatement.

Measured here (float32 restatement against the FP64 layer, cases of tests/new_kf_cases.py): positions 1.1e-6 of their norm,
informations 2.3e-6 of their largest entry at worst; the device is allowed four times the figure measured in the run."""
import numpy as np
import pytest

import new_kf_cases as nc
import new_kf_model as nk

EYE = nk.EYE12


def _shift_x(t):
    """Tcw of a camera at world (t, 0, 0) without rotation, its inverse"""
    Tcw, Twc = np.eye(4, dtype=np.float32)[:3].copy(), np.eye(4, dtype=np.float32)[:3].copy()
    Tcw[0, 3], Twc[0, 3] = -t, t
    return Tcw.ravel(), Twc.ravel()


@pytest.mark.parametrize("L", [nk.L64, nk.L32])
def test_point_on_the_optical_axis_has_a_diagonal_information(L):
    """xyz1 = (e, 0, 4) in camera 1 (the identity), camera 2 one unit along x.  R1 is the identity - for FP64 by the limit at
    e = 0, for the restatement through cv::Rodrigues' branch below DBL_EPSILON at e = 1e-20 - so info1 = diag(1 / dxy1^2,
    1 / dxy1^2, 1 / dz1^2) with dxy1 = 2 * 4 / fx, sinParallax = 1 / sqrt(17), dxy2 = 2 sqrt(17) / fx, dz1 = dxy2 / sinParallax
    = 34 / fx."""
    fx = 200.0
    Tcw2, Twc2 = _shift_x(1.0)
    e = 0.0 if L is nk.L64 else 1e-20
    info1, info2, xyz2 = L.se3_to_xyz_info([e, 0.0, 4.0], EYE, Tcw2, Twc2, fx)
    want = np.diag([(fx / 8.0) ** 2, (fx / 8.0) ** 2, (fx / 34.0) ** 2])
    assert np.allclose(info1, want, rtol=2e-6, atol=1e-9 * want.max())
    assert np.allclose(xyz2, [-1.0, 0.0, 4.0], atol=1e-6)
    # camera 2 sees the point 14.04 degrees off its axis: info2 = R2^T diag(1 / dxy2^2, 1 / dxy2^2, 1 / dz2^2) R2 with
    # dz2 = dxy1 / sinParallax = 8 sqrt(17) / fx and R2 the rotation about y that turns (-1, 0, 4) onto z
    c, s = 4 / np.sqrt(17), 1 / np.sqrt(17)
    R2 = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    assert np.allclose(R2 @ [-1, 0, 4], [0, 0, np.sqrt(17)])
    D2 = np.diag([fx ** 2 / 68.0, fx ** 2 / 68.0, fx ** 2 / (64 * 17.0)])
    assert np.allclose(info2, R2.T @ D2 @ R2, rtol=2e-6, atol=2e-6 * D2.max())


def test_restatement_on_the_axis_itself_is_nan_as_the_reference_is():
    info1, _, _ = nk.L32.se3_to_xyz_info([0.0, 0.0, 4.0], EYE, *_shift_x(1.0), 200.0)
    assert np.isnan(info1).all()          # k1 = (0, 0, 0) * (asin(0) / 0)


def _frames(idkf, depth=3.0):
    """cameras without rotation at x = 0.1 * idkf; feature 0 of every frame sees the world point (0.2, 0.1, depth) exactly"""
    n = len(idkf)
    K = np.array([[nc.FX, 0, nc.CX], [0, nc.FX, nc.CY], [0, 0, 1.0]])
    kps = np.zeros(n * 4, nc.KP)
    T = [_shift_x(0.1 * i) for i in idkf]
    Tcw, Twc = np.array([t[0] for t in T]), np.array([t[1] for t in T])
    P = np.array([(K @ t.reshape(3, 4).astype(np.float64)).astype(np.float32).ravel() for t in Tcw])
    for f in range(n):
        pc = np.array([0.2 - 0.1 * idkf[f], 0.1, depth])
        uv = K @ (pc / pc[2])
        kps["x"][4 * f], kps["y"][4 * f] = uv[0], uv[1]
    return nk.Frames(kps, np.full(n, 4, np.int32), 4, Tcw, Twc, P, idkf)


def _one(L, fr, frames, new, good=0, observed=None, upper=100.0):
    ptr, f, k = nc.csr([[(x, 0) for x in frames]])
    return nk.parallax_batch(L, fr, ptr, f, k, [good], [new], nc.FX, 0.3, upper, observed)


@pytest.mark.parametrize("L", [nk.L64, nk.L32])
def test_age_rule_at_differences_of_exactly_six_and_seven(L):
    # a far point never passes the parallax test: what happens to it depends on the age of pKF0 alone
    fr = _frames([0, 1, 6, 7], depth=90.0)                 # frames 0..3
    obs = np.ones(16, np.uint8)
    o = _one(L, fr, [0, 2], 2, observed=obs)               # N = 2: nothing, however old
    assert o["status"][0] == 0 and o["place"][0] == -1 and o["kf_observed"].all()
    o = _one(L, fr, [0, 1, 2], 2, observed=obs)            # N = 3, idkf 6 - 0 = 6: frame 0 is pKF0, abandoned
    assert o["status"][0] == 2 and o["place"][0] == 0
    assert o["kf_observed"].reshape(4, 4)[:3, 0].tolist() == [0, 0, 0] and o["kf_observed"].sum() == 13
    o = _one(L, fr, [0, 1, 3], 3, observed=obs)            # 7 - 0 = 7: frame 0 is out, pKF0 = frame 1 at 7 - 1 = 6: abandoned
    assert o["status"][0] == 2 and o["place"][0] == 1
    fr = _frames([0, 2, 6, 7], depth=90.0)
    o = _one(L, fr, [0, 1, 3], 3, observed=obs)            # pKF0 = frame 1 at 7 - 2 = 5: kept
    assert o["status"][0] == 3 and o["place"][0] == 1 and o["kf_observed"].all()
    assert (o["pos"] == nk.SENT).all() and (o["obs_view"] == nk.SENT).all()


@pytest.mark.parametrize("L", [nk.L64, nk.L32])
def test_promotion_by_hand(L):
    """exact projections of (0.2, 0.1, 3) from cameras at x = 0, 0.1, 0.3, 0.6: the DLT returns the point, every view is the
    point minus the camera centre, and the information of an entry is that of pKF0 turned by the identity"""
    fr = _frames([0, 1, 3, 6])
    o = _one(L, fr, [3, 0, 1, 2], 3)                       # pKF0 = frame 0 (6 - 0 = 6), second in the list
    assert o["status"][0] == 1 and o["place"][0] == 1
    assert np.allclose(o["pos"][0], [0.2, 0.1, 3.0], rtol=2e-5)
    for e, f in enumerate([3, 0, 1, 2]):
        assert np.allclose(o["obs_view"][e], [0.2 - 0.1 * fr.idkf[f], 0.1, 3.0], rtol=2e-5, atol=2e-5)
    i0, i1, _ = nk.L64.se3_to_xyz_info(o["obs_view"][1], fr.Twc[0], fr.Tcw[3], fr.Twc[3], nc.FX)
    assert np.allclose(o["obs_info"][1].reshape(3, 3), i0, rtol=1e-4, atol=1e-4 * i0.max())
    assert np.allclose(o["obs_info"][0].reshape(3, 3), i1, rtol=1e-4, atol=1e-4 * i1.max())
    assert np.allclose(o["obs_info"][2], o["obs_info"][1], rtol=1e-5) and np.allclose(o["obs_info"][3], o["obs_info"][1], rtol=1e-5)
    # cos of the parallax between the rays from x = 0 and x = 0.6
    p0, p1 = np.array([0.2, 0.1, 3.0]), np.array([-0.4, 0.1, 3.0])
    assert p0 @ p1 / np.linalg.norm(p0) / np.linalg.norm(p1) < nk.MIN_COS
    # the same list when the point is good already, and when pKF0 is pKF itself (every other frame is more than six older)
    assert _one(L, fr, [3, 0, 1, 2], 3, good=1)["status"][0] == 0
    fr7 = _frames([0, 1, 2, 9])
    o = _one(L, fr7, [0, 1, 3, 2], 3)
    assert o["status"][0] == 3 and o["place"][0] == 2 and (o["pos"] == nk.SENT).all()


def test_accept_new_observe_by_hand():
    pos, n = [0.0, 3.0, 4.0], [0.0, 0.0, 1.0]              # dist 5, cos 0.8
    for L in (nk.L64, nk.L32):
        assert not nk.accept_new_observe(L, pos, n, 2, 2, 1.0, 9.0)
        assert nk.accept_new_observe(L, pos, [0.0, 3.0, 4.0], 2, 4, 5.0, 5.0)           # cos 1, |octave| = 2, dist on both bounds
        assert not nk.accept_new_observe(L, pos, [0.0, 3.0, 4.0], 2, 5, 1.0, 9.0)
        assert not nk.accept_new_observe(L, pos, [0.0, 3.0, 4.0], 2, 2, 5.5, 9.0)
        assert not nk.accept_new_observe(L, pos, [0.0, 3.0, 4.0], 2, 2, 1.0, 4.5)
        assert nk.accept_new_observe(L, pos, [0.0, -3.0, -4.0], 0, 2, 1.0, 9.0)         # |dot|


@pytest.fixture(scope="module")
def cases():
    return nc.ParallaxCases(), nc.CorrespdCases(), nc.CorrespdCases(abandoned=True)


def test_float_restatement_against_the_fp64_layer(cases):
    pc, cc, cca = cases
    e_pos, e_mat = nc.restatement_errors(pc, [cc, cca])
    print("float32 restatement against FP64: positions %.3g, informations %.3g" % (e_pos, e_mat))
    # float32 has 2^-24 = 6e-8 per operation; a DLT at 2-8 degrees of parallax and a sine of the parallax formed from float
    # differences amplify it by 1 / angle, 10-30 here: anything beyond 1e-5 would be a mistake, not rounding
    assert e_pos < 1e-5 and e_mat < 1e-5
    assert 4 * max(e_pos, e_mat) <= nc.TOL      # the margins below are at least ten of the device's tolerances


def test_emitted_cases_keep_their_distance_from_every_threshold(cases):
    pc, cc, cca = cases
    mg = []
    out = pc.run(nk.L64, mg)
    assert out["status"].tolist() == pc.want_status
    for c in (cc, cca):
        c.run(nk.L64, 7, margins=mg)
        c.run(nk.L64, 6, margins=mg)
    if hasattr(cca, "abandoned"):
        ptr, f, k = nc.csr([cca.abandoned["entries"]])
        o = nk.parallax_batch(nk.L64, cca.sc.fr, ptr, f, k, [0], [8], nc.FX, nc.LOWER, nc.UPPER, None, mg)
        assert o["status"][0] == 2
    assert len(mg) > 300 and {n for n, _, _ in mg} == {"sinParallax", "cosParallax", "cosAngle", "dist_min", "dist_max",
                                                         "depth_lower", "depth_upper"}
    assert nk.near_threshold(mg, nc.TOL) == []
    # and the named cases are what their names say
    st = dict(zip(pc.names, out["status"]))
    assert [st[n] for n in ("promote_3", "promote_9", "already_good", "two_observations", "age_6_abandoned", "age_7_excluded",
                            "pkf0_is_pkf", "depth_gate", "out_of_range_entries")] == [1, 1, 0, 0, 2, 3, 3, 3, 1]
    pl = dict(zip(pc.names, out["place"]))
    assert pl["tie_first_wins_3"] == 0 and pl["tie_first_wins_2"] == 0 and pl["age_7_excluded"] == 1 and pl["promote_9"] == 2
    assert pl["promote_9_reversed"] == 5 and pl["out_of_range_entries"] == 1 and pl["pkf0_is_pkf"] == 2
    o7 = cc.run(nk.L64, 7)
    k0 = o7["kind"][0]
    want = dict(accept=2, octave=0, angle=0, dist_min=0, dist_max=0, depth=0, main_out_of_range=0, q_out_of_range=0)
    for name, js in cc.pass2.items():
        assert [int(k0[j]) for j in js] == [want[name]] * len(js), name
    assert o7["counts"].tolist() == [[21, 14, 3, 26, 0], [0, 21, 0, 42, 0], [0, 1, 0, 0, 0]]


def test_pass_sequence_of_the_model(cases):
    """passes 1 then 6 equal passes 7 without an abandoned point; with one, its feature goes to pass 2"""
    _, cc, cca = cases
    a = cc.run(nk.L64, 7)
    s1 = cc.run(nk.L64, 1)
    s6 = cc.run(nk.L64, 6, observed=s1["kf_observed"])
    kind = np.where(s1["kind"] > 0, s1["kind"], s6["kind"])
    assert np.array_equal(kind, a["kind"]) and np.array_equal(s6["kf_observed"], a["kf_observed"])
    s1 = cca.run(nk.L64, 1)
    ab = cca.abandoned
    assert s1["kind"][0, ab["j"]] == 1
    ptr, f, k = nc.csr([ab["entries"]])
    o = nk.parallax_batch(nk.L64, cca.sc.fr, ptr, f, k, [0], [8], nc.FX, nc.LOWER, nc.UPPER, s1["kf_observed"])
    assert o["status"][0] == 2 and o["kf_observed"][8 * nc.CAP + ab["j"]] == 0 and o["kf_observed"][6 * nc.CAP + ab["i"]] == 0
    mi = cca.match_idx_mp.copy()
    mi[0, ab["j"]] = ab["q"]
    s6 = cca.run(nk.L64, 6, observed=o["kf_observed"], match_idx_mp=mi)
    assert s6["kind"][0, ab["j"]] == 2 and s6["src"][0, ab["j"]] == ab["q"]


# ---- the header's host functions (C++) against the float32 restatement

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return nc.cpp_build(tmp_path_factory.mktemp("find_correspd"))


_bits = nc.bits


def test_host_functions_equal_the_restatement(program, tmp_path, cases):
    """calcSE3toXYZInfo and acceptNewObserve on 60 cases, updateParallax on the 48 points of the parallax batch.  Integers
    exactly; floats to 4e-6 relative: the two sides differ in asinf / sin / cos of the C library against numpy's alone."""
    pc, cc, _ = cases
    rng = np.random.default_rng(11)
    sc = pc.sc
    lines, want = [], []
    for _ in range(60):
        f1, f2 = rng.choice(nc.NFRAMES, 2, replace=False)
        xyz1 = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), rng.uniform(2, 6)], np.float32)
        normal = (xyz1 / np.linalg.norm(xyz1) + 0.3 * rng.standard_normal(3)).astype(np.float32)
        octs = rng.integers(0, 8, 2)
        d = float(np.linalg.norm(xyz1))
        mind, maxd = np.float32(d * rng.uniform(0.5, 1.1)), np.float32(d * rng.uniform(0.9, 2.0))
        lines.append("I " + " ".join(map(str, _bits(xyz1) + _bits(sc.fr.Twc[f1]) + _bits(sc.fr.Tcw[f2]) + _bits(sc.fr.Twc[f2]) +
                                         _bits([nc.FX]) + _bits(normal) + octs.tolist() + _bits([mind, maxd]))))
        i1, i2, x2 = nk.L32.se3_to_xyz_info(xyz1, sc.fr.Twc[f1], sc.fr.Tcw[f2], sc.fr.Twc[f2], nc.FX)
        want.append((np.concatenate([i1.ravel(), i2.ravel(), x2]), int(nk.accept_new_observe(nk.L32, xyz1, normal, octs[0], octs[1], mind, maxd))))
    rows, mirror = nc.cpp_run_parallax(program, tmp_path / "cases.txt", sc.fr, pc.ptr, pc.obs_frame, pc.obs_ftr, pc.good, pc.new,
                                    pc.observed, lines=lines)
    assert len(rows) == 60
    for ln, (w, acc) in zip(rows, want):
        v = ln.split()
        got = np.array([int(x) for x in v[:21]], np.uint32).view(np.float32)
        assert int(v[21]) == acc
        assert nk.rel_err_mat(got[:9], w[:9])[0] < 4e-6 and nk.rel_err_mat(got[9:18], w[9:18])[0] < 4e-6
        assert np.array_equal(got[18:].view(np.uint32), w[18:].astype(np.float32).view(np.uint32))
    ref = pc.run(nk.L32)
    assert (ref["status"] == 1).sum() >= 10
    nc.same_parallax(mirror, ref)
