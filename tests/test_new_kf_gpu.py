"""se2gpu_mappoint_parallax_batch_device and se2gpu_kf_correspd_batch_device on the GPU against the numpy model
(tests/new_kf_model.py, cases of tests/new_kf_cases.py: cap 64, nine frames, 48 points, three jobs).

Integer outputs (kind, src, inv, status, the place of pKF0, the counts, the hasObservation bytes) equal the model EXACTLY.
Positions and informations are compared with the model's FP64 layer.  The yardstick is the float32 restatement's own error
against that layer on the same cases, measured on the CPU in this run - relative per 3x3 matrix against its largest entry,
per position against its norm; measured: 1.1e-6 for positions, 2.3e-6 for informations - and the device gets FOUR times the
worst of the two (about 9e-6): the margin covers another asinf / sin / cos and another legal order of the double sums.  No
case is left out of a comparison: the generator keeps every gated quantity ten tolerances away from its threshold
(test_new_kf_model.py asserts it), so the integer outputs cannot depend on rounding."""
import numpy as np
import pytest

import new_kf_cases as nc
import new_kf_model as nk

pytestmark = pytest.mark.gpu
INTS = ("inv", "kind", "src", "counts")


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


@pytest.fixture(scope="module")
def cases():
    return nc.ParallaxCases(), nc.CorrespdCases(), nc.CorrespdCases(abandoned=True)


@pytest.fixture(scope="module")
def bound(cases):
    pc, cc, cca = cases
    e_pos, e_mat = nc.restatement_errors(pc, [cc, cca])
    b = 4 * max(e_pos, e_mat)
    print("restatement: positions %.3g, informations %.3g; device bound %.3g" % (e_pos, e_mat, b))
    assert b <= nc.TOL
    return b


def _poses(sc, observed=None, view_pos=None):
    from se2lam_amd import newkf
    fr = sc.fr
    return newkf.DevicePoses(fr.kps, fr.counts, fr.cap, fr.Tcw, fr.Twc, fr.P, fr.idkf, observed, view_pos)


def _close_pos(got, want, w, bound, what):
    assert np.array_equal(got.reshape(-1, 3)[:, 0] != np.float32(nk.SENT), w.ravel()), what
    if w.any():
        e = nk.rel_err_pos(got[w], want[w]).max()
        print(what, "positions", e)
        assert e <= bound, (what, e)


def _close_mat(got, want, w, bound, what):
    assert np.array_equal(got.reshape(-1, 9)[:, 0] != np.float32(nk.SENT), w.ravel()), what
    if w.any():
        e = nk.rel_err_mat(got[w], want[w]).max()
        print(what, "informations", e)
        assert e <= bound, (what, e)


def _parallax_device(matcher, pc, sel=None, clear=True):
    from se2lam_amd import newkf
    sel = range(len(pc.lists)) if sel is None else sel
    ptr, f, k = nc.csr([pc.lists[p] for p in sel])
    poses = _poses(pc.sc, pc.observed)
    out = newkf.promote_batch_device(matcher, poses, ptr, f, k, pc.good[list(sel)], pc.new[list(sel)], nc.FX, nc.LOWER, nc.UPPER, clear)
    out["kf_observed"] = poses.observed()
    return out


@pytest.fixture(scope="module")
def parallax(cases, matcher):
    pc = cases[0]
    return pc, pc.run(nk.L64), _parallax_device(matcher, pc)


def test_parallax_batch_equals_the_model(parallax, bound):
    """the age boundary at 6 and 7, a tie of idkf, entries out of range, a point that is good already, promotion with 3 and
    with 9 observations and its propagation, abandoned points and their bytes, the depth gate, pKF0 == pKF"""
    pc, want, got = parallax
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["place"], want["place"])
    assert want["status"].tolist() == pc.want_status and set(want["status"]) == {0, 1, 2, 3}
    assert np.array_equal(got["kf_observed"], want["kf_observed"]) and (want["kf_observed"] != pc.observed).sum() >= 6
    w = want["status"] == 1
    _close_pos(got["pos"], want["pos"], w, bound, "mPos")
    w = want["obs_view"][:, 0] != nk.SENT
    p9 = pc.index("promote_9")
    assert w[pc.ptr[p9]:pc.ptr[p9 + 1]].sum() == 8                   # frames 2 and 3 tie: one of them is pKF0, the other is skipped
    p3 = pc.index("promote_3")
    assert w[pc.ptr[p3]:pc.ptr[p3 + 1]].all()
    _close_pos(got["obs_view"], want["obs_view"], w, bound, "mViewMPs")
    _close_mat(got["obs_info"], want["obs_info"], w, bound, "mViewMPsInfo")


def test_parallax_without_the_flags_leaves_them(cases, matcher, parallax):
    pc, _, first = parallax
    got = _parallax_device(matcher, pc, clear=False)
    assert np.array_equal(got["kf_observed"], pc.observed)
    for k in ("status", "place"):
        assert np.array_equal(got[k], first[k])


def test_parallax_is_independent_of_batch_position_and_run(cases, matcher, parallax):
    pc, _, first = parallax
    again = _parallax_device(matcher, pc)
    for k in first:
        assert np.array_equal(again[k].view(np.uint8), first[k].view(np.uint8)), k           # two runs, bit for bit
    sel = list(range(len(pc.lists)))[::-1][:20]
    got = _parallax_device(matcher, pc, sel)
    off = 0
    for n, p in enumerate(sel):
        assert got["status"][n] == first["status"][p] and got["place"][n] == first["place"][p]
        assert np.array_equal(got["pos"][n].view(np.uint32), first["pos"][p].view(np.uint32))
        s, e = pc.ptr[p], pc.ptr[p + 1]
        for k in ("obs_view", "obs_info"):
            assert np.array_equal(got[k][off:off + e - s].view(np.uint32), first[k][s:e].view(np.uint32)), (k, p)
        off += e - s


def _correspd_device(matcher, cc, passes, observed=None, match_idx_mp="own", jobs=None, poses=None):
    from se2lam_amd import newkf
    sel = list(range(len(cc.JOBS))) if jobs is None else list(jobs)
    mi = cc.match_idx_mp if isinstance(match_idx_mp, str) else match_idx_mp
    poses = poses or _poses(cc.sc, cc.observed if observed is None else observed, cc.view_pos)
    out = newkf.observe_batch_device(matcher, poses, cc.job_prev[sel], cc.job_new[sel], cc.Tcr[sel], cc.Trc[sel], cc.matched12[sel],
                                     cc.local_pos[sel], None if mi is None else mi[sel], cc.mp, nc.FX, nc.LOWER, nc.UPPER, passes)
    out["kf_observed"] = poses.observed()
    return out


def _same_correspd(got, want, bound, what):
    for k in INTS + ("kf_observed",):
        assert np.array_equal(got[k], want[k]), (what, k)
    w, w3 = want["kind"] > 0, want["kind"] == 3
    _close_pos(got["view"], want["view"], w, bound, what + " view")
    _close_mat(got["info"], want["info"], w, bound, what + " info")
    _close_pos(got["new_pos_w"], want["new_pos_w"], w3, bound, what + " posW")
    _close_mat(got["info_prev"], want["info_prev"], w3, bound, what + " info of prev")


@pytest.fixture(scope="module")
def all_passes(cases, matcher):
    cc = cases[1]
    return cc, cc.run(nk.L64, 7), _correspd_device(matcher, cc, 7)


def test_three_passes_equal_the_model(all_passes, bound):
    """jobs whose new key frames hold 64, 63 and 1 features; in job 0 each condition of acceptNewObserve and the depth gate
    fails alone, a map point without a valid main observation and a match beyond the table are passed over"""
    cc, want, got = all_passes
    assert want["counts"].tolist() == [[21, 14, 3, 26, 0], [0, 21, 0, 42, 0], [0, 1, 0, 0, 0]]
    for name, js in cc.pass2.items():
        assert [int(want["kind"][0, j]) for j in js] == [2 if name == "accept" else 0] * len(js), name
    _same_correspd(got, want, bound, "passes 7")


def test_duplicated_match_is_counted(cases, matcher, bound):
    cc = cases[1]
    m12 = cc.matched12.copy()
    i_lo, i_hi = 1, 2                                   # two new-point features of the previous key frame claim one j
    m12[0, i_lo] = m12[0, i_hi]
    keep, cc.matched12 = cc.matched12, m12
    try:
        want, got = cc.run(nk.L64, 7), _correspd_device(matcher, cc, 7)
    finally:
        cc.matched12 = keep
    assert want["counts"][0, 4] == 1 and want["inv"][0, m12[0, i_hi]] == i_hi
    _same_correspd(got, want, bound, "duplicate")


def test_correspd_is_independent_of_batch_position_and_run(cases, matcher, all_passes):
    cc, _, first = all_passes
    again = _correspd_device(matcher, cc, 7)
    for k in first:
        assert np.array_equal(again[k].view(np.uint8), first[k].view(np.uint8)), k
    got = _correspd_device(matcher, cc, 7, jobs=[2, 0])
    for n, b in enumerate([2, 0]):
        for k in INTS + ("view", "info", "new_pos_w", "info_prev"):
            assert np.array_equal(got[k][n].view(np.uint8), first[k][b].view(np.uint8)), (k, b)


def _tracked_lists(cc, kind, src, extra=None):
    """the observation lists of the tracked points after pass 1: (prev, i), (new, j), and what `extra` adds for (b, j)"""
    lists, new = [], []
    for b in range(len(cc.JOBS)):
        for j in np.flatnonzero(kind[b] == 1):
            l = [(int(cc.job_prev[b]), int(src[b, j])), (int(cc.job_new[b]), int(j))]
            lists.append((extra or {}).get((b, int(j)), []) + l)
            new.append(int(cc.job_new[b]))
    return lists, new


def _sequence(matcher, cc, match_idx_mp, extra=None):
    """passes = 1, the parallax update of the tracked points, passes = 6, on one set of device tables"""
    from se2lam_amd import newkf
    poses = _poses(cc.sc, cc.observed, cc.view_pos)
    s1 = _correspd_device(matcher, cc, 1, poses=poses)
    lists, new = _tracked_lists(cc, s1["kind"], s1["src"], extra)
    ptr, f, k = nc.csr(lists)
    prl = newkf.promote_batch_device(matcher, poses, ptr, f, k, np.zeros(len(lists), np.uint8), new, nc.FX, nc.LOWER, nc.UPPER)
    s6 = _correspd_device(matcher, cc, 6, match_idx_mp=match_idx_mp, poses=poses)
    return s1, prl, s6, lists


def test_pass_sequence_equals_one_call_without_an_abandoned_point(cases, matcher, all_passes):
    cc, _, one = all_passes
    s1, prl, s6, _ = _sequence(matcher, cc, cc.match_idx_mp)
    assert (prl["status"] == 0).all()                                   # two observations each: nothing to do
    assert (s6["kind"][s1["kind"] > 0] == 0).all()
    took1 = s1["kind"] > 0
    for k in ("kind", "src"):
        assert np.array_equal(np.where(took1, s1[k], s6[k]), one[k]), k
    for k in ("view", "info"):
        merged = np.where(took1[..., None], s1[k], s6[k])
        assert np.array_equal(merged.view(np.uint32), one[k].view(np.uint32)), k
    for k in ("new_pos_w", "info_prev", "kf_observed", "inv"):
        assert np.array_equal(s6[k].view(np.uint8), one[k].view(np.uint8)), k
    assert np.array_equal(s1["counts"][:, 1:4] + s6["counts"][:, 1:4], one["counts"][:, 1:4])


def test_pass_sequence_with_an_abandoned_point_frees_its_feature(cases, matcher, bound):
    cca = cases[2]
    ab = cca.abandoned
    mi = cca.match_idx_mp.copy()
    mi[0, ab["j"]] = ab["q"]
    s1, prl, s6, lists = _sequence(matcher, cca, mi, extra={(0, ab["j"]): [ab["entries"][0]]})
    assert s1["kind"][0, ab["j"]] == 1 and s1["src"][0, ab["j"]] == ab["i"]
    at = lists.index(ab["entries"])
    assert prl["status"][at] == 2 and prl["place"][at] == 0 and (np.delete(prl["status"], at) == 0).all()
    assert s6["kind"][0, ab["j"]] == 2 and s6["src"][0, ab["j"]] == ab["q"]
    # the model, the same three steps
    m1 = cca.run(nk.L64, 1)
    ptr, f, k = nc.csr(lists)
    mp = nk.parallax_batch(nk.L64, cca.sc.fr, ptr, f, k, np.zeros(len(lists), np.uint8), [l[-1][0] for l in lists], nc.FX,
                           nc.LOWER, nc.UPPER, m1["kf_observed"])
    m6 = cca.run(nk.L64, 6, observed=mp["kf_observed"], match_idx_mp=mi)
    _same_correspd(s1, m1, bound, "passes 1")
    assert np.array_equal(prl["status"], mp["status"])
    _same_correspd(s6, m6, bound, "passes 6")
    # in one call the feature stays with the tracked point
    assert cca.run(nk.L64, 7, match_idx_mp=mi)["kind"][0, ab["j"]] == 1


def test_the_shared_observation_table(matcher, bound):
    """the irregular table of tests/obs_table_cases.py, which the main-key-frame and covisibility calls are fed too: planted
    entries out of range, descending and overlapping d_mp_ptr segments (all inside 0..nobs; no entry has two writers)"""
    import obs_table_cases as oc
    from se2lam_amd import newkf
    t = oc.table()
    want = t.parallax_model(nk.L64)
    t.check_one_writer(want["status"])
    assert set(want["status"]) == {0, 1, 2, 3} and want["status"][9] != 0 and want["status"][25] != 0 and 60 <= t.nobs <= 160
    fr = t.sc.fr
    poses = newkf.DevicePoses(fr.kps, fr.counts, fr.cap, fr.Tcw, fr.Twc, fr.P, fr.idkf, t.observed)
    got = newkf.promote_batch_device(matcher, poses, t.ptr, t.obs_frame, t.obs_ftr, t.good, t.new, nc.FX, nc.LOWER, nc.UPPER)
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["place"], want["place"])
    assert np.array_equal(poses.observed(), want["kf_observed"]) and (want["kf_observed"] != t.observed).any()
    _close_pos(got["pos"], want["pos"], want["status"] == 1, bound, "shared table mPos")
    w = want["obs_view"][:, 0] != nk.SENT
    _close_pos(got["obs_view"], want["obs_view"], w, bound, "shared table mViewMPs")
    _close_mat(got["obs_info"], want["obs_info"], w, bound, "shared table mViewMPsInfo")
