"""se2gpu_feat_edge_batch_device (csrc/feat_edge_device.hip in front of k_feat_edge and k_sparsify) on the GPU.

Gather: the rows read out of d_ws through se2gpu_feat_edge_ws_layout against tests/feat_edge_gather_model.py, to the bit, on
both routes, with invalid entries planted on both sides of a 64-entry boundary, slots outside 0..nframes-1 and indices >= m.
Prior: the information matrix against the host function to the bit, the measurement within 1e-12 * max(1, |t|_inf).
Result: against the host route se2gpu_feat_edge_batch fed the numpy gather of the same tables, and against
tests/feat_edge_model.py directly, with the tolerances tests/test_feat_edge_gpu.py states: chi2 at the start rel 1e-11, LM
histories rtol 1e-5 with equal trial counts over feat_edge_model.compared_prefix, poses and points within 1e-5 of the largest
update, edge chi2 rtol 1e-4 / atol 1e-7, the outlier mask exact (every case keeps its edge chi2 more than 1e-3 relative from 5.0,
asserted on the model by feat_edge_model.check_against_model).
Independence of run, batch and position; neighbours below the minimum (status 1) and with a NaN (status 2).
Chain: build -> pairs -> feat edge with one wait against the three calls with a wait and a host gather in between.
A match call on verify-style rows queued behind another call, one wait for both.  The optional outputs NULL.
Every table, model and device batch is computed once for the module."""
import numpy as np
import pytest

import covis_cases as cc
import feat_edge_cases as fc
import feat_edge_device_cases as dc
import feat_edge_gather_model as gm
import feat_edge_model as fm

pytestmark = pytest.mark.gpu
REL = fm.REL

# points per pair: none, below both minima, either side of the covisibility minimum, the lane boundary, two strides and a tail
SHAPES = ((0, 0), (2, 0), (9, 0), (10, 0), (63, 0), (64, 1), (65, 0), (129, 0))
W129, W65, W64, W63, W10, W9, W2, W0 = 7, 6, 5, 4, 3, 2, 1, 0
OUTLIERS = {W64: 5}          # match mode: planted outliers; seed 1 is one at which the model rejects all five
# invalid entries of the 129-point pair: inside the first chunk, its last lane, the first lane of the next, inside it, the last
BAD_ENTRIES = (5, 63, 64, 100, 128)
KEEP129 = np.array([j for j in range(129) if j not in BAD_ENTRIES])


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


@pytest.fixture(scope="module")
def tab():
    return dc.Tables(SHAPES, OUTLIERS)


def _covis_plant(tab, p):
    """the five kinds of invalid entry, at BAD_ENTRIES of pair p (a 129-point pair)"""
    return [(p, 5, 0, tab.m), (p, 63, 1, -1), (p, 64, 2, tab.nobs), (p, 100, 0, -1), (p, 128, 1, tab.nobs + 7)]


def _match_plant(tab, p, w=W129):
    """feature of key frame 0 -> no match, a value past counts[b], and (through the tables, see the mtab fixture) no map point
    on either side and a point index >= m: the same five points as BAD_ENTRIES"""
    f = tab.ftr_of(w, 0)
    return [(p, int(f[5]), -1), (p, int(f[63]), dc.CAP)]


@pytest.fixture(scope="module")
def mtab(tab):
    """the match tables with the map points of three features of world W129 removed / out of range"""
    import copy
    t = copy.copy(tab)
    t.ftr_mp = tab.ftr_mp.copy()
    t.ftr_mp[2 * W129, tab.ftr_of(W129, 0)[64]] = -1
    t.ftr_mp[2 * W129 + 1, tab.ftr_of(W129, 1)[100]] = -1
    t.ftr_mp[2 * W129, tab.ftr_of(W129, 0)[128]] = tab.m
    return t


def _batch_worlds(npairs):
    if npairs == 1:
        return [W129]
    if npairs == 3:
        return [W129, W10, W0]
    return [(W129, W65, W64, W63, W10, W9, W2, W0)[p % 8] for p in range(npairs)]


def _run_covis(matcher, tab, worlds, row_cap, list_cap, plant=(), bad_slots=(), refused=(), **kw):
    """bad_slots: (pair, a, b) replacements; refused: pairs whose record is what the pairs call writes for such slots"""
    from se2lam_amd import feat_edge as fe
    pair_a, pair_b, pair_out, common = tab.covis_inputs(worlds, list_cap, plant)
    for p, a, b in bad_slots:
        pair_a[p], pair_b[p] = a, b
    for p in refused:
        pair_out[p] = (-1, 0, 0, 0)
    buf = fe.CreateFeatEdgeCovisBatchDevice(matcher, pair_a, pair_b, tab.Twc, tab.pos, pair_out, common, list_cap, tab.obs_view,
                                            tab.obs_info, row_cap, **kw)
    g = gm.gather_covis(pair_a, pair_b, tab.nframes, tab.Twc, tab.pos, row_cap, pair_out, common, list_cap, tab.obs_view, tab.obs_info)
    return buf, g


def _run_match(matcher, tab, worlds, row_cap, plant=(), bad_slots=(), **kw):
    from se2lam_amd import feat_edge as fe
    pair_a, pair_b, matches = tab.match_inputs(worlds, plant)
    for p, a, b in bad_slots:
        pair_a[p], pair_b[p] = a, b
    buf = fe.CreateFeatEdgeMatchBatchDevice(matcher, pair_a, pair_b, tab.Twc, tab.pos, matches, tab.counts, dc.CAP, tab.ftr_mp,
                                            tab.view_pos, tab.view_info, row_cap, **kw)
    g = gm.gather_match(pair_a, pair_b, tab.nframes, tab.Twc, tab.pos, row_cap, matches, tab.counts, dc.CAP, tab.ftr_mp, tab.view_pos,
                        tab.view_info)
    return buf, g


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_gather(buf, g, label):
    """the rows in d_ws, d_info8 and the untouched tails of the per-point outputs against the numpy gather"""
    from se2lam_amd import capi
    got, res = buf.read_gather(), buf.read()
    print("%s: counts %s raw %s dropped %s cut %s" % (label, got["count"].tolist()[:8], got["raw"].tolist()[:8],
                                                    got["dropped"].tolist()[:8], got["cut"].tolist()[:8]))
    for k in ("count", "raw", "dropped", "cut"):
        assert np.array_equal(got[k], g[k]), k
    assert np.array_equal(_bits(got["kf12"]), _bits(g["kf12"]))
    for p, r in enumerate(res):
        c = int(g["count"][p])
        for k in ("xyz", "z", "info"):
            assert np.array_equal(_bits(got[k][p, :c]), _bits(g[k][p])), (p, k)
        assert (r["n_points"], r["raw"], r["dropped"], r["cut"], int(r["info8"][7])) == (c, g["raw"][p], g["dropped"][p], g["cut"][p], 0)
        assert np.all(r["mp_row"][c:] == capi.SENT) and np.all(r["edge_chi2_row"][c:] == capi.SENT), p
        assert np.all(r["outlier_row"][c:] == capi.SENTINEL_DESC), p
    return got, res


GRID = [(n, r, l) for n in (1, 3, 70) for r, l in ((3, 70), (64, 70), (65, 200), (130, 70), (130, 200))]


@pytest.mark.parametrize("npairs,row_cap,list_cap", GRID)
def test_covis_gather_equals_the_numpy_gather_to_the_bit(matcher, tab, npairs, row_cap, list_cap):
    """list_cap 70 lies below n_same = 129 and above the rest, 200 above all; row_cap 3 cuts every pair that has points"""
    worlds = _batch_worlds(npairs)
    bad = [(10, -1, 3), (11, 2, tab.nframes), (12, 1 << 30, 0)] if npairs == 70 else []
    buf, g = _run_covis(matcher, tab, worlds, row_cap, list_cap, plant=_covis_plant(tab, 0) if list_cap > 128 else _covis_plant(tab, 0)[:3],
                        bad_slots=bad, refused=[p for p, _, _ in bad[:2]], iters=2)
    got, res = _check_gather(buf, g, "covis %d pairs row_cap %d list_cap %d" % (npairs, row_cap, list_cap))
    if row_cap == 130 and list_cap == 200:
        assert g["count"][0] == 124 and g["dropped"][0] == 5 and g["cut"][0] == 0      # the prefix crossed both chunk boundaries
    if row_cap == 130 and list_cap == 70:
        assert g["count"][0] == 67 and g["dropped"][0] == 3 and g["cut"][0] == 1
    for i, (p, _, _) in enumerate(bad):      # the third keeps its n_same: no points, but not below the minimum
        assert g["count"][p] == 0 and res[p]["n_points"] == 0 and res[p]["status"] == (1 if i < 2 else 0)
        assert res[p]["z12"].any() == (i == 2)


@pytest.mark.parametrize("npairs,row_cap", [(n, r) for n in (1, 3, 70) for r in (3, 64, 65, 130)])
def test_match_gather_equals_the_numpy_gather_to_the_bit(matcher, mtab, npairs, row_cap):
    worlds = _batch_worlds(npairs)
    bad = [(10, -1, 3), (11, 2, mtab.nframes)] if npairs == 70 else []
    buf, g = _run_match(matcher, mtab, worlds, row_cap, plant=_match_plant(mtab, 0), bad_slots=bad, iters=2)
    _check_gather(buf, g, "match %d pairs row_cap %d" % (npairs, row_cap))
    if row_cap == 130:
        assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (124, 127, 3, 0)
    if row_cap == 64:
        assert (g["count"][0], g["raw"][0], g["dropped"][0], g["cut"][0]) == (64, 127, 3, 1)
    for p, _, _ in bad:
        assert (g["count"][p], g["raw"][p]) == (0, 0)


def test_prior_information_to_the_bit_and_measurement_within_the_bound(matcher, tab):
    """the poses of a 70-pair batch (the identity of a bad slot among them): info36 is the same arithmetic with no library
    function; meas12 goes through atan2 / cos / sin, a few ulp apart between glibc and the device library"""
    from se2lam_amd import capi, feat_edge as fe
    buf, g = _run_covis(matcher, tab, _batch_worlds(70), 8, 8, bad_slots=[(10, -1, 3)], iters=1)
    got = buf.read_gather()
    kf = np.ascontiguousarray(g["kf12"].reshape(-1, 12))
    tbc = fe.Tbc12()
    meas, info = np.zeros((len(kf), 12)), np.zeros((len(kf), 36))
    for i in range(len(kf)):
        capi.check(capi.lib().se2gpu_plane_motion_prior_iso3(kf[i].ctypes.data, tbc.ctypes.data, 1e6, 1e6, 1.0, meas[i].ctypes.data,
                                                             info[i].ctypes.data))
    assert np.array_equal(_bits(got["prior_info"].reshape(-1, 36)), _bits(info))
    diff = np.abs(got["prior_meas"].reshape(-1, 12) - meas).max(axis=1)
    bound = 1e-12 * np.maximum(1.0, np.abs(kf[:, 9:]).max(axis=1))
    print("plane-motion prior: largest |meas12 - host| = %.3g (largest |t|_inf %.4g, bound %.3g there); largest ratio to the bound %.3g"
          % (diff.max(), np.abs(kf[:, 9:]).max(), bound[np.argmax(diff)], (diff / bound).max()))
    assert np.all(diff <= bound)
    # roll and pitch are removed: a formula that kept them would be 1e-3 and more away
    assert np.abs(meas - kf).max() > 1e-3


# ---- results

def _host_route(g, mode, **kw):
    """se2gpu_feat_edge_batch on the numpy gather, with a min_points that lets every pair through"""
    from se2lam_amd import capi, feat_edge as fe
    kf, mp_ptr, mp, z, info = gm.host_call_arrays(g)
    n = len(g["count"])
    iters = kw.pop("iters", fe.COVIS_ITERS if mode == fe.COVIS else fe.MATCH_ITERS)
    rc, o = fe.feat_edge_raw(n, mode, iters, 0, kf, mp_ptr, mp, z, info, **kw)
    capi.check(rc)
    return [fe._pair_dict(o["info4"][p, 0], o["info4"][p, 1], o["info4"][p, 2], o["info4"][p, 3], o["kf"][p], o["mp"][mp_ptr[p]:mp_ptr[p + 1]],
                          o["outlier"][mp_ptr[p]:mp_ptr[p + 1]], o["edge_chi2"][mp_ptr[p]:mp_ptr[p + 1]], o["stats"][p], o["z"][p], o["info"][p])
            for p in range(n)], (kf, mp)


def _close_to_host(dev, host, kf_in, mp_in, label):
    """the two routes run the same kernel on the same rows; only the prior's measurement differs by a few ulp.  The tolerances
    of tests/test_feat_edge_gpu.py, with the host route in the model's place."""
    sd, sh = dev["stats"], host["stats"]
    assert dev["status"] == host["status"] and dev["n_points"] == host["n_points"]
    assert np.isclose(sd["chi2_init"], sh["chi2_init"], rtol=1e-11, atol=0)
    n = fm.compared_prefix(sh["chi2_init"], sh["chi2_hist"])
    assert sd["iterations"] >= n
    assert np.allclose(sd["chi2_hist"][:n], sh["chi2_hist"][:n], rtol=REL, atol=0)
    assert np.allclose(sd["lambda_hist"][:n], sh["lambda_hist"][:n], rtol=REL, atol=0)
    assert np.array_equal(sd["trials_hist"][:n], sh["trials_hist"][:n])
    update = max(np.abs(host["kf12"] - kf_in).max(), np.abs(host["mp"] - mp_in).max() if len(mp_in) else 0.0)
    off = max(np.abs(dev["kf12"] - host["kf12"]).max(), np.abs(dev["mp"] - host["mp"]).max() if len(mp_in) else 0.0)
    print("%s: device route off the host route by %.3g, largest update %.3g, compared prefix %d" % (label, off, update, n))
    assert off <= REL * update
    assert np.allclose(dev["edge_chi2"], host["edge_chi2"], rtol=1e-4, atol=1e-7)
    assert np.array_equal(dev["outlier"], host["outlier"])
    assert dev["n_outliers"] == host["n_outliers"] and dev["n_sparsified"] == host["n_sparsified"]


COVIS8 = [W129, W65, W64, W63, W10, W9, W2, W0, W129]       # the last one with the invalid entries planted
MATCH8 = [W129, W65, W64, W63, W10, W9, W2, W0, W129]


@pytest.fixture(scope="module")
def covis_result(matcher, tab):
    buf, g = _run_covis(matcher, tab, COVIS8, 130, 130, plant=_covis_plant(tab, 8))
    host, (kf, mp) = _host_route(g, fm.COVIS)
    return dict(dev=buf.read(), gather=g, host=host, kf=kf, mp=mp, models={})


@pytest.fixture(scope="module")
def match_result(matcher, mtab):
    buf, g = _run_match(matcher, mtab, MATCH8, 130, plant=_match_plant(mtab, 8))
    # the planted tables hold for every pair of world W129: pair 0 has 127 points (the two match plants are pair 8's alone)
    host, (kf, mp) = _host_route(g, fm.MATCH)
    return dict(dev=buf.read(), gather=g, host=host, kf=kf, mp=mp, models={})


def _model(res, tab, w, keep, mode):
    key = (w, None if keep is None else tuple(keep))
    if key not in res["models"]:
        c = tab.case(w, keep)
        res["models"][key] = (c, fm.optimize(fm.Problem(c["kf"], c["mp"], c["z"], c["info"], mode), 15 if mode == fm.COVIS else 30))
    return res["models"][key]


MATCH_KEEP0 = np.array([j for j in range(129) if j not in (64, 100, 128)])


@pytest.mark.parametrize("slot", [0, 1, 2, 3, 4, 8])
def test_covis_route_against_the_model_and_the_host_route(covis_result, tab, oracle, slot):
    r, w = covis_result, COVIS8[slot]
    c, m = _model(r, tab, w, KEEP129 if slot == 8 else None, fm.COVIS)
    label = "covis slot %d (%d points)" % (slot, len(c["mp"]))
    fm.check_against_model(r["dev"][slot], c, m, fm.COVIS, oracle, label)
    assert not r["dev"][slot]["outlier"].any()
    a, b = int(np.sum(r["gather"]["count"][:slot])), int(np.sum(r["gather"]["count"][:slot + 1]))
    _close_to_host(r["dev"][slot], r["host"][slot], r["kf"][slot], r["mp"][a:b], label)


@pytest.mark.parametrize("slot", [0, 1, 2, 3, 4, 5, 8])
def test_match_route_against_the_model_and_the_host_route(match_result, mtab, oracle, slot):
    r, w = match_result, MATCH8[slot]
    keep = MATCH_KEEP0 if slot == 0 else KEEP129 if slot == 8 else None
    c, m = _model(r, mtab, w, keep, fm.MATCH)
    label = "match slot %d (%d points)" % (slot, len(c["mp"]))
    fm.check_against_model(r["dev"][slot], c, m, fm.MATCH, oracle, label)
    if w == W64:
        assert c["planted"].sum() == 5 and np.all(m["outlier"][c["planted"]])        # the condition on the inputs, on the model
        assert np.all(r["dev"][slot]["outlier"][c["planted"]])
    a, b = int(np.sum(r["gather"]["count"][:slot])), int(np.sum(r["gather"]["count"][:slot + 1]))
    _close_to_host(r["dev"][slot], r["host"][slot], r["kf"][slot], r["mp"][a:b], label)


def test_pairs_below_the_minimum_are_not_run(covis_result, match_result):
    """status 1: nothing is run, kf12_out is the input pose, the constraint is zero - on the RAW count"""
    for r, slots in ((covis_result, (5, 6, 7)), (match_result, (6, 7))):
        for s in slots:
            d, g = r["dev"][s], r["gather"]
            assert d["status"] == 1 and d["n_points"] == g["count"][s] == d["raw"] and d["n_outliers"] == 0 and d["n_sparsified"] == 0
            assert np.array_equal(_bits(d["kf12"]), _bits(g["kf12"][s]))
            assert np.array_equal(_bits(d["mp"]), _bits(g["xyz"][s]))
            assert not d["z12"].any() and not d["info"].any() and not d["outlier"].any() and not d["edge_chi2"].any()
            st = d["stats"]
            assert st["iterations"] == 0 and st["trials"] == 0 and st["chi2_init"] == 0 and st["chi2_final"] == 0


def test_the_minimum_is_tested_on_the_raw_count(matcher, mtab):
    """five raw matches of which two have both map points: status 0 on two points, as the host route with those rows"""
    f0, f1 = mtab.ftr_of(W10, 0), mtab.ftr_of(W10, 1)
    t = __import__("copy").copy(mtab)
    t.ftr_mp = mtab.ftr_mp.copy()
    t.ftr_mp[2 * W10, f0[2:5]] = -1
    plant = [(0, int(f0[j]), -1) for j in range(5, 10)]
    buf, g = _run_match(matcher, t, [W10], 16, plant=plant)
    d = buf.read()[0]
    assert (g["count"][0], g["raw"][0], g["dropped"][0]) == (2, 5, 3)
    assert d["status"] == 0 and d["n_points"] == 2 and d["raw"] == 5 and d["dropped"] == 3
    host, (kf, mp) = _host_route(g, fm.MATCH)
    _close_to_host(d, host[0], kf[0], mp, "two points of five raw matches")
    # and an empty gather above the minimum is the sparsifier's answer for no points, as the host route gives it
    buf, g = _run_match(matcher, t, [W10], 16, plant=plant, min_points=0, bad_slots=[(0, -1, 0)])
    d = buf.read()[0]
    host, _ = _host_route(g, fm.MATCH)
    assert d["status"] == 0 == host[0]["status"] and d["n_points"] == 0 and d["n_sparsified"] == 0 and d["z12"].any()
    _close_to_host(d, host[0], gm.host_call_arrays(g)[0][0], np.zeros((0, 3)), "no points above the minimum")


# ---- independence

WORDS = ("status", "n_points", "n_outliers", "n_sparsified", "kf12", "mp", "outlier", "edge_chi2", "z12", "info", "info8")


def _same(a, b):
    for k in WORDS:
        assert np.array_equal(a[k], b[k]), k
    for k, v in a["stats"].items():
        assert np.array_equal(v, b["stats"][k]), k


def test_a_pair_does_not_depend_on_run_batch_or_position(matcher, tab):
    worlds = _batch_worlds(70)
    worlds[69] = W65
    one = _run_covis(matcher, tab, [W65], 130, 130)[0].read()
    b70 = _run_covis(matcher, tab, worlds, 130, 130)[0]
    first, g1 = b70.read(), b70.read_gather()
    again = _run_covis(matcher, tab, worlds, 130, 130, buf=b70)[0]       # the same buffers, work space included
    second, g2 = again.read(), again.read_gather()
    assert first[69]["status"] == 0
    _same(one[0], first[69])
    for a, b in zip(first, second):
        _same(a, b)
    for k in g1:
        assert np.array_equal(_bits(g1[k]) if g1[k].dtype == np.float64 else g1[k], _bits(g2[k]) if g2[k].dtype == np.float64 else g2[k]), k


def test_neighbours_below_the_minimum_or_with_a_nan_disturb_nobody(matcher, tab):
    alone = _run_covis(matcher, tab, [W65, W63], 80, 80)[0].read()
    quiet = _run_covis(matcher, tab, [W65, W9, W63], 80, 80)[0].read()
    assert quiet[1]["status"] == 1 and not quiet[1]["z12"].any() and not quiet[1]["info"].any()
    assert np.array_equal(quiet[1]["kf12"].ravel(), gm.kf12_of_slot(tab.Twc, 2 * W9, tab.nframes).tolist() + gm.kf12_of_slot(tab.Twc, 2 * W9 + 1, tab.nframes).tolist())
    _same(alone[0], quiet[0])
    _same(alone[1], quiet[2])
    t = __import__("copy").copy(tab)
    t.obs_info = tab.obs_info.copy()
    t.obs_info[2 * (tab.off[W10] + 4) + 1, 4] = np.nan           # one entry of key frame 1's information of point 4
    nan = _run_covis(matcher, t, [W65, W10, W63], 80, 80)[0].read()
    assert nan[1]["status"] == 2 and nan[1]["n_sparsified"] == 0 and not nan[1]["z12"].any() and not nan[1]["info"].any()
    _same(alone[0], nan[0])
    _same(alone[1], nan[2])


# ---- chains

def _chain_map():
    """6 key frames, 60 points: the even slots stand at key frame 0 of a make_pair world, the odd ones at key frame 1, each with
    its own set of observed points.  8 pairs (even, odd) with 30, 5, 12, 40, 25, 0, 5 and 7 common points."""
    c = fc.make_pair(60, 3)
    r = lambda a, b: list(range(a, b))  # noqa: E731
    sets = [r(0, 40), r(10, 60), r(20, 60), r(35, 60), r(5, 15), r(0, 12)]
    t = cc.from_kf_lists(sets, 60)
    nobs = len(t["obs_frame"])
    owner = np.repeat(np.arange(60), np.diff(t["mp_ptr"]))
    view, info = np.zeros((nobs, 3), np.float32), np.zeros((nobs, 9), np.float32)
    for e in range(nobs):
        k = int(t["obs_frame"][e]) % 2
        view[e], info[e] = c["z"][owner[e], k], c["info"][owner[e], k].ravel()
    Twc = np.stack([c["kf"][f % 2][:3, :4].ravel() for f in range(6)]).astype(np.float32)
    pairs = (np.array([0, 0, 0, 2, 2, 2, 4, 4], np.int32), np.array([1, 3, 5, 1, 3, 5, 1, 5], np.int32))
    return t, Twc, c["mp"].astype(np.float32), view, info, pairs, [30, 5, 12, 40, 25, 0, 5, 7]


def test_covis_chain_with_one_wait_equals_the_three_calls_with_waits(matcher):
    from se2lam_amd import capi, covis, feat_edge as fe
    t, Twc, pos, view, info, (pa, pb), n_common = _chain_map()
    LIST, ROW, n = 32, 48, len(pa)
    # the parent's route: build, wait, pairs, wait, download, gather on the host, the host call
    cv = covis.build_device(matcher, *cc.tables(t))
    pr = covis.pairs_device(matcher, cv, pa, pb, list_cap=LIST)
    assert pr["out"][:, 0].tolist() == n_common
    g = gm.gather_covis(pa, pb, 6, Twc, pos, ROW, pr["out"], pr["common"], LIST, view, info)
    host, (kf, mp) = _host_route(g, fm.COVIS)
    # the chain: three calls, one wait
    up = capi.upload
    cv2 = covis.DeviceCovis(*cc.tables(t))
    d = dict(a=up(pa, np.int32), b=up(pb, np.int32), out=up(np.full((n, 4), capi.ISENT, np.int32)), ratio=up(np.full((n, 2), capi.SENT, np.float32)),
             common=up(np.full((n, LIST, 3), capi.ISENT, np.int32)), Twc=up(Twc), pos=up(pos), view=up(view), info=up(info))
    buf = fe.FeatEdgeDeviceBuffers(n, ROW)
    cv2.build(matcher, sync=False)
    p = capi.dev_ptr
    capi.check(capi.lib().se2gpu_covis_pairs_device(matcher._h, p(cv2.bits), cv2.nframes, cv2.m, p(d["a"]), p(d["b"]), n, 0.3, 0.1, p(d["out"]),
                                                    p(d["ratio"]), p(d["common"]), LIST, p(cv2.counts), cv2.cap, p(cv2.mp_ptr),
                                                    p(cv2.obs_frame), p(cv2.obs_ftr), cv2.nobs))
    fe.CreateFeatEdgeCovisBatchDevice(matcher, d["a"], d["b"], d["Twc"], d["pos"], d["out"], d["common"], LIST, d["view"], d["info"], ROW,
                                      npairs=n, nframes=6, m=60, nobs=cv2.nobs, buf=buf, sync=False)
    matcher.sync()
    dev, got = buf.read(), buf.read_gather()
    assert np.array_equal(got["count"], g["count"]) and got["count"].tolist() == [30, 5, 12, 32, 25, 0, 5, 7]
    assert got["cut"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    for s in range(n):
        c = int(g["count"][s])
        for k in ("xyz", "z", "info"):
            assert np.array_equal(_bits(got[k][s, :c]), _bits(g[k][s])), (s, k)
        if n_common[s] < 10:
            assert dev[s]["status"] == 1 and not dev[s]["z12"].any()
        else:
            a, b = int(np.sum(g["count"][:s])), int(np.sum(g["count"][:s + 1]))
            assert dev[s]["status"] == 0 and dev[s]["z12"].any()
            _close_to_host(dev[s], host[s], kf[s], mp[a:b], "chain pair %d (%d common)" % (s, n_common[s]))


def test_match_call_queued_behind_another_call_with_one_wait(matcher, tab, mtab, match_result):
    """verify-style rows (-1 where RemoveKPMatch or the RANSAC took a match, -1 from counts[a] on) through the match route, queued
    without a wait behind a covisibility call on the same stream, one wait for both: the same words as the batch that ran and
    was waited for alone, and the host route (download, numpy gather, se2gpu_feat_edge_batch) within the tolerances"""
    before = _run_covis(matcher, tab, [W65, W9, W63], 80, 80, sync=False)[0]
    buf, g = _run_match(matcher, mtab, MATCH8, 130, plant=_match_plant(mtab, 8), sync=False)
    matcher.sync()
    assert [d["status"] for d in before.read()] == [0, 1, 0]
    r, dev = match_result, buf.read()
    for s, (d, h) in enumerate(zip(dev, r["host"])):
        _same(d, r["dev"][s])
        assert d["n_points"] == h["n_points"] == g["count"][s]
        if d["status"] == 1:
            assert d["raw"] < 3 and not d["z12"].any()
        else:
            a, b = int(np.sum(g["count"][:s])), int(np.sum(g["count"][:s + 1]))
            _close_to_host(d, h, r["kf"][s], r["mp"][a:b], "match row %d" % s)


@pytest.mark.parametrize("route", ["covis", "match"])
def test_without_the_optional_outputs_the_required_ones_are_the_same_words(matcher, tab, route):
    """d_mp_xyz_out, d_outlier, d_edge_chi2 and d_stats NULL: the per-point rows go to the work space, no statistics are kept,
    and d_info8 (the outlier count included), kf12_out, z_out12 and info_out36 do not change by a bit"""
    from se2lam_amd import feat_edge as fe
    worlds, run = [W65, W9, W64, W0], (lambda **kw: _run_covis(matcher, tab, worlds, 80, 80, **kw)) if route == "covis" else \
        (lambda **kw: _run_match(matcher, tab, worlds, 80, **kw))
    full = run()[0].read()
    bare = run(buf=fe.FeatEdgeDeviceBuffers(len(worlds), 80, points=False, stats=False))[0].read()
    assert [d["status"] for d in full] == ([0, 1, 0, 1] if route == "covis" else [0, 0, 0, 1])
    assert route == "covis" or full[2]["n_outliers"] >= 5
    for a, b in zip(full, bare):
        for k in ("info8", "kf12", "z12", "info"):
            assert np.array_equal(a[k], b[k]), k
        assert b["stats"]["iterations"] == 0 and len(b["mp"]) == 0


# ---- a camera off the body's axes ----------------------------------------------------------------------------------------------

def test_off_axis_camera_prior_and_a_pair_against_the_model_and_the_host_route(matcher, oracle):
    """two worlds of `tab` (10 and 65 points, the same draws) as a camera at synth.OFF_AXIS_TBC sees them, the call given that
    Tbc12: in k_plane_prior_iso3 the adjoint of Tbc and the products with Tbc^-1 are full matrices.  The prior as
    test_prior_information_to_the_bit_and_measurement_within_the_bound, the pairs as test_covis_route_against_the_model_and_the_host_route."""
    from se2lam_amd import capi, feat_edge as fe, synth
    Tbc = synth.OFF_AXIS_TBC
    tbc = fe.Tbc12(Tbc[:3, :3], Tbc[:3, 3])
    assert np.abs(tbc[:9]).min() > 0.02
    t = dc.Tables(((10, 0), (65, 0)), Tbc=Tbc)
    worlds = [1, 0]
    buf, g = _run_covis(matcher, t, worlds, 130, 130, tbc=tbc)
    got, res = _check_gather(buf, g, "off axis")
    kf = np.ascontiguousarray(g["kf12"].reshape(-1, 12))
    meas, info = np.zeros((len(kf), 12)), np.zeros((len(kf), 36))
    for i in range(len(kf)):
        capi.check(capi.lib().se2gpu_plane_motion_prior_iso3(kf[i].ctypes.data, tbc.ctypes.data, 1e6, 1e6, 1.0, meas[i].ctypes.data,
                                                             info[i].ctypes.data))
    assert np.array_equal(_bits(got["prior_info"].reshape(-1, 36)), _bits(info))
    diff = np.abs(got["prior_meas"].reshape(-1, 12) - meas).max(axis=1)
    assert np.all(diff <= 1e-12 * np.maximum(1.0, np.abs(kf[:, 9:]).max(axis=1)))
    assert np.abs(meas - kf).max() > 1e-3
    host, (kf_in, mp_in) = _host_route(g, fm.COVIS, tbc=tbc)
    dev = buf.read()
    for slot, w in enumerate(worlds):
        c = t.case(w)
        m = fm.optimize(fm.Problem(c["kf"], c["mp"], c["z"], c["info"], fm.COVIS, prior_kw=dict(Rbc=Tbc[:3, :3], tbc=Tbc[:3, 3])), 15)
        label = "off axis covis slot %d (%d points)" % (slot, len(c["mp"]))
        fm.check_against_model(dev[slot], c, m, fm.COVIS, oracle, label)
        a, b = int(np.sum(g["count"][:slot])), int(np.sum(g["count"][:slot + 1]))
        _close_to_host(dev[slot], host[slot], kf_in[slot], mp_in[a:b], label)
