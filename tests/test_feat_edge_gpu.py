"""se2gpu_feat_edge_batch (csrc/feat_edge.hip + k_sparsify) on the GPU against tests/feat_edge_model.py, the independent dense
numpy Levenberg-Marquardt, and - for the sparsifier stage - against oracle.sparsify fed the device's own poses and inliers.

Tolerances are the project's (tests/test_pg_gpu.py, BASELINE's BA tolerance): chi2 at the start rel 1e-11, LM histories rtol
1e-5 with equal trial counts over the compared prefix (feat_edge_model.compared_prefix: near convergence a trial is accepted
or rejected by rounding), final poses and points within 1e-5 of the model's largest update, edge chi2 rtol 1e-4 / atol 1e-7,
the outlier mask exact (the cases keep every edge chi2 more than 1e-3 relative away from the threshold), sparsifier output
as tests/test_sparsify.py.  Every model and every device batch is computed once for the module."""
import numpy as np
import pytest

import feat_edge_cases as fc
import feat_edge_model as fm

pytestmark = pytest.mark.gpu
REL = fm.REL

# match mode, 30 iterations, 16 pairs: the six shapes, the two pairs with planted outliers, a pair with no point and one below
# min_points inside the batch, and the first pair again in the last place
M16 = [("m", 65, 0, 0), ("m", 3, 0, 0), ("m", 10, 0, 0), ("m", 63, 0, 0), ("m", 64, 0, 0), ("m", 130, 0, 0), ("m", 40, 0, 5),
       ("m", 65, 1, 9), ("empty", 0, 0, 0), ("m", 2, 0, 0), ("m", 10, 0, 0), ("m", 3, 0, 0), ("m", 64, 0, 0), ("m", 63, 0, 0),
       ("m", 10, 0, 0), ("m", 65, 0, 0)]
# covisibility mode, 15 iterations, 7 pairs: its five shapes, and two pairs below its minimum of 10
C7 = [("c", 10, 0, 0), ("c", 63, 0, 0), ("c", 3, 0, 0), ("c", 64, 0, 0), ("c", 65, 0, 0), ("empty", 0, 0, 0), ("c", 130, 0, 0)]


def _case(key):
    kind, N, seed, planted = key
    return fc.empty_pair(seed) if kind == "empty" else fc.make_pair(N, seed, n_outliers=planted)


@pytest.fixture(scope="module")
def world():
    from se2lam_amd import feat_edge as fe
    cases = {k: _case(k) for k in set(M16 + C7)}
    q = fc.REJECTING
    rej = fc.make_pair(q["N"], q["seed"], turn_y=q["turn_y"])
    models = {}
    for k, c in cases.items():
        mode = fm.COVIS if k[0] == "c" else fm.MATCH
        if k[0] != "empty" and k[1] >= (10 if mode == fm.COVIS else 3):
            models[k] = fm.optimize(fm.Problem(c["kf"], c["mp"], c["z"], c["info"], mode), 15 if mode == fm.COVIS else 30)
    w = dict(cases=cases, models=models, rej_case=rej,
             rej_model=fm.optimize(fm.Problem(rej["kf"], rej["mp"], rej["z"], rej["info"], fm.COVIS), q["iters"]))
    tup = lambda keys: [fc.as_tuple(cases[k]) for k in keys]
    w["m16"] = fe.CreateFeatEdgeBatch(tup(M16), fe.MATCH)
    w["m16_again"] = fe.CreateFeatEdgeBatch(tup(M16), fe.MATCH)
    w["m1"] = fe.CreateFeatEdgeBatch(tup(M16[:1]), fe.MATCH)
    w["m14"] = fe.CreateFeatEdgeBatch(tup([k for k in M16 if k[1] >= 3]), fe.MATCH)     # without the two status-1 pairs
    w["c7"] = fe.CreateFeatEdgeBatch(tup(C7), fe.COVIS)
    w["rej"] = fe.CreateFeatEdgeBatch([fc.as_tuple(rej)], fe.COVIS, iters=q["iters"])
    return w


def _same(a, b):
    for k in ("status", "n_points", "n_outliers", "n_sparsified", "kf12", "mp", "outlier", "edge_chi2", "z12", "info"):
        assert np.array_equal(a[k], b[k]), k
    for k, v in a["stats"].items():
        assert np.array_equal(v, b["stats"][k]), k


@pytest.mark.parametrize("slot", [i for i, k in enumerate(M16[:8])])
def test_match_mode_against_the_model(world, oracle, slot):
    k = M16[slot]
    fm.check_against_model(world["m16"][slot], world["cases"][k], world["models"][k], fm.MATCH, oracle, "match N=%d seed %d planted %d" % k[1:])
    if k[3]:
        assert np.all(world["m16"][slot]["outlier"][world["cases"][k]["planted"]])


@pytest.mark.parametrize("slot", [i for i, k in enumerate(C7) if k[1] >= 10])
def test_covis_mode_against_the_model(world, oracle, slot):
    k = C7[slot]
    got = world["c7"][slot]
    fm.check_against_model(got, world["cases"][k], world["models"][k], fm.COVIS, oracle, "covis N=%d seed %d" % k[1:3])
    assert not got["outlier"].any()


def test_rejected_trials_follow_the_model(world, oracle):
    m, got = world["rej_model"], world["rej"][0]
    n = fm.compared_prefix(m["chi2_init"], m["chi2_hist"])
    assert (m["trials_hist"][:n] >= 2).any(), "the case must make the model reject trials inside the compared prefix"
    fm.check_against_model(got, world["rej_case"], m, fm.COVIS, oracle, "turned start")
    assert got["stats"]["trials"] == int(m["trials_hist"].sum())


def test_a_pair_does_not_depend_on_run_batch_or_position(world):
    alone, batch, again = world["m1"][0], world["m16"], world["m16_again"]
    _same(alone, batch[0])
    _same(alone, batch[15])
    for a, b in zip(batch, again):
        _same(a, b)


def test_pairs_below_the_minimum_are_not_run_and_disturb_nobody(world, oracle):
    for res, keys, slots, minimum in ((world["m16"], M16, (8, 9), 3), (world["c7"], C7, (2, 5), 10)):
        for s in slots:
            got, c = res[s], world["cases"][keys[s]]
            assert len(c["mp"]) < minimum
            assert got["status"] == 1 and got["n_points"] == len(c["mp"]) and got["n_outliers"] == 0 and got["n_sparsified"] == 0
            assert np.array_equal(got["kf"], c["kf"]) and np.array_equal(got["mp"], c["mp"])
            assert not got["z12"].any() and not got["info"].any() and not got["outlier"].any() and not got["edge_chi2"].any()
            st = got["stats"]
            assert st["iterations"] == 0 and st["trials"] == 0 and st["chi2_init"] == 0 and st["chi2_final"] == 0 and st["lambda_final"] == 0
    others = [r for r, k in zip(world["m16"], M16) if k[1] >= 3]
    assert len(others) == len(world["m14"]) == 14
    for a, b in zip(others, world["m14"]):
        _same(a, b)


def test_all_points_rejected_gives_the_sparsifiers_answer_for_no_points(world, oracle):
    """the minimum is on the raw count (GlobalMapper.cpp:790): a threshold below every edge's chi2 rejects all points, and the
    constraint is what k_sparsify gives for none"""
    from se2lam_amd import feat_edge as fe
    c = world["cases"][("m", 10, 0, 0)]
    got = fe.CreateFeatEdgeBatch([fc.as_tuple(c)], fe.MATCH, outlier_chi2=1e-12)[0]
    assert got["status"] == 0 and got["outlier"].all() and got["n_outliers"] == 10 and got["n_sparsified"] == 0
    ref = world["m16"][2]
    assert np.array_equal(got["kf12"], ref["kf12"]) and np.array_equal(got["mp"], ref["mp"])     # the rejection follows the optimisation
    zr, ir, _ = oracle.sparsify(got["kf"], np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3, 3)))
    assert np.allclose(got["z"], zr, atol=1e-12) and np.abs(got["info"] - ir).max() <= REL * np.abs(ir).max()
    none = fe.CreateFeatEdgeBatch([fc.as_tuple(c)], fe.MATCH, outlier_chi2=0.0)[0]               # <= 0: no rejection
    assert none["status"] == 0 and not none["outlier"].any() and none["n_sparsified"] == 10
