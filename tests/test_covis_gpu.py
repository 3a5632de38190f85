"""se2gpu_covis_build_device, _pairs_device and _refset_device on the GPU against the set model (tests/covis_model.py) on the
maps of tests/covis_cases.py, and against the compiled reference's own results (tests/golden/covis_ref.npz).

Everything is an integer or a single IEEE operation, so EVERY output equals the model exactly: the words of d_bits, the sizes,
the counts and flags, the float and double ratios (NaN equal to NaN), the lists and the sentinels of what a call leaves alone.
No case is left out of a comparison."""
import os

import numpy as np
import pytest

import covis_cases as cc
import covis_model as cm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covis_ref.npz")


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


def _device(matcher, t):
    from se2lam_amd import covis
    return covis.build_device(matcher, *cc.tables(t))


def _same_pairs(got, want, what):
    assert np.array_equal(got["out"], want["out"]), what
    assert cm.same_floats(got["ratio"], want["ratio"]), what
    if want["common"] is None:
        assert got["common"] is None
    else:
        assert np.array_equal(got["common"], want["common"]), what


def _same_jobs(got, want, what):
    assert np.array_equal(got["out"], want["out"]), what
    assert cm.same_floats(got["ratio"], want["ratio"]), what


@pytest.mark.parametrize("nframes", [2, 5, 70])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 129, 4097])
def test_random_maps_equal_the_model(matcher, nframes, m):
    """word edges and one point past a wave's 64 x 64-bit stride; more than 64 reference frames in one job at 70 frames;
    invalid entries and descending d_mp_ptr segments planted"""
    from se2lam_amd import covis
    t = cc.random_map(1000 * nframes + m, nframes, m)
    model = cm.Model(*cc.tables(t))
    cv = _device(matcher, t)
    assert np.array_equal(cv.read_bits(), model.bits())
    assert np.array_equal(cv.read_size_obs(), model.size_obs())
    pa, pb = cc.pair_list(m, nframes, None if nframes <= 5 else 40)
    _same_pairs(covis.pairs_device(matcher, cv, pa, pb), model.pairs(pa, pb), "no list")
    for list_cap in (0, 3, m):
        want = model.pairs(pa, pb, np.float32(0.3), 0.1, list_cap)
        _same_pairs(covis.pairs_device(matcher, cv, pa, pb, 0.3, 0.1, list_cap), want, "list_cap %d" % list_cap)
    if m == 4097:
        assert (want["out"][:, 0] > 3).any() and (want["common"][:, :, 0] == cm.ISENT).any()   # truncated at 3, sentinels at m
    kf, rp, ri = cc.job_list(m + 1, nframes, 24, 80 if nframes == 70 else 9)
    for k in (1, 2, 3, 7):
        _same_jobs(covis.refset_device(matcher, cv, kf, rp, ri, k, 0.8), model.refset(kf, rp, ri, k, 0.8), "k %d" % k)
    # other thresholds than the reference's constants
    _same_pairs(covis.pairs_device(matcher, cv, pa, pb, 0.55, 0.7), model.pairs(pa, pb, 0.55, 0.7), "ratios 0.55, 0.7")
    _same_jobs(covis.refset_device(matcher, cv, kf, rp, ri, 2, 0.5), model.refset(kf, rp, ri, 2, 0.5), "thresh 0.5")


@pytest.mark.parametrize("name", sorted(cc.hand_cases()))
def test_hand_cases(matcher, name):
    from se2lam_amd import covis
    t, call, want = cc.hand_cases()[name]
    model = cm.Model(*cc.tables(t))
    cv = _device(matcher, t)
    assert np.array_equal(cv.read_bits(), model.bits()) and np.array_equal(cv.read_size_obs(), model.size_obs())
    if call[0] == "pairs":
        got = covis.pairs_device(matcher, cv, [call[1]], [call[2]], 0.3, 0.1, 64)
        _same_pairs(got, model.pairs([call[1]], [call[2]], 0.3, 0.1, 64), name)
        assert tuple(got["out"][0]) == want["out"] and cm.same_floats(got["ratio"][0], np.asarray(want["ratio"], np.float32))
        if "common" in want:
            assert got["common"][0, :len(want["common"]), 0].tolist() == want["common"]
    else:
        got = covis.refset_device(matcher, cv, [call[1]], [0, len(call[2])], call[2], call[3], 0.8)
        assert tuple(got["out"][0]) == want["out"] and got["ratio"][0] == want["ratio"]


def test_empty_inputs(matcher):
    """m == 0 still writes zero counts for the pairs; empty reference lists; no jobs and no pairs"""
    from se2lam_amd import covis
    t = cc.from_kf_lists([[], [], []], 0)
    cv = _device(matcher, t)
    assert (cv.read_size_obs() == cm.ISENT).all()                     # m == 0 launches nothing
    model = cm.Model(*cc.tables(t))
    pa, pb = cc.pair_list(0, 3)
    got = covis.pairs_device(matcher, cv, pa, pb, list_cap=2)
    _same_pairs(got, model.pairs(pa, pb, list_cap=2), "m = 0")
    assert got["out"][0].tolist() == [0, 0, 0, 0] and np.isnan(got["ratio"][0]).all()
    got = covis.refset_device(matcher, cv, [0, 1], [0, 0, 0], [], 1, 0.8)
    assert got["out"].tolist() == [[0, 0, 0]] * 2 and got["ratio"].tolist() == [-1.0, -1.0]
    assert covis.pairs_device(matcher, cv, [], [])["out"].shape == (0, 4)
    assert covis.refset_device(matcher, cv, [], [0], [])["out"].shape == (0, 3)


def test_outputs_depend_on_their_own_pair_or_job_and_not_on_the_run(matcher):
    from se2lam_amd import covis
    t = cc.random_map(77, 5, 4097)
    cv = _device(matcher, t)
    bits = cv.read_bits()
    pa, pb = cc.pair_list(0, 5)
    one = covis.pairs_device(matcher, cv, [3], [1], list_cap=40)
    first = covis.pairs_device(matcher, cv, np.r_[3, pa], np.r_[1, pb], list_cap=40)
    last = covis.pairs_device(matcher, cv, np.r_[pa, 3], np.r_[pb, 1], list_cap=40)
    for k in ("out", "ratio", "common"):
        assert np.array_equal(one[k][0], first[k][0]) and np.array_equal(one[k][0], last[k][-1]), k
    again = covis.pairs_device(matcher, cv, np.r_[pa, 3], np.r_[pb, 1], list_cap=40)
    _same_pairs(again, last, "the same call twice")
    kf, rp, ri = cc.job_list(5, 5, 12, 9)
    s, e = rp[4], rp[5]
    one = covis.refset_device(matcher, cv, [kf[4]], [0, e - s], ri[s:e], 2)
    many = covis.refset_device(matcher, cv, kf, rp, ri, 2)
    lastj = covis.refset_device(matcher, cv, np.r_[kf, kf[4]], np.r_[rp, rp[-1] + e - s], np.r_[ri, ri[s:e]], 2)
    for k in ("out", "ratio"):
        assert np.array_equal(one[k][0], many[k][4]) and np.array_equal(one[k][0], lastj[k][-1]), k
    _same_jobs(covis.refset_device(matcher, cv, kf, rp, ri, 2), many, "the same call twice")
    assert np.array_equal(cv.read_bits(), bits)                       # the queries leave d_bits alone
    cv.build(matcher)                                                 # the memset is inside the call
    assert np.array_equal(cv.read_bits(), bits) and np.array_equal(cv.read_size_obs(), cm.Model(*cc.tables(t)).size_obs())


def test_chain_on_the_stream_with_one_wait(matcher):
    """build -> pairs -> refset queued on the matcher's stream, a single se2gpu_matcher_sync at the end"""
    from se2lam_amd import covis
    t = cc.random_map(5, 70, 4097)
    model = cm.Model(*cc.tables(t))
    pa, pb = cc.pair_list(9, 70, 40)
    kf, rp, ri = cc.job_list(9, 70, 24, 80)
    cv = covis.DeviceCovis(*cc.tables(t)).build(matcher, sync=False)
    p = covis.pairs_device(matcher, cv, pa, pb, list_cap=8, sync=False)
    r = covis.refset_device(matcher, cv, kf, rp, ri, 2, 0.8, sync=False)
    matcher.sync()
    assert np.array_equal(cv.read_bits(), model.bits()) and np.array_equal(cv.read_size_obs(), model.size_obs())
    _same_pairs(p.read(), model.pairs(pa, pb, list_cap=8), "chain")
    _same_jobs(r.read(), model.refset(kf, rp, ri, 2, 0.8), "chain")


def test_fixture_of_the_compiled_reference(matcher):
    """the 100 maps of tests/golden/covis_ref.npz on the device: Map::compareViewMPs of the compiled reference in both
    overloads (ratios to the bit, the common points through the list) and what Map::updateCovisibility connected"""
    from se2lam_amd import covis
    for i, g in enumerate(cc.golden_maps(GOLDEN)):
        t = g["tables"]
        cv = _device(matcher, t)
        m = len(t["mp_null"])
        got = covis.pairs_device(matcher, cv, [p[0] for p in g["pairs"]], [p[1] for p in g["pairs"]], 0.3, 0.1, m)
        for (a, b, ratio, common), out, r, cl in zip(g["pairs"], got["out"], got["ratio"], got["common"]):
            assert out[0] == len(common) and cm.same_floats(r, ratio), (i, a, b)
            assert cl[:len(common), 0].tolist() == common and (cl[len(common):] == cm.ISENT).all(), (i, a, b)
        ptr = np.cumsum([0] + [len(j[1]) for j in g["jobs"]])
        idx = [f for j in g["jobs"] for f in j[1]]
        r = covis.refset_device(matcher, cv, [j[0] for j in g["jobs"]], ptr, idx, 2, 0.8)
        want = np.array([j[2] for j in g["jobs"]])
        assert cm.same_floats(r["ratio"], want) and r["out"][:, 0].tolist() == [len(j[3]) for j in g["jobs"]], i
        assert r["out"][:, 2].tolist() == [int(x >= 0.8) for x in want], i
        local = g["local_kfs"]
        flags = covis.pairs_device(matcher, cv, [g["new_kf"]] * len(local), local)["out"][:, 3]
        assert [f for f, fl in zip(local, flags) if fl & 1] == g["connect"], i
