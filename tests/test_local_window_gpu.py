"""se2gpu_covis_connect_device, _disconnect_device and se2gpu_local_window_batch_device on the GPU against the set model
(tests/local_window_model.py) on the maps of tests/covis_cases.py with random directed adjacencies, on the hand cases of
tests/local_window_cases.py, and against the compiled reference's own lists (tests/golden/local_window_ref.npz).

Every output is an integer, so EVERY word of d_win_kf and d_win_mp, every count, every list entry and the sentinels of what a
call leaves alone equal the model exactly.  No case is left out of a comparison."""
import os

import numpy as np
import pytest

import covis_cases as cc
import covis_model as cm
import local_window_cases as lc
import local_window_model as lm

pytestmark = pytest.mark.gpu
COVIS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covis_ref.npz")


@pytest.fixture(scope="module")
def matcher():
    from se2lam_amd.matcher import ORBmatcher
    return ORBmatcher()


def _covis(matcher, t):
    from se2lam_amd import covis
    return covis.build_device(matcher, *cc.tables(t))


def _adjacency(nframes, adj):
    from se2lam_amd import localwindow as lw
    return lw.DeviceAdjacency(nframes, rows=adj)


def _same(got, want, what):
    assert lm.same_window(got, want) is None, (what, lm.same_window(got, want))


@pytest.mark.parametrize("nframes", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("m", [0, 1, 64, 65, 4097])
def test_random_maps_equal_the_model(matcher, nframes, m):
    """the word edges of the key-frame rows up to three words; more than 64 point words, so a lane strides twice; invalid CSR
    entries and adjacency bits past nframes planted; the two observation sides differ and key frames are null at some sizes"""
    from se2lam_amd import localwindow as lw
    seed = 1000 * nframes + m
    t_kf = cc.random_map(seed, nframes, m)
    t_mp = cc.random_map(seed + 500, nframes, m) if nframes in (2, 65, 130) else None
    if t_mp is not None:
        t_mp["mp_null"] = t_kf["mp_null"]                             # one map: the points' null flags are the same
    frame_null = (np.random.default_rng(seed).random(nframes) < 0.15).astype(np.uint8) if nframes >= 63 else None
    adj = lc.random_adjacency(seed, nframes)
    model = lm.Model(cc.tables(t_kf), adj, None if t_mp is None else cc.tables(t_mp), frame_null)
    cv_kf = _covis(matcher, t_kf)
    cv_mp = None if t_mp is None else _covis(matcher, t_mp)
    d_adj = _adjacency(nframes, adj)
    jobs = lc.job_list(nframes)
    ko, mo = lc.permuted_order(seed, nframes), lc.permuted_order(seed + 1, m)
    for level in sorted({0, 1, 3, nframes}):
        for orders in ((None, None), (ko, mo)):
            for caps in ((None, None), (3, 3), (nframes, m)):
                if caps[0] is None and orders[0] is not None:
                    continue                                          # without lists the order arrays are not read
                kw = dict(kf_order=orders[0], mp_order=orders[1], kf_list_cap=caps[0], mp_list_cap=caps[1])
                got = lw.window_device(matcher, cv_kf, d_adj, jobs, level, cv_mp=cv_mp, frame_null=frame_null, **kw)
                _same(got, model.window(jobs, level, **kw), (level, caps, orders[0] is not None))
    if nframes == 130 and m == 4097:
        w = model.window(jobs, 3, kf_list_cap=3, mp_list_cap=3)
        assert (w["out"][:, 0] > 3).any() and (w["out"][:, 1] > 3).any() and (w["out"][:, 2] > 3).any()   # all three truncate
        assert len(set(w["out"][:, 0].tolist())) > 3                  # windows of several sizes


@pytest.mark.parametrize("name", sorted(lc.hand_cases()))
def test_hand_cases(matcher, name):
    from se2lam_amd import localwindow as lw
    h = lc.hand_cases()[name]
    model = lm.Model(cc.tables(h["kf"]), h["adj"], None if h["mp"] is None else cc.tables(h["mp"]), h["frame_null"])
    nframes, m = model.nframes, model.m
    cv_kf = _covis(matcher, h["kf"])
    cv_mp = None if h["mp"] is None else _covis(matcher, h["mp"])
    got = lw.window_device(matcher, cv_kf, _adjacency(nframes, h["adj"]), [h["cur"]], h["level"], cv_mp=cv_mp,
                           frame_null=h["frame_null"], kf_list_cap=nframes, mp_list_cap=m)
    _same(got, model.window([h["cur"]], h["level"], kf_list_cap=nframes, mp_list_cap=m), name)
    assert got["out"][0].tolist() == [len(h["local"]), len(h["ref"]), len(h["mps"]), h["n_obs"]]
    assert got["local_list"][0, :len(h["local"])].tolist() == h["local"] and lw.unpack_rows(got["win_kf"][0], nframes) == [h["local"], h["ref"]]
    assert got["ref_list"][0, :len(h["ref"])].tolist() == h["ref"] and got["mp_list"][0, :len(h["mps"])].tolist() == h["mps"]


def test_fixture_of_the_compiled_reference(matcher):
    """the maps of tests/golden/local_window_ref.npz on the device: the lists through the id order arrays equal
    mLocalGraphKFs, mRefKFs and mLocalGraphMPs of the compiled reference, order included"""
    from se2lam_amd import localwindow as lw
    maps = lc.golden_maps()
    assert len(maps) >= 90
    for i, g in enumerate(maps):
        nkf, m = len(g["kf_id"]), len(g["mp_id"])
        cv = _covis(matcher, lc.golden_tables(g))
        got = lw.window_device(matcher, cv, _adjacency(nkf, g["adj"]), np.arange(nkf), 3, kf_order=lc.id_order(g["kf_id"]),
                               mp_order=lc.id_order(g["mp_id"]), kf_list_cap=nkf, mp_list_cap=m)
        for cur, (local, ref, mps) in enumerate(g["jobs"]):
            assert got["out"][cur, :3].tolist() == [len(local), len(ref), len(mps)], (i, cur)
            for key, want, cap in (("local_list", local, nkf), ("ref_list", ref, nkf), ("mp_list", mps, m)):
                assert got[key][cur].tolist() == want + [lm.ISENT] * (cap - len(want)), (i, cur, key)


def test_connect_and_disconnect_equal_the_model(matcher):
    from se2lam_amd import localwindow as lw
    for nframes in (1, 64, 65, 130):
        rng = np.random.default_rng(nframes)
        adj = [set(a) for a in lc.random_adjacency(nframes, nframes, tail_bits=False)]
        d = _adjacency(nframes, adj)
        pa = np.r_[rng.integers(0, nframes, 50), -1, 0, nframes, nframes - 1].astype(np.int32)
        pb = np.r_[rng.integers(0, nframes, 50), 0, nframes, 0, nframes - 1].astype(np.int32)
        d.connect(matcher, pa, pb)                                    # the unconditional links
        lm.connect(adj, pa, pb)
        assert d.read_lists() == [sorted(a) for a in adj], nframes
        qa, qb = rng.integers(0, nframes, 50).astype(np.int32), rng.integers(0, nframes, 50).astype(np.int32)
        out = rng.integers(0, 4, (50, 4)).astype(np.int32)
        for mask in (2, 1):
            d.connect(matcher, qa, qb, out, mask)
            lm.connect(adj, qa, qb, out, mask)
            assert d.read_lists() == [sorted(a) for a in adj], (nframes, mask)
        a0 = int(pa[0])
        slots = np.array([a0, nframes, int(pb[0]), -1, a0, nframes - 1], np.int32)   # two that name each other, one twice
        d.disconnect(matcher, slots)
        lm.disconnect(adj, slots)
        assert d.read_lists() == [sorted(a) for a in adj], nframes
        assert adj[a0] == set() and adj[nframes - 1] == set()
        d.connect(matcher, [], [])
        d.disconnect(matcher, [])                                     # nothing to do, nothing launched
        assert d.read_lists() == [sorted(a) for a in adj], nframes


def test_disconnect_of_two_slots_that_name_each_other(matcher):
    """0 <-> 1, 2 -> 0 one way, 1 -> 3 and 3 -> 1: after setNull of 0 and 1, in either order, rows 0 and 1 are empty, 3 has
    lost 1, and 2 keeps 0 because 0 never listed 2 (KeyFrame.cpp:107-109)"""
    adj = [[1], [0, 3], [0], [1]]
    for slots in ([0, 1], [1, 0]):
        d = _adjacency(4, adj).disconnect(matcher, slots)
        assert d.read_lists() == [[], [], [0], []] == [sorted(a) for a in lm.disconnect([set(a) for a in adj], slots)]


def test_connect_on_the_covisibility_fixture(matcher):
    """tests/golden/covis_ref.npz: pairs (new_kf x local_kfs) -> connect with flag_mask 1; row and column new_kf of d_adj
    equal what Map::updateCovisibility of the compiled reference connected, and nothing else is set"""
    from se2lam_amd import covis, localwindow as lw
    for i, g in enumerate(cc.golden_maps(COVIS_GOLDEN)):
        cv = _covis(matcher, g["tables"])
        new, local = g["new_kf"], g["local_kfs"]
        out = covis.pairs_device(matcher, cv, [new] * len(local), local)["out"]
        d = lw.DeviceAdjacency(g["nkf"]).connect(matcher, [new] * len(local), local, out, 1)
        want = [set() for _ in range(g["nkf"])]
        for b in g["connect"]:
            want[new].add(b)
            want[b].add(new)
        assert d.read_lists() == [sorted(s) for s in want], i


def test_chain_on_the_stream_with_one_wait(matcher):
    """build -> pairs -> connect -> window queued on the matcher's stream, a single se2gpu_matcher_sync at the end; connect reads
    the flags where se2gpu_covis_pairs_device left them in device memory"""
    from se2lam_amd import capi, covis, localwindow as lw
    nframes, m = 70, 4097
    t = cc.random_map(5, nframes, m)
    cmodel = cm.Model(*cc.tables(t))
    rng = np.random.default_rng(6)
    pa = np.repeat(np.arange(nframes), 4).astype(np.int32)
    pb = ((pa + rng.integers(-3, 4, len(pa))) % nframes).astype(np.int32)
    jobs = lc.job_list(nframes)
    ko, mo = lc.permuted_order(7, nframes), lc.permuted_order(8, m)
    # the model's chain
    flags = cmodel.pairs(pa, pb, 0.3, 0.1)["out"]
    adj = lm.connect([set() for _ in range(nframes)], pa, pb, flags, 1)
    assert 0 < sum(len(a) for a in adj) < nframes * 8
    want = lm.Model(cc.tables(t), adj).window(jobs, 3, kf_order=ko, mp_order=mo, kf_list_cap=8, mp_list_cap=100)
    # the device's
    cv = covis.DeviceCovis(*cc.tables(t)).build(matcher, sync=False)
    d_a, d_b = capi.upload(pa, np.int32), capi.upload(pb, np.int32)
    d_out = capi.upload(np.full((len(pa), 4), cm.ISENT, np.int32), np.int32)
    d_ratio = capi.upload(np.zeros((len(pa), 2), np.float32), np.float32)
    capi.check(capi.lib().se2gpu_covis_pairs_device(matcher._h, cv.bits.ptr, nframes, m, d_a.ptr, d_b.ptr, len(pa), 0.3, 0.1,
                                                    d_out.ptr, d_ratio.ptr, None, 0, None, 0, None, None, None, 0))
    d = lw.DeviceAdjacency(nframes).connect(matcher, pa, pb, d_out, 1, sync=False)
    p = lw.window_device(matcher, cv, d, jobs, 3, kf_order=ko, mp_order=mo, kf_list_cap=8, mp_list_cap=100, sync=False)
    matcher.sync()
    assert d.read_lists() == [sorted(a) for a in adj]
    _same(p.read(), want, "chain")


def test_a_second_run_and_a_shuffled_batch_give_the_same_words(matcher):
    from se2lam_amd import localwindow as lw
    nframes, m = 130, 4097
    t = cc.random_map(77, nframes, m)
    adj = lc.random_adjacency(77, nframes)
    cv, d = _covis(matcher, t), _adjacency(nframes, adj)
    jobs = lc.job_list(nframes)
    kw = dict(kf_order=lc.permuted_order(1, nframes), mp_order=lc.permuted_order(2, m), kf_list_cap=9, mp_list_cap=50)
    first = lw.window_device(matcher, cv, d, jobs, 3, **kw)
    _same(lw.window_device(matcher, cv, d, jobs, 3, **kw), first, "the same call twice")
    perm = np.random.default_rng(3).permutation(len(jobs))
    shuffled = lw.window_device(matcher, cv, d, jobs[perm], 3, **kw)
    _same(shuffled, {k: v[perm] for k, v in first.items()}, "a job's outputs do not depend on its place in the batch")
    one = lw.window_device(matcher, cv, d, jobs[7:8], 3, **kw)
    _same(one, {k: v[7:8] for k, v in first.items()}, "a job alone")
    assert lw.window_device(matcher, cv, d, [], 3, **kw)["out"].shape == (0, 4)   # no jobs: nothing launched
    assert np.array_equal(d.read(), lw.pack_rows(adj, nframes))        # the window call leaves d_adj alone, tail bits included
