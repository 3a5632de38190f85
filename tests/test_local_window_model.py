"""The set model of the local-window calls (tests/local_window_model.py) held to the compiled reference's own lists
(tests/golden/local_window_ref.npz), to the library's host implementation on consistent maps (se2gpu_map_update_local_graph)
and to hand-worked cases (tests/local_window_cases.py); and the header's host functions (include/se2lam_amd/LocalWindow.h,
through tests/cpp_local_window.cpp) held to the golden and to the model.  Everything is an integer: every comparison is exact.

The compiled reference's driver builds consistent maps without nulls, so null points, null key frames and observation sides
that disagree are pinned by the model and the hand cases only."""
import itertools

import numpy as np
import pytest

import covis_cases as cc
import local_window_cases as lc
import local_window_model as lm

HAND = lc.hand_cases()


@pytest.fixture(scope="module")
def golden():
    return lc.golden_maps()


def _model_lists(model, cur, level, kf_id, mp_id):
    local, refs, mps, n_obs = model.update_local_graph(cur, level)
    return (sorted(local, key=lambda a: kf_id[a]), sorted(refs, key=lambda a: kf_id[a]), sorted(mps, key=lambda p: mp_id[p]), n_obs)


def test_golden_file_covers_what_it_is_for(golden):
    partial, with_ref, one_way, in_order = lc.golden_coverage(golden)
    assert len(golden) >= 90 and partial >= 0.5 and with_ref >= 0.5 and one_way >= 20 and in_order == 0
    assert all(3 <= len(g["kf_id"]) <= 12 and 10 <= len(g["mp_id"]) <= 80 for g in golden)
    assert all(len(g["jobs"]) == len(g["kf_id"]) for g in golden)     # every key frame serves once as the current one
    assert any(len(j[0]) >= 4 for g in golden for j in g["jobs"])     # the three hops are walked, not only the first


def test_model_equals_the_compiled_reference(golden):
    n = 0
    for i, g in enumerate(golden):
        model = lm.Model(cc.tables(lc.golden_tables(g)), g["adj"])
        for cur, (local, ref, mps) in enumerate(g["jobs"]):
            got = _model_lists(model, cur, 3, g["kf_id"], g["mp_id"])
            assert got[0] == local and got[1] == ref and got[2] == mps, (i, cur)
            assert got[3] == sum(len(set(g["kf_obs"][f]) & set(mps)) for f in local + ref), (i, cur)
            n += 1
    assert n > 500


def test_model_equals_the_host_implementation_on_consistent_maps(golden):
    from se2lam_amd.mapview import updateLocalGraph
    from test_mapview import _random_map
    rng = np.random.default_rng(23)
    views = [_random_map(rng, K, M, reach) for K, M, reach in ((6, 40, 2), (60, 900, 3), (70, 300, 1))]
    for g in golden[:10]:
        mp_obs = [[f for f in range(len(g["kf_id"])) if p in g["kf_obs"][f]] for p in range(len(g["mp_id"]))]
        views.append((g["kf_id"], g["adj"], g["kf_obs"], g["mp_id"], mp_obs))
    for kf_id, covisible, kf_obs, mp_id, mp_obs in views:
        K, M = len(kf_id), len(mp_id)
        model = lm.Model(cc.tables(cc.from_kf_lists(kf_obs, M, cap=1 << 12)), covisible)
        for cur, level in itertools.product(sorted({0, K // 2, K - 1}), (0, 1, 3, K)):
            lk, rk, mps = updateLocalGraph(kf_id, covisible, kf_obs, mp_id, mp_obs, cur, level)
            want = _model_lists(model, cur, level, kf_id, mp_id)
            assert lk.tolist() == want[0] and rk.tolist() == want[1] and mps.tolist() == want[2], (K, cur, level)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case_against_the_model(name):
    h = HAND[name]
    model = lm.Model(cc.tables(h["kf"]), h["adj"], None if h["mp"] is None else cc.tables(h["mp"]), h["frame_null"])
    local, refs, mps, n_obs = model.update_local_graph(h["cur"], h["level"])
    assert (sorted(local), sorted(refs), sorted(mps), n_obs) == (h["local"], h["ref"], h["mps"], h["n_obs"])
    w = model.window([h["cur"]], h["level"], kf_list_cap=2, mp_list_cap=1)
    assert w["out"][0].tolist() == [len(h["local"]), len(h["ref"]), len(h["mps"]), h["n_obs"]]
    assert w["local_list"][0].tolist() == (h["local"] + [lm.ISENT] * 2)[:2] and w["mp_list"][0].tolist() == h["mps"][:1]


def test_an_in_place_sweep_would_reach_too_far():
    """the bug the chain cases are there for, shown on the model's own inputs"""
    h = HAND["chain_ascending"]
    local = {h["cur"]}
    for _ in range(h["level"]):
        for a in range(6):                                            # ascending slots, expanding what this round added
            if a in local:
                local |= set(h["adj"][a])
    assert sorted(local) == [0, 1, 2, 3, 4, 5] and h["local"] == [0, 1, 2, 3]


def test_window_model_on_an_irregular_map():
    t = cc.random_map(3, 65, 129)
    adj = lc.random_adjacency(3, 65)
    assert any(b >= 65 for a in adj for b in a)                       # tail bits planted, ignored below
    model = lm.Model(cc.tables(t), adj, frame_null=(np.arange(65) % 7 == 0))
    jobs = lc.job_list(65)
    order = lc.permuted_order(1, 65)
    w = model.window(jobs, 3, kf_order=order, kf_list_cap=3, mp_list_cap=129)
    bad = [j for j, c in enumerate(jobs) if not 0 <= c < 65]
    assert len(bad) == 2 and all(w["out"][j].tolist() == [-1, 0, 0, 0] for j in bad)
    assert all((w["win_kf"][j] == lm.WSENT).all() and (w["local_list"][j] == lm.ISENT).all() for j in bad)
    ok = [j for j in range(len(jobs)) if j not in bad]
    assert (w["out"][ok, 0] > 3).any() and (w["out"][ok, 0] < 65).all()   # truncation happens; no window is the whole map
    assert not (w["win_kf"][ok][:, :, 1] >> np.uint64(1)).any()       # bits past 65 are zero in both rows
    assert not (w["win_kf"][ok][:, 0] & w["win_kf"][ok][:, 1]).any()   # local and ref are disjoint
    j = ok[5]
    members = [s for s in order if 0 <= s < 65 and (int(w["win_kf"][j, 0, s >> 6]) >> (s & 63)) & 1]
    assert w["local_list"][j].tolist() == (members + [lm.ISENT] * 3)[:3]


def test_upkeep_model():
    adj = [set() for _ in range(4)]
    lm.connect(adj, [0, 1, 2, 9, 3], [1, 2, 2, 0, -1])
    assert adj == [{1}, {0, 2}, {1, 2}, set()]                        # both ways; a == b one bit; out of range skipped
    lm.connect(adj, [0, 0], [3, 2], pair_out=[[5, 9, 9, 0b10], [5, 9, 9, 0b01]], flag_mask=1)
    assert adj == [{1, 2}, {0, 2}, {0, 1, 2}, set()]
    adj[3].add(0)                                                     # 3 lists 0, 0 does not list 3
    both = [lm.disconnect([set(a) for a in adj], order) for order in ([0, 2], [2, 0], [0, 2, 0])]
    # rows 0 and 2 named 1, so 1 loses both; 3 lists 0 while 0 does not list 3, so 3 keeps 0 (KeyFrame.cpp:107-109)
    assert both[0] == both[1] == both[2] == [set(), set(), set(), {0}]


# ---- include/se2lam_amd/LocalWindow.h

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return lc.cpp_build(tmp_path_factory.mktemp("local_window"))


def test_header_host_functions_equal_the_compiled_reference(program, tmp_path, golden):
    lines, want = [], []
    for g in golden:
        nkf, m = len(g["kf_id"]), len(g["mp_id"])
        mp_obs = [[f for f in range(nkf) if p in g["kf_obs"][f]] for p in range(m)]
        lines += lc.cpp_map_lines(g["kf_id"], g["mp_id"], g["kf_obs"], mp_obs, g["adj"])
        for cur, job in enumerate(g["jobs"]):
            lines.append("U %d 3" % cur)
            want.append(job)
    got = lc.cpp_run(program, tmp_path / "golden.txt", lines)
    assert len(got) == len(want) > 500
    for g, w in zip(got, want):
        assert g[0] == "U" and (g[2], g[3], g[4]) == w


def test_header_host_functions_equal_the_model(program, tmp_path):
    lines, want = [], []
    for name in sorted(HAND):
        h = HAND[name]
        model = lm.Model(cc.tables(h["kf"]), h["adj"], None if h["mp"] is None else cc.tables(h["mp"]), h["frame_null"])
        nkf, m = model.nframes, model.m
        mp_null = [0 if p in model.notnull else 1 for p in range(m)]
        lines += lc.cpp_map_lines(range(nkf), range(m), model.kf_obs, model.mp_obs, model.adj, h["frame_null"], mp_null)
        for level in (0, 1, h["level"], nkf):
            lines.append("U %d %d" % (h["cur"], level))
            local, refs, mps, n_obs = model.update_local_graph(h["cur"], level)
            want.append(("U", n_obs, sorted(local), sorted(refs), sorted(mps)))
    # upkeep on a random directed graph: connect, then setNull of slots that name each other and of one listed twice
    adj = [set(a) for a in lc.random_adjacency(8, 20, tail_bits=False)]
    lines += lc.cpp_map_lines(range(20), [], adj, [], adj)
    pa, pb = [0, 5, 7, 7, 19], [1, 5, 3, 12, 0]
    lines += ["C %d %d" % ab for ab in zip(pa, pb)] + ["G"]
    lm.connect(adj, pa, pb)
    want += [("G", f, sorted(a)) for f, a in enumerate(adj)]
    lines += ["D 7", "D 3", "D 0", "D 7", "G"]
    lm.disconnect(adj, [7, 3, 0, 7])
    assert adj[7] == adj[3] == adj[0] == set()
    want += [("G", f, sorted(a)) for f, a in enumerate(adj)]
    got = lc.cpp_run(program, tmp_path / "cases.txt", lines)
    assert [tuple(g) for g in got] == want
