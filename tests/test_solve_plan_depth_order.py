"""The ORDER of a tile task's dependency list (csrc/ba.hip: solve_plan_build) - host code, no device needed.
A task of k_chol_tiles takes the entries of its list strictly one after the other, so the list is written in the order in which
the block columns are published: by depth on the dependency chain, ties by index.  Where two chains of equal length meet - the
last columns of the two arcs of a ring in front of the first separator column - only those two are left to multiply when they
arrive, and both are polled in earnest (`neager` = the number of entries of the largest depth at the end of the list)."""
import ctypes as C

import numpy as np
import pytest

from test_solve_plan import NB, _band, _plan, _random_spd, _solve_by_tasks


def _neager(P, D, pattern, allow_nd, ntask, tile=32):
    from se2lam_amd import capi
    pat = None if pattern is None else np.ascontiguousarray(pattern, np.uint8)
    ne = np.full(max(ntask, 1), -1, np.int32)
    capi.check(capi.lib().se2gpu_ba_debug_solve_plan_neager(P, D, None if pat is None else pat.ctypes.data, int(allow_nd), tile,
                                                             ne.ctypes.data, len(ne)))
    return ne[:ntask]


def _graph_pattern(g):
    """which pairs of key frames share a landmark or an odometry edge (what initialize hands to the chooser)"""
    P = g.P
    pat = np.eye(P, dtype=np.uint8)
    order = np.argsort(g.e_lm, kind="stable")
    lm, kf = g.e_lm[order], g.e_kf[order]
    ptr = np.searchsorted(lm, np.arange(g.L + 1))
    for l in range(g.L):
        k = kf[ptr[l]:ptr[l + 1]]
        pat[np.ix_(k, k)] = 1
    pat[g.o_i, g.o_j] = 1
    pat[g.o_j, g.o_i] = 1
    fx = np.asarray(g.fixed, bool)
    pat[fx, :] = 0
    pat[:, fx] = 0
    np.fill_diagonal(pat, 1)
    return pat


def _bench_pattern(P, L):
    from se2lam_amd import synth
    return _graph_pattern(synth.ba_graph(P, L))


PATTERNS = {
    "dense 40": (40, lambda: None),
    "ring 200 / 41": (200, lambda: _band(200, 41, True)),
    "ring 200 / 43": (200, lambda: _band(200, 43, True)),
    "ring 50 / 10": (50, lambda: _band(50, 10, True)),
    "open band 120 / 12": (120, lambda: _band(120, 12, False)),
    "open band 64 / 30": (64, lambda: _band(64, 30, False)),
    "bench graph 200 / 20000": (200, lambda: _bench_pattern(200, 20000)),
    "bench graph 50 / 5000": (50, lambda: _bench_pattern(50, 5000)),
}
RINGS = ("ring 200 / 41", "ring 200 / 43", "ring 50 / 10", "bench graph 200 / 20000", "bench graph 50 / 5000")
_cache = {}


def _case(name):
    """(P, pattern, plan, neager) of the chosen plan: built once, shared, never modified"""
    if name not in _cache:
        P, make = PATTERNS[name]
        pat = make()
        plan = _plan(P, 3, pat, True)
        _cache[name] = (P, pat, plan, _neager(P, 3, pat, True, len(plan["tasks"])))
    return _cache[name]


def _depths(plan):
    """depth of every block column, recomputed from the diagonal tasks' lists"""
    depth = np.zeros(plan["nbc"], int)
    for ti, j, d0, d1 in plan["tasks"]:
        if ti >> 16 == 0 and ti == j:
            ms = plan["deps"][d0:d1] & 0x7fff
            assert (ms < j).all()
            depth[j] = 1 + (depth[ms].max() if len(ms) else 0)
    assert (depth > 0).all() and depth.max() == plan["depth"]
    return depth


def _makespan(plan, deps):
    """Unit-cost schedule of the task graph: a task takes its entries in list order, an entry costs 1 once its tiles are
    published, the elimination costs 2; an x task has no elimination.  Every task has a workgroup of its own."""
    nsys, tasks = plan["nsys"], plan["tasks"]
    it = nsys // NB
    done = {}

    def published(kind, i, m):
        # R(m, m) and L(m, m) both come from the diagonal task
        return done[(0, m, m)] if i == m else done[(kind, i, m)]

    end = 0
    for ti, j, d0, d1 in tasks:
        kind, i = ti >> 16, ti & 0xffff
        t = 0
        for dep in deps[d0:d1]:
            m, has = int(dep) & 0x7fff, int(dep) >> 15
            if kind == 2:       # x(r): R(r, m) and y(m)
                ready = max(published(1, i, m), published(0, it, m))
            else:
                ready = published(0, j, m)
                if has:
                    ready = max(ready, published(kind, i, m))
            t = max(t, ready) + 1
        if kind != 2:
            t += 2
            done[(kind, i, j)] = t
        end = max(end, t)
    return end


def _sorted_by_column(plan):
    deps = plan["deps"].copy()
    for ti, j, d0, d1 in plan["tasks"]:
        seg = deps[d0:d1]
        deps[d0:d1] = seg[np.argsort(seg & 0x7fff, kind="stable")]
    return deps


@pytest.mark.parametrize("name", list(PATTERNS))
def test_lists_are_in_depth_order_and_neager_counts_the_deepest(name):
    P, pat, plan, ne = _case(name)
    depth = _depths(plan)
    permuted = plan["nsys"] != 3 * P
    assert len(ne) == len(plan["tasks"])
    for t, (ti, j, d0, d1) in enumerate(plan["tasks"]):
        kind = ti >> 16
        ms = plan["deps"][d0:d1] & 0x7fff
        if kind == 2:                                   # the x tasks keep their lists: ascending block columns, the last one eager
            assert (np.diff(ms) > 0).all() and ms[0] == (ti & 0xffff) and ne[t] == 1
            continue
        assert len(np.unique(ms)) == len(ms)
        if len(ms) == 0:
            assert j == 0 or depth[j] == 1
            assert ne[t] == 0
            continue
        d = depth[ms]
        assert (np.diff(d) >= 0).all(), (name, t, ms, d)
        for a in range(len(ms) - 1):                    # ties by ascending column
            assert d[a] < d[a + 1] or ms[a] < ms[a + 1]
        assert ne[t] == int((d == d.max()).sum()) >= 1
        assert d.max() == depth[j] - 1
        if not permuted:
            assert (np.diff(ms) > 0).all() and ne[t] == 1


@pytest.mark.parametrize("name", ["dense 40", "open band 64 / 30"])
def test_natural_order_plans_keep_their_ascending_lists(name):
    """depth = index + 1 where nothing is permuted: the lists are the ascending ones (bit-identical sums), one eager entry"""
    P, pat, plan, ne = _case(name)
    assert plan["nsys"] == 3 * P and plan["depth"] == plan["nbc"]
    assert np.array_equal(_depths(plan), 1 + np.arange(plan["nbc"]))
    assert np.array_equal(plan["deps"], _sorted_by_column(plan))
    for t, (ti, j, d0, d1) in enumerate(plan["tasks"]):
        if ti >> 16 != 2:
            ms = plan["deps"][d0:d1] & 0x7fff
            assert (np.diff(ms) > 0).all() and (j == 0 or ms[-1] == j - 1)
            if pat is None:
                assert np.array_equal(ms, np.arange(j))
            assert ne[t] == (1 if j > 0 else 0)


def test_first_separator_column_ends_with_the_last_columns_of_both_arcs():
    """ring 200 / 43 (the bench's shape): arcs = columns 0-4 and 5-9, separators 10-18"""
    P, pat, plan, ne = _case("ring 200 / 43")
    assert plan["nsys"] == 608 and plan["depth"] == 14
    depth = _depths(plan)
    assert list(depth[:10]) == [1, 2, 3, 4, 5] * 2 and depth[10] == 6
    seen = 0
    for t, (ti, j, d0, d1) in enumerate(plan["tasks"]):
        if ti >> 16 != 2 and j == 10:
            ms = list(plan["deps"][d0:d1] & 0x7fff)
            assert ms[-2:] == [4, 9] and ne[t] == 2, (t, ms, ne[t])
            assert ms == sorted(ms, key=lambda m: (depth[m], m))
            seen += 1
    assert seen >= 2
    # deeper separator columns wait for one column again
    assert all(ne[t] == 1 for t, (ti, j, d0, d1) in enumerate(plan["tasks"]) if ti >> 16 != 2 and j > 10)


@pytest.mark.parametrize("name", list(PATTERNS))
def test_depth_order_never_lengthens_the_schedule(name):
    P, pat, plan, ne = _case(name)
    new, old = _makespan(plan, plan["deps"]), _makespan(plan, _sorted_by_column(plan))
    print(f"{name}: makespan {new} in depth order, {old} in column order")
    assert new <= old
    if name in RINGS:
        assert plan["nsys"] != 3 * P, "expected a permuted plan"
        assert new < old


@pytest.mark.parametrize("name", list(PATTERNS))
def test_tile_tasks_in_depth_order_solve_the_system(name):
    """the numpy executor of tests/test_solve_plan.py takes the entries in list order, like the kernel"""
    P, pat, plan, ne = _case(name)
    rng = np.random.default_rng(P + 1)
    S = _random_spd(rng, P, 3, pat)
    b = rng.normal(size=3 * P)
    want = np.linalg.solve(S, b)
    got = _solve_by_tasks(plan, P, 3, S, b)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-11), (name, np.abs(got - want).max())
