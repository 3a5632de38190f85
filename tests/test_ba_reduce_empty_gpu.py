"""k_reduce2 without the workgroups of the empty Schur blocks (csrc/ba.hip: pack_takes, reduce2_split).

An off-diagonal block of the reduced system with no contributor pair and no PreEdgeSE2 edge does no arithmetic: its group stores
eighteen zeros into S on every trial.  The plan packs those blocks BEHIND all others (block order kept inside either class, one
stream, per-block chunking untouched), `initialize` clears S once, and a handle whose S keeps the zeros launches only the
nwg_real workgroups in front of them.  Handles that write into S elsewhere (k_chol_step, an all-reduce) launch the tail as well.

Every sum keeps its order: the reduced system and everything a run reports are compared BIT FOR BIT with block-order packing and
the full grid (SE2GPU_BA_REDUCE_EMPTY=0, read at initialize: a child process, once per module), replayed (this process) and
synchronous (SE2GPU_BA_SYNC=1, a second child).  SE2GPU_BA_CHOL and SE2GPU_BA_PLAN are read at every initialize too: those
variants run inside each of the three processes.  The bounds against the oracle are test_ba_gpu.py's and are not restated here.

The windows (the smallest that reach a branch):
    tiny       ba_graph(8, 60): one mixed workgroup, nwg_real == nwg_all == 1
    thin       ba_graph(30, 2000) keeping only the edges whose key frame lies within 2 of the landmark's first key frame (and the
               landmarks that keep two edges: 172 of the 2,000 would keep one): most blocks empty, whole tail workgroups, three
               block columns in the solve
    thin_long  thin with PreEdgeSE2 edges between key frames that share no landmark: blocks with an edge and no pairs are real
    dense      ba_cases.dense_window, all key frames sharing all landmarks: nwg_real == nwg_all
    ring50     ba_graph(50, 5000): the permuted plan (pose_off); 727 of 1,225 blocks empty
"""
import dataclasses
import os
import sys

import numpy as np
import pytest

import ba_ab
from ba_ab import assert_equal_runs, record, same_bits
from ba_cases import dense_window, env, opt, thin, thin4

GRP_PER_WG, CHUNK = 28, 16   # csrc/ba.hip: kGrpPerWG, kChunk
LAMBDA = 3.0e-2
SWITCHES = ("SE2GPU_BA_REDUCE_EMPTY", "SE2GPU_BA_SYNC", "SE2GPU_BA_CHOL", "SE2GPU_BA_PLAN")


def _grid(o):
    """se2gpu_ba_debug_reduce_grid: (nwg_all, nwg_real, off-diagonal workgroups the next reduction launches)"""
    from se2lam_amd import capi
    out = np.zeros(3, np.int32)
    capi.check(capi.lib().se2gpu_ba_debug_reduce_grid(o._h, out.ctypes.data))
    return [int(v) for v in out]


def _graphs(synth):
    t = thin(synth)
    return [("tiny", synth.ba_graph(8, 60)), ("thin", t), ("thin_long", synth.odometry_topology(t, "long", seed=1)),
            ("dense", dense_window(synth)), ("ring50", synth.ba_graph(50, 5000))]


BATCH = ("tiny", "thin", "thin_long")
EXEMPT = ("/grid",)   # what the two sides differ in by design


def _system(o, out, key):
    ba_ab.system(o, out, key, LAMBDA)


def _scenarios(synth, out):
    from se2lam_amd import capi
    from se2lam_amd.optimizer import SlamOptimizer, optimize_batch
    graphs = _graphs(synth)
    by_name = dict(graphs)
    for name, g in graphs:
        o = opt(g)
        out[name + "/grid"] = np.asarray(_grid(o), np.int64)
        _system(o, out, name)
        out[name + "/permuted"] = np.asarray([int(o.plan_neager()[1])], np.int64)
        for n in (10, 3):   # (the third run of a shape is the replayed graph)
            o = opt(g)
            for _ in range(3):
                o.reset_estimates()
                o.optimize(n)
            record(o, out, "%s/n%d" % (name, n))
    opts = [opt(by_name[k]) for k in BATCH]
    optimize_batch(opts, 10)
    out["batch/path"] = np.asarray([int(capi.lib().se2gpu_ba_last_batch_path())], np.int64)
    for k, o in zip(BATCH, opts):
        record(o, out, "batch/" + k)
    # reload: a handle that held a window with more non-zero blocks, optimised, cleared, loaded with a thin window of the same P
    for key, before, after in (("reload4", by_name["dense"], thin4(synth)), ("reload30", synth.ba_graph(30, 2000), by_name["thin"])):
        assert before.P == after.P
        o = opt(before)
        o.optimize(10)
        o.clear()
        o.load(after)
        o.initializeOptimization(0)
        out[key + "/grid"] = np.asarray(_grid(o), np.int64)
        _system(o, out, key)
        _system(opt(after), out, key + "_fresh")
    # the in-place factorisation writes into the empty blocks: optimize(10) twice, then the reduced system
    with env(SE2GPU_BA_CHOL="steps"):
        o = opt(by_name["thin"])
        out["steps/path"] = np.asarray([o.solver_path()], np.int64)
        out["steps/grid"] = np.asarray(_grid(o), np.int64)
        for _ in range(2):
            o.optimize(10)
        record(o, out, "steps/n10")
        _system(o, out, "steps")
    # the host builder of the plan: the device kernels' mirror
    with env(SE2GPU_BA_PLAN="host"):
        for name in ("thin", "ring50"):
            o = opt(by_name[name])
            out["host_%s/grid" % name] = np.asarray(_grid(o), np.int64)
            _system(o, out, "host_" + name)
            o.optimize(10)
            record(o, out, "host_%s/n10" % name)
    # a handle with an all-reduce set (world 1: the callback has nothing to add) keeps block order and the full grid
    o = SlamOptimizer()
    o.set_allreduce(lambda ptr, count, stream: None)
    o.load(by_name["thin"])
    o.initializeOptimization(0)
    out["sharded/grid"] = np.asarray(_grid(o), np.int64)
    _system(o, out, "sharded")


@pytest.fixture(scope="module")
def runs(synth, tmp_path_factory):
    """the scenarios with the empty blocks packed last (this process), in block order with the full grid, and synchronous"""
    assert os.environ.get("SE2GPU_BA_REDUCE_EMPTY", "1") != "0" and os.environ.get("SE2GPU_BA_SYNC", "0") != "1"
    assert "SE2GPU_BA_CHOL" not in os.environ and "SE2GPU_BA_PLAN" not in os.environ
    new = {}
    _scenarios(synth, new)
    tmp = tmp_path_factory.mktemp("reduce_empty")
    old = ba_ab.child(__file__, tmp, "old", unset=SWITCHES, env_set={"SE2GPU_BA_REDUCE_EMPTY": "0"})
    sync = ba_ab.child(__file__, tmp, "sync", unset=SWITCHES, env_set={"SE2GPU_BA_SYNC": "1"})
    return new, old, sync


@pytest.mark.gpu
def test_the_windows_reach_the_branches(runs, synth):
    """what each window is there for, asserted on the window and on the grids the debug entry reports"""
    new, old, sync = runs
    g = dict(_graphs(synth))
    thin = g["thin"]
    assert np.bincount(thin.e_lm, minlength=thin.L).min() >= 2 and (np.diff(thin.e_lm) >= 0).all()
    cov = synth.covisible(thin)
    off = ~np.eye(thin.P, dtype=bool)
    assert cov[off].mean() < 0.25                                            # most blocks are empty
    assert 3 * thin.P > 2 * 32                                               # three block columns of 32 in the solve
    cl = synth.covisible(g["thin_long"])
    assert any(not cl[i, j] for i, j in zip(g["thin_long"].o_i, g["thin_long"].o_j))   # an edge and no pairs
    # SE2GPU_BA_REDUCE_EMPTY=0 was honoured: block order, everything launched
    for name in g:
        a, r, launched = new[name + "/grid"]
        assert 0 < r <= a and launched == r, (name, new[name + "/grid"])
        assert list(sync[name + "/grid"]) == [a, r, r], name
        oa, orl, ol = old[name + "/grid"]
        assert oa == orl == ol and ol >= r, (name, old[name + "/grid"])
    assert list(new["tiny/grid"]) == [1, 1, 1]
    assert new["thin/grid"][1] < new["thin/grid"][0] and new["thin_long/grid"][1] < new["thin_long/grid"][0]   # whole tail workgroups
    assert new["thin_long/grid"][1] >= new["thin/grid"][1]
    assert new["dense/grid"][1] == new["dense/grid"][0]                       # no block empty
    assert new["ring50/permuted"][0] == 1 and old["ring50/permuted"][0] == 1 and new["ring50/grid"][1] < new["ring50/grid"][0]
    assert all(new[k + "/permuted"][0] == 0 for k in ("tiny", "thin", "thin_long", "dense"))
    assert new["batch/path"][0] != 2 and old["batch/path"][0] != 2            # the lock-step batch, not the resident kernel
    # the in-place factorisation: the full grid there, nwg_real without it
    assert new["steps/path"][0] == 1 and old["steps/path"][0] == 1
    a, r, launched = new["steps/grid"]
    assert launched == a and [a, r] == list(new["thin/grid"][:2]) and r < a
    # the host builder reports the device kernels' counts
    for name in ("thin", "ring50"):
        assert list(new["host_%s/grid" % name]) == list(new[name + "/grid"]), name
    # an all-reduce is set: block order, the full grid (beyond that, sharded handles are untested here: world > 1 runs in
    # test_ba_gpu.py, on plans in block order)
    a, r, launched = new["sharded/grid"]
    assert a == r == launched == old["thin/grid"][0]
    # the reload cases do skip workgroups
    assert new["reload30/grid"][2] < new["reload30/grid"][0] and list(new["reload30/grid"]) == list(new["thin/grid"])


@pytest.mark.gpu
def test_reduced_system_and_runs_equal_block_order(runs):
    """S and bs of every window, chi2_hist, lambda_hist, trials_hist, poses and landmarks of optimize(10) and optimize(3)
    (replayed), the lock-step batch, the in-place solver, the host plan: equal to the bit"""
    new, old, _ = runs
    assert sum(1 for k in new if k.endswith("/S")) == 5 + 4 + 1 + 2 + 1
    assert sum(1 for k in new if k.endswith("/trials")) == 5 * 2 + len(BATCH) + 1 + 2
    assert_equal_runs(new, old, exempt_suffix=EXEMPT)


@pytest.mark.gpu
def test_synchronous_form_equals_block_order(runs):
    """SE2GPU_BA_SYNC=1 with the empty blocks packed last: the same bits again"""
    _, old, sync = runs
    assert_equal_runs(sync, old, exempt_suffix=EXEMPT, skip=("batch/path",))   # (a synchronous process runs the windows of a batch one by one)


@pytest.mark.gpu
def test_reloaded_handle_equals_a_fresh_one(runs):
    """a handle that held other non-zero blocks: `initialize` cleared them, S equals a fresh handle's to the bit; and the host
    plan's and the device plan's systems are the same bits"""
    new, _, sync = runs
    for r in (new, sync):
        for key in ("reload4", "reload30"):
            assert same_bits(r[key + "/S"], r[key + "_fresh/S"]) and same_bits(r[key + "/bs"], r[key + "_fresh/bs"]), key
        for name in ("thin", "ring50"):
            assert same_bits(r["host_%s/S" % name], r[name + "/S"]) and same_bits(r["host_%s/bs" % name], r[name + "/bs"]), name
        assert same_bits(r["sharded/S"], r["thin/S"])


def _descriptors(o):
    """the group descriptors of an initialised handle (se2gpu_ba_debug_flat_records)"""
    import ctypes as C
    from se2lam_amd import capi
    n = C.c_int(-1)
    capi.check(capi.lib().se2gpu_ba_debug_flat_records(o._h, None, None, 0, C.byref(n)))
    grp, flat = np.zeros((n.value, 4), np.int32), np.zeros((n.value, 11, 4), np.int32)
    capi.check(capi.lib().se2gpu_ba_debug_flat_records(o._h, grp.ctypes.data, flat.ctypes.data, n.value, C.byref(n)))
    return grp


@pytest.mark.gpu
def test_device_packers_equal_the_host_builder(synth):
    """the group descriptors of the device plan are the host builder's, element for element, in the new order: k_plan_tab /
    k_plan_tabscan / k_plan_place (up to 96 K blocks) and k_plan_pack (450 key frames: 101,475 blocks)"""
    assert os.environ.get("SE2GPU_BA_REDUCE_EMPTY", "1") != "0" and "SE2GPU_BA_PLAN" not in os.environ
    for g in (thin(synth), synth.ba_graph(50, 5000), synth.ba_graph(450, 1500)):
        assert g.P != 450 or g.P * (g.P + 1) // 2 > 96 * 1024
        dev = opt(g)
        with env(SE2GPU_BA_PLAN="host"):
            host = opt(g)
        assert _grid(dev) == _grid(host) and _grid(dev)[1] < _grid(dev)[0], g.P
        a, b = _descriptors(dev), _descriptors(host)
        assert a.shape == b.shape and np.array_equal(a, b), g.P
        want, nwg, real = _host_pack(g, True)
        assert np.array_equal(a, want) and _grid(dev)[:2] == [nwg, real], g.P


# ---- the host builder's packing against a model of it: host code, no device
def _blk_index(P, a, b):
    return a * P - a * (a - 1) // 2 + (b - a)


def _block_tables(g):
    """(contributor pairs per block, non-empty flag per block) of the upper triangle.  Pairs are those of two FREE key frames
    that see a landmark; a block is non-empty when its key frames - fixed or not - share a landmark or a PreEdgeSE2 edge (a block
    that is zero only because a key frame is fixed stays with the others)"""
    P = g.P
    cnt = np.zeros(P * (P + 1) // 2, np.int64)
    nz = np.zeros(P * (P + 1) // 2, bool)
    ptr = np.searchsorted(g.e_lm, np.arange(g.L + 1))
    free = g.fixed == 0
    for l in range(g.L):
        kfs = g.e_kf[ptr[l]:ptr[l + 1]]
        a, b = np.meshgrid(kfs, kfs, indexing="ij")
        m = np.triu(np.ones(a.shape, bool), 1) & (a != b)
        lo, hi = np.minimum(a[m], b[m]), np.maximum(a[m], b[m])
        q = lo * P - lo * (lo - 1) // 2 + (hi - lo)
        nz[q] = True
        np.add.at(cnt, q[free[lo] & free[hi]], 1)
    for i, j in zip(g.o_i, g.o_j):
        nz[_blk_index(P, min(i, j), max(i, j))] = True
    return cnt, nz


def _model_pack(P, cnt, nz, empty_last):
    """first fit in order, 28 groups per workgroup, chunks of 16: [(block, first pair, last pair, first | ng << 8) or None] per
    slot, the number of workgroups and of those that hold a group of a non-empty block"""
    slots, used, real = [], 0, None
    ptr = np.concatenate([[0], np.cumsum(cnt)])

    def flush():
        nonlocal used
        while len(slots) % GRP_PER_WG:
            slots.append(None)
        used = 0

    for cls in ((0, 1) if empty_last else (0,)):
        for a in range(P):
            for b in range(a + 1, P):
                kb = _blk_index(P, a, b)
                if empty_last and bool(nz[kb]) != (cls == 0):
                    continue
                n, chunk = int(cnt[kb]), CHUNK
                ng = max(1, -(-n // chunk))
                if ng > GRP_PER_WG:
                    chunk = -(-n // GRP_PER_WG)
                    ng = -(-n // chunk)
                if used + ng > GRP_PER_WG:
                    flush()
                first = used
                for t in range(ng):
                    a0 = int(ptr[kb]) + t * chunk
                    a1 = min(int(ptr[kb + 1]), a0 + chunk)
                    slots.append((kb, a0, max(a0, a1), first | (ng << 8)))
                used = (used + ng) % GRP_PER_WG
        if cls == 0:
            real = -(-len(slots) // GRP_PER_WG)
    flush()
    nwg = len(slots) // GRP_PER_WG
    return slots, nwg, (real if empty_last else nwg)


def _host_pack(g, empty_last, odo_ok=1):
    from se2lam_amd import capi
    out = np.zeros(3, np.int32)
    a = [np.ascontiguousarray(g.e_kf, np.int32), np.ascontiguousarray(g.e_lm, np.int32), np.ascontiguousarray(g.fixed, np.uint8),
         np.ascontiguousarray(g.o_i, np.int32), np.ascontiguousarray(g.o_j, np.int32)]
    call = lambda grp, cap: capi.check(capi.lib().se2gpu_ba_debug_plan_host(
        g.P, g.L, g.E, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, g.O, a[3].ctypes.data, a[4].ctypes.data, odo_ok,
        int(empty_last), grp, cap, out.ctypes.data))
    call(None, 0)
    grp = np.zeros((int(out[0]), 4), np.int32)
    call(grp.ctypes.data, len(grp))
    return grp, int(out[1]), int(out[2])


def _check_packing(g, empty_last, odo_ok=1):
    cnt, nz = _block_tables(g)
    grp, nwg, real = _host_pack(g, empty_last, odo_ok)
    slots, m_nwg, m_real = _model_pack(g.P, cnt, nz, empty_last)
    assert (nwg, real) == (m_nwg, m_real) and len(grp) == nwg * GRP_PER_WG
    want = np.array([s if s is not None else (-1, 0, 0, 0) for s in slots], np.int32)
    assert np.array_equal(grp, want)
    # ... and the properties, on the builder's output itself
    used = grp[:, 0] >= 0
    per_wg = used.reshape(-1, GRP_PER_WG)
    assert all(not row[int(row.sum()):].any() for row in per_wg)                 # used slots come before padding
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    where = np.nonzero(used)[0]
    seen = {}
    for s in where:
        seen.setdefault(int(grp[s, 0]), []).append(int(s))
    off = [_blk_index(g.P, a, b) for a in range(g.P) for b in range(a + 1, g.P)]
    assert sorted(seen) == sorted(off)                                            # every off-diagonal block, no diagonal one
    for kb, ss in seen.items():
        assert ss == list(range(ss[0], ss[0] + len(ss))) and ss[0] // GRP_PER_WG == ss[-1] // GRP_PER_WG   # consecutive, one workgroup
        assert (grp[ss, 3] == ((ss[0] % GRP_PER_WG) | (len(ss) << 8))).all()
        assert grp[ss[0], 1] == ptr[kb] and max(grp[ss[-1], 2], ptr[kb]) == ptr[kb + 1]          # exactly its chunks
        assert (grp[ss[1:], 1] == grp[ss[:-1], 2]).all() and (grp[ss, 2] >= grp[ss, 1]).all()
        assert len(ss) == max(1, -(-int(cnt[kb]) // CHUNK)) or cnt[kb] > GRP_PER_WG * CHUNK
    if empty_last:
        e = ~nz[grp[where, 0]]
        assert not e[:int((~e).sum())].any()                                      # no non-empty block behind an empty one
        last_real = where[~e][-1] if (~e).any() else -1
        assert real == (last_real // GRP_PER_WG + 1 if last_real >= 0 else 0)
    else:
        assert (np.diff(grp[where, 0]) >= 0).all() and real == nwg
    return nwg, real, int((~nz[off]).sum()), len(off)


def test_host_packing_equals_its_model(synth):
    """ba_plan_host through se2gpu_ba_debug_plan_host against the model above, in both orders"""
    t = thin(synth)
    for g in (synth.ba_graph(8, 60), t, synth.odometry_topology(t, "long", seed=1), thin4(synth), dense_window(synth)):
        for empty_last in (False, True):
            _check_packing(g, empty_last)
    # PreEdgeSE2 edges outside the block plan (odo_ok = 0) still make their blocks non-empty
    assert _check_packing(synth.odometry_topology(t, "long", seed=1), True, odo_ok=0)[:2] == \
        _check_packing(synth.odometry_topology(t, "long", seed=1), True)[:2]
    nwg, real, empty, nblk = _check_packing(synth.ba_graph(50, 5000), True)
    assert (empty, nblk) == (727, 1225) and real < nwg


def test_host_packing_of_the_headline_window(synth):
    """200 key frames / 20,000 landmarks: 11,711 of the 19,900 off-diagonal blocks are empty; the workgroups of the others fit
    the device in one round with the diagonal part (1,280 workgroups are resident at 5 waves per SIMD)"""
    g = synth.ba_graph(200, 20000)
    nwg, real, empty, nblk = _check_packing(g, True)
    assert (empty, nblk) == (11711, 19900)
    assert (real, nwg) == (974, 1392)
    assert ((g.P + 1 + 7) & ~7) + ((real + 7) & ~7) <= 1280
    assert _check_packing(g, False)[0] == 1395                    # block order: what the device plan reports
    # a model that also counts the pairs of the fixed key frame 0 - the plan drops them, its 81 blocks with a shared landmark have one group each - gives
    # 1,409 workgroups in block order and 987 for the non-empty blocks: the difference to the device's 1,395
    free = dataclasses.replace(g, fixed=np.zeros_like(g.fixed))
    cnt, nz = _block_tables(free)
    assert _model_pack(g.P, cnt, nz, False)[1] == 1409 and _model_pack(g.P, cnt, nz, True)[2] == 987



if __name__ == "__main__":
    ba_ab.child_main(_scenarios, sys.argv[1:])
