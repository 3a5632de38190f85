"""k_reduce2's flat plan records (csrc/ba.hip: flat_record, k_plan_flat): a plan post-pass writes, per group slot,
the group descriptor, the block's system columns / PreEdgeSE2 edge / fixed flags and the chunk's first sixteen pair indices side
by side, so an off-diagonal workgroup of d_reduce2 goes record -> W -> store without the hops through pair_i / pair_j / blk_* /
o_i / o_j, and a block's PreEdgeSE2 term is finished in front of the W rounds.

Same products, same order of every sum: the reduced system and everything a run reports are compared BIT FOR BIT with the chain
through the old arrays (SE2GPU_BA_REDUCE_FLAT=0, read at initialize: a child process computes it, once per module), in the
graph-replayed form (this process) and in the synchronous form (SE2GPU_BA_SYNC=1, a second child).  The bounds against the
oracle are test_ba_gpu.py's and are not restated here.
"""
import os
import sys

import numpy as np
import pytest

import ba_ab
from ba_ab import assert_equal_runs, record
from ba_cases import bare_pose, dense_window, no_odometry, opt

GRP_PER_WG, CHUNK, FLAT_Q = 28, 16, 11   # csrc/ba.hip: kGrpPerWG, kChunk, kFlatQ
LAMBDA = 3.0e-2
SWITCHES = ("SE2GPU_BA_REDUCE_FLAT", "SE2GPU_BA_SYNC")


def _graphs(synth):
    """(name, graph): the smallest windows that reach every branch of the flat path
        tiny         8 key frames: one workgroup, every slot used, the blocks of the fixed key frame among them
        plain        30 key frames: several workgroups, blocks of several chunks, workgroups whose last slots are padding
        dense        blocks of 500 pairs: chunks longer than sixteen pairs; an edge that runs b -> a
        long         PreEdgeSE2 edges between key frames that share no landmark: blocks with an edge and no pairs
        hub12        twelve PreEdgeSE2 edges at one key frame: the serial tail behind the eight parallel lanes
        fixed_ends   fixed key frames inside blocks and at either / both ends of PreEdgeSE2 edges
        no_odometry  O = 0
        bare_pose    a key frame without observation edges
        ring50       50 key frames: the solver takes its fill-reducing order (pose_off)"""
    g30 = synth.ba_graph(30, 2000)
    return [("tiny", synth.ba_graph(8, 60)), ("plain", g30), ("dense", dense_window(synth)),
            ("long", synth.odometry_topology(g30, "long", seed=1)),
            ("hub12", synth.odometry_topology(synth.ba_graph(21, 800), "hub12", seed=1)),
            ("fixed_ends", synth.odometry_topology(g30, "fixed_ends", seed=1)),
            ("no_odometry", no_odometry(synth)), ("bare_pose", bare_pose(synth)), ("ring50", synth.ba_graph(50, 5000))]


BATCH = ("tiny", "hub12", "fixed_ends")   # the lock-step batch: three distinct small windows
EXEMPT = ("/nslots",)                     # what the two sides differ in by design


def _nslots(o):
    """group slots of the handle's flat records; 0: the handle runs without them"""
    import ctypes as C
    from se2lam_amd import capi
    n = C.c_int(-1)
    capi.check(capi.lib().se2gpu_ba_debug_flat_records(o._h, None, None, 0, C.byref(n)))
    return n.value


def _readback(o):
    """(group descriptors, records) of an initialised handle"""
    import ctypes as C
    from se2lam_amd import capi
    n = C.c_int(_nslots(o))
    grp, flat = np.zeros((n.value, 4), np.int32), np.zeros((n.value, FLAT_Q, 4), np.int32)
    capi.check(capi.lib().se2gpu_ba_debug_flat_records(o._h, grp.ctypes.data, flat.ctypes.data, n.value, C.byref(n)))
    return grp, flat


EMPTY_TAIL = np.array([0, 0, -1, 0] + [0] * (4 * (FLAT_Q - 2)), np.int32).reshape(FLAT_Q - 1, 4)   # words 1 .. 10 of an unused slot


def _scenarios(synth, out):
    """per graph: the reduced system of the start; optimize(10) and optimize(3), each three times from the start on a handle of its
    own (the third run of a shape is the replayed graph).  Then the three windows of BATCH in one lock-step batch."""
    from se2lam_amd import capi
    from se2lam_amd.optimizer import optimize_batch
    graphs = _graphs(synth)
    for name, g in graphs:
        o = opt(g)
        ba_ab.system(o, out, name, LAMBDA)
        nsys, permuted, _ = o.plan_neager()
        out[name + "/permuted"] = np.asarray([int(permuted)], np.int64)
        out[name + "/nslots"] = np.asarray([_nslots(o)], np.int64)
        for n in (10, 3):
            o = opt(g)
            for _ in range(3):
                o.reset_estimates()
                o.optimize(n)
            record(o, out, "%s/n%d" % (name, n))
    by_name = dict(graphs)
    opts = [opt(by_name[k]) for k in BATCH]
    optimize_batch(opts, 10)
    out["batch/path"] = np.asarray([int(capi.lib().se2gpu_ba_last_batch_path())], np.int64)
    for k, o in zip(BATCH, opts):
        record(o, out, "batch/" + k)


@pytest.fixture(scope="module")
def runs(synth, tmp_path_factory):
    """the scenarios with the flat records (this process), without them, and with them in the synchronous form"""
    assert os.environ.get("SE2GPU_BA_REDUCE_FLAT", "1") != "0" and os.environ.get("SE2GPU_BA_SYNC", "0") != "1"
    new = {}
    _scenarios(synth, new)
    tmp = tmp_path_factory.mktemp("reduce_flat")
    old = ba_ab.child(__file__, tmp, "old", unset=SWITCHES, env_set={"SE2GPU_BA_REDUCE_FLAT": "0"})
    sync = ba_ab.child(__file__, tmp, "sync", unset=SWITCHES, env_set={"SE2GPU_BA_SYNC": "1"})
    return new, old, sync


@pytest.mark.gpu
def test_the_graphs_reach_the_branches(runs, synth):
    """what each window is there for, asserted on the window: the solver's permuted order (as plan_neager reports it), the
    records in use / not in use, blocks with an edge and no pairs, the serial tail, fixed ends"""
    new, old, sync = runs
    g = dict(_graphs(synth))
    # SE2GPU_BA_REDUCE_FLAT=0 was honoured: the child it was set for built no records, this process and the synchronous child did
    for name in g:
        assert old[name + "/nslots"][0] == 0, name
        assert new[name + "/nslots"][0] > 0 and new[name + "/nslots"][0] % GRP_PER_WG == 0, name
        assert sync[name + "/nslots"][0] == new[name + "/nslots"][0], name
    assert new["tiny/nslots"][0] == GRP_PER_WG and new["plain/nslots"][0] > 2 * GRP_PER_WG
    assert new["ring50/permuted"][0] == 1 and old["ring50/permuted"][0] == 1
    assert all(new[k + "/permuted"][0] == 0 for k in ("tiny", "plain", "dense", "hub12"))
    cov = synth.covisible(g["long"])
    assert any(not cov[i, j] for i, j in zip(g["long"].o_i, g["long"].o_j))
    assert np.bincount(np.concatenate([g["hub12"].o_i, g["hub12"].o_j])).max() == 12
    fe = g["fixed_ends"]
    ends = {(int(fe.fixed[i]), int(fe.fixed[j])) for i, j in zip(fe.o_i, fe.o_j)}
    assert ends == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert g["no_odometry"].o_i.size == 0
    assert new["batch/path"][0] != 2 and old["batch/path"][0] != 2   # the lock-step batch, not the resident kernel
    # tiny: ONE workgroup, all 28 slots taken by the 28 blocks of 8 key frames (those of the fixed one: not free, no pairs);
    # plain: several workgroups, in each the used slots first and the padding behind them, and some do end in padding
    for name in ("tiny", "plain"):
        grp, flat = _readback(opt(g[name]))
        assert np.array_equal(flat[:, 0], grp)
        used = grp[:, 0] >= 0
        per_wg = used.reshape(-1, GRP_PER_WG)
        assert all(not row[int(row.sum()):].any() for row in per_wg), name
        assert (flat[~used, 1:] == EMPTY_TAIL).all(), name
        first = flat[used][:, 3:, :]   # a used slot's indices: clamped to the chunk's last pair, never past it
        assert (grp[used, 2] - grp[used, 1] <= CHUNK).all() and (first >= 0).all(), name
        if name == "tiny":
            assert used.all() and (flat[:, 1, 3] == 0).sum() == g[name].P - 1
        else:
            assert (per_wg.sum(axis=1) < GRP_PER_WG).any() and per_wg[-1].any()
    # dense: whole workgroups of 28 slots
    grp, flat = _readback(opt(g["dense"]))
    assert np.array_equal(flat[:, 0], grp)
    used = grp[:, 0] >= 0
    # three blocks of 500 pairs in 28 chunks each: 27 of 18 pairs - longer than the sixteen a record holds - and one of 14
    assert ((grp[used, 2] - grp[used, 1]) > CHUNK).sum() == 3 * (GRP_PER_WG - 1)
    assert (flat[~used, 1:] == EMPTY_TAIL).all()


@pytest.mark.gpu
def test_reduced_system_and_runs_equal_the_old_chain(runs):
    """S and bs of every window, then chi2_hist, lambda_hist, trials_hist, poses and landmarks of optimize(10) and optimize(3)
    (replayed) and of the lock-step batch: equal to the bit"""
    new, old, _ = runs
    assert sum(1 for k in new if k.endswith("/S")) == 9
    assert sum(1 for k in new if k.endswith("/trials")) == 9 * 2 + len(BATCH)
    assert_equal_runs(new, old, exempt_suffix=EXEMPT)


@pytest.mark.gpu
def test_synchronous_form_equals_the_old_chain(runs):
    """SE2GPU_BA_SYNC=1 with the records: the same bits again"""
    _, old, sync = runs
    assert_equal_runs(sync, old, exempt_suffix=EXEMPT, skip=("batch/path",))   # (a synchronous process runs the windows of a batch one by one)


# ---- the record builder against a model of it: host code, no device
def _model_record(d, blk_a, blk_b, blk_odo, pair_i, pair_j, fixed, pose_off, o_i, o_j):
    rec = np.zeros((FLAT_Q, 4), np.int32)
    rec[0] = d
    rec[1, 2] = -1
    if d[0] < 0:
        return rec
    a, b, od = blk_a[d[0]], blk_b[d[0]], blk_odo[d[0]]
    col = (lambda p: pose_off[p]) if pose_off is not None else (lambda p: 3 * p)
    rec[1] = [col(a), col(b), od, int(not fixed[a] and not fixed[b])]
    if od >= 0:
        rec[2, :2] = [o_i[od >> 1], o_j[od >> 1]]
    for t in range(8):
        if d[2] > d[1]:
            q0, q1 = min(d[1] + t, d[2] - 1), min(d[1] + 8 + t, d[2] - 1)
            rec[3 + t] = [pair_i[q0], pair_j[q0], pair_i[q1], pair_j[q1]]
    return rec


@pytest.mark.parametrize("permuted", [False, True])
def test_record_builder_equals_its_model(permuted):
    """group descriptor + block table + pair arrays -> record: empty slots, blocks without pairs (an edge only), chunks of 1, 8, 9,
    15, 16 and more than 16 pairs, edges in both directions, fixed poses, natural and permuted columns"""
    from se2lam_amd import capi
    rng = np.random.default_rng(11 + permuted)
    P, O = 9, 7
    nblk = P * (P + 1) // 2
    blk_a, blk_b = rng.integers(0, P, nblk).astype(np.int32), rng.integers(0, P, nblk).astype(np.int32)
    o_i, o_j = rng.integers(0, P, O).astype(np.int32), rng.integers(0, P, O).astype(np.int32)
    blk_odo = np.where(rng.random(nblk) < 0.4, rng.integers(0, 2 * O, nblk), -1).astype(np.int32)
    fixed = (rng.random(P) < 0.3).astype(np.uint8)
    pose_off = (32 * rng.permutation(P) + 3 * rng.integers(0, 5, P)).astype(np.int32) if permuted else None
    sizes = [0, 1, 8, 9, 15, 16, 17, 40, 0, 16, 3]
    npair = sum(sizes)
    pair_i, pair_j = rng.integers(0, 1000, npair).astype(np.int32), rng.integers(0, 1000, npair).astype(np.int32)
    grp, q = [], 0
    for s, n in enumerate(sizes):
        grp.append([int(rng.integers(0, nblk)), q, q + n, (s % GRP_PER_WG) | (1 << 8)])
        q += n
        if s % 3 == 2:
            grp.append([-1, 0, 0, 0])
    grp = np.asarray(grp, np.int32)
    flat = np.full((len(grp), FLAT_Q, 4), 12345, np.int32)
    capi.check(capi.lib().se2gpu_ba_debug_flat_records_host(
        len(grp), grp.ctypes.data, blk_a.ctypes.data, blk_b.ctypes.data, blk_odo.ctypes.data, pair_i.ctypes.data, pair_j.ctypes.data,
        fixed.ctypes.data, None if pose_off is None else pose_off.ctypes.data, o_i.ctypes.data, o_j.ctypes.data, flat.ctypes.data))
    want = np.stack([_model_record(d, blk_a, blk_b, blk_odo, pair_i, pair_j, fixed, pose_off, o_i, o_j) for d in grp])
    assert np.array_equal(flat, want)
    assert (blk_odo[grp[grp[:, 0] >= 0, 0]] >= 0).any() and (fixed[blk_a[grp[grp[:, 0] >= 0, 0]]] == 1).any()


if __name__ == "__main__":
    ba_ab.child_main(_scenarios, sys.argv[1:])
