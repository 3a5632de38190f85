"""The opening of an un-sharded SE(2) optimize(): k_open evaluates the starting state inside the first linearisation pass (one
edge pass where k_update<false> and k_linearize made two), carries the PreEdgeSE2 blocks in the same launch, and k_lambda0<true>
gathers the pose diagonals with its loads in flight (csrc/ba.hip).

The new opening runs the same expressions on the same inputs in the same order of summation, so everything a run reports is
compared BIT FOR BIT with the old opening's (SE2GPU_BA_OPEN=0, read once per process: a child process computes it, once per
module), in the graph-replayed form (this process) and in the synchronous form (SE2GPU_BA_SYNC=1, a second child), and with the
CPU oracle under the bounds of test_ba_gpu.py.
"""
import os
import sys

import numpy as np
import pytest

import ba_ab
from ba_ab import assert_equal_runs, same_bits
from ba_cases import LM_REJECT_CASES, REL, bare_pose, kidnapped, no_odometry, opt, pose_update_close

pytestmark = pytest.mark.gpu

# poses with fewer than 64 edges (a lane of k_lambda0 has zero or one); ~400 edges per pose (one partial batch of eight rounds);
# ~600 edges per pose (one full batch and a remainder)
PLAIN = [(8, 60), (30, 2000), (50, 5000)]
LM, GN = 0, 1
BARE_POSE = 2   # the key frame of ba_graph(30, 2000) whose observation edges are taken away


def _graphs(synth):
    """(name, graph): the three plain windows, the kidnapped starts that reject trials, O = 0, a pose without observations"""
    out = [("plain%d" % i, synth.ba_graph(P, L)) for i, (P, L) in enumerate(PLAIN)]
    out += [("reject%d" % i, kidnapped(synth, *c[0])) for i, c in enumerate(LM_REJECT_CASES)]
    out += [("no_odometry", no_odometry(synth)), ("bare_pose", bare_pose(synth, BARE_POSE))]
    return out


SWITCHES = ("SE2GPU_BA_OPEN", "SE2GPU_BA_SYNC")


def _record(o, out, key):
    ba_ab.record(o, out, key, counts=2)


def _scenarios(synth, out):
    """every graph x {LM, GN} x {optimize(10); optimize(1); optimize(3) twice without a reset}, each on a handle of its own; a stop
    flag that is up before the run, and the run after it"""
    for name, g in _graphs(synth):
        for mode in (LM, GN):
            for sc, calls in (("a", [10]), ("b", [1]), ("c", [3, 3])):
                o = opt(g)
                for ci, n in enumerate(calls):
                    o.optimize(n, mode)
                    _record(o, out, "%s/m%d/%s%d" % (name, mode, sc, ci))
    for mode in (LM, GN):
        g = synth.ba_graph(30, 2000)
        o = opt(g)
        flag = np.ones(1, np.uint8)
        o.setForceStopFlag(flag)
        assert o.optimize(10, mode) == 0 and o.stats["stopped"]
        _record(o, out, "stop/m%d/before" % mode)
        flag[0] = 0
        assert o.optimize(4, mode) == 4
        _record(o, out, "stop/m%d/after" % mode)


@pytest.fixture(scope="module")
def runs(synth, tmp_path_factory):
    """the scenarios by the new opening (this process: graph-replayed form), by the old one and by the new one's synchronous form"""
    assert os.environ.get("SE2GPU_BA_OPEN", "1") != "0" and os.environ.get("SE2GPU_BA_SYNC", "0") != "1"
    new = {}
    _scenarios(synth, new)
    tmp = tmp_path_factory.mktemp("opening")
    old = ba_ab.child(__file__, tmp, "old", unset=SWITCHES, env_set={"SE2GPU_BA_OPEN": "0"})
    sync = ba_ab.child(__file__, tmp, "sync", unset=SWITCHES, env_set={"SE2GPU_BA_SYNC": "1"})
    return new, old, sync


def test_same_results_as_the_old_opening(runs):
    """chi2_init, chi2_hist, lambda_hist, trials_hist, poses, landmarks and the linearisation counters, LM and GN, optimize(10) /
    optimize(1) / optimize(3) twice, on every graph: equal to the bit"""
    new, old, _ = runs
    n = sum(1 for k in new if k.endswith("/trials") and not k.startswith("stop"))
    assert n == (len(PLAIN) + len(LM_REJECT_CASES) + 2) * 2 * 4
    assert_equal_runs(new, old)
    for gi, (_, trials) in enumerate(LM_REJECT_CASES):     # the fixtures did reject (and so did the new opening)
        assert new["reject%d/m0/a0/trials" % gi].tolist() == trials


def test_synchronous_form_equals_the_old_opening(runs):
    """SE2GPU_BA_SYNC=1 (one slot enqueued at a time, the form the per-kernel pass takes): the same bits again"""
    _, old, sync = runs
    assert_equal_runs(sync, old)


def test_stop_flag_before_the_run(runs, synth):
    """a flag that is already up ends the run in k_open's finisher: the estimate is untouched, nothing was counted, chi2_init is
    the start's - and the run after it is the old opening's"""
    new, old, _ = runs
    g = synth.ba_graph(30, 2000)
    for mode in (LM, GN):
        k = "stop/m%d/" % mode
        assert np.array_equal(new[k + "before/poses"], g.poses) and np.array_equal(new[k + "before/lms"], g.lms)
        assert new[k + "before/counts"].tolist() == [0, 0]
        assert new[k + "before/chi2"][-2] == new[k + "after/chi2"][-2] == new["plain1/m%d/a0/chi2" % mode][-2]
        for f in ("trials", "lambda", "chi2", "poses", "lms", "counts"):
            assert same_bits(new[k + "after/" + f], old[k + "after/" + f]), (mode, f)


# Gauss-Newton on ba_graph(50, 5000) is not among the oracle's cases: the oracle's own fifth undamped step there meets a
# non-positive pivot (its chi2_hist holds DBL_MAX), and what follows a factorisation of a system that is singular to rounding is
# decided by the last bits of either implementation - the oracle is no reference for it.  (That run is still compared bit for
# bit with the old opening's above.)  The kidnapped starts are test_lm_rejected_trials_follow_the_oracle's, which now runs k_open.
ORACLE_CASES = [(w, m) for w in ("plain0", "plain1", "plain2", "no_odometry", "bare_pose") for m in (LM, GN)
                if (w, m) != ("plain2", GN)]


@pytest.mark.parametrize("which,mode", ORACLE_CASES)
def test_matches_oracle(runs, oracle, synth, which, mode):
    """the assertions of test_lm_10_iterations_match_oracle on the runs of the new opening"""
    new = runs[0]
    g = dict(_graphs(synth))[which]
    p_ref, l_ref, st = oracle.ba_optimize(g, 10, mode)
    assert max(st["chi2_hist"]) < 1e300      # the oracle's own run is well posed (see ORACLE_CASES)
    k = "%s/m%d/a0/" % (which, mode)
    chi2 = new[k + "chi2"]
    assert new[k + "trials"].tolist() == st["trials_hist"]
    n = len(st["chi2_hist"])
    assert n == 10
    assert np.allclose(chi2[:n], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(new[k + "lambda"][:n], st["lambda_hist"], rtol=REL, atol=0)
    assert chi2[-2] == pytest.approx(st["chi2_init"], rel=1e-12)
    assert chi2[-1] == pytest.approx(st["chi2_final"], rel=REL)
    pose_update_close(new[k + "poses"], p_ref, g.poses)
    dl = np.abs((new[k + "lms"] - g.lms) - (l_ref - g.lms)).max()
    assert dl <= REL * np.abs(l_ref - g.lms).max()


if __name__ == "__main__":
    ba_ab.child_main(_scenarios, sys.argv[1:])
