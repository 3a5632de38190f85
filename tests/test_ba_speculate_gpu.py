"""The speculating trial slot of the single-window SE(2) run: k_update<true> also linearises the trial state it evaluates, for
the damping lambda / 3 that an accepted trial with a gain ratio >= 0.937 leaves, and the next slot's k_linearize<true> returns
at once when that guess held (csrc/ba.hip).

Both slots run the same expressions on the same inputs, so the results of the default library are compared BIT FOR BIT with the
old slot's (SE2GPU_BA_SPECULATE=0, read once per process: a child process computes them), and with the CPU oracle under the
bounds of test_ba_gpu.py.  How many stand-alone linearisations a run needs follows from the oracle's histories alone.
"""
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import ba_ab
from ba_ab import same_bits
from ba_cases import LM_REJECT_CASES, REL, ROOT, kidnapped, opt, pose_update_close

pytestmark = pytest.mark.gpu

PLAIN = [(8, 60), (30, 2000), (50, 5000)]
LM, GN = 0, 1


def _graphs(synth):
    return [synth.ba_graph(P, L) for P, L in PLAIN] + [kidnapped(synth, *c[0]) for c in LM_REJECT_CASES]


def _record(o, out, key):
    ba_ab.record(o, out, key, counts=3)


def _scenarios(synth, out):
    """every graph x {LM, GN} x {optimize(10); optimize(1); optimize(3) twice without a reset}, each on a handle of its own;
    optimize(5) - reset_estimates - optimize(5); a stop flag that is up before the run"""
    for gi, g in enumerate(_graphs(synth)):
        for mode in (LM, GN):
            for name, calls in (("a", [10]), ("b", [1]), ("c", [3, 3])):
                o = opt(g)
                for ci, n in enumerate(calls):
                    o.optimize(n, mode)
                    _record(o, out, "g%d/m%d/%s%d" % (gi, mode, name, ci))
    for gi, g in enumerate(_graphs(synth)):
        o = opt(g)
        o.optimize(5)
        o.reset_estimates()
        o.optimize(5)
        _record(o, out, "reset/g%d" % gi)
        f = opt(g)
        f.optimize(5)
        _record(f, out, "fresh/g%d" % gi)
    g = synth.ba_graph(30, 2000)
    o = opt(g)
    flag = np.ones(1, np.uint8)
    o.setForceStopFlag(flag)
    assert o.optimize(10) == 0 and o.stats["stopped"]
    _record(o, out, "stop/before")
    flag[0] = 0
    assert o.optimize(4) == 4
    _record(o, out, "stop/after")


def _child_scenarios(synth, out, which, *args):
    """python test_ba_speculate_gpu.py OUT.npz all | python test_ba_speculate_gpu.py OUT.npz iters P L K MODE"""
    if which == "all":
        return _scenarios(synth, out)
    P, L, k, mode = (int(a) for a in args)
    o = opt(synth.ba_graph(P, L))
    o.optimize(k, mode)
    _record(o, out, "iters")


def _old_slot(tmp_path, *args):
    """the same work by the old slot: a child process that inherits this environment with SE2GPU_BA_SPECULATE=0"""
    return ba_ab.child(__file__, tmp_path, "old_" + "_".join(str(a) for a in args), *args, env_set={"SE2GPU_BA_SPECULATE": "0"})


def _counts(k, new, old):
    """the counters are the one thing that differs (the old slot never skips)"""
    assert old[1] == 0 and old[2] == 0, (k, old)      # old slot: no skip, no second record set
    assert new[0] + new[1] == old[0], (k, new, old)


def _assert_equal_runs(new, old, only):
    """histories identical, cost / poses / landmarks bit for bit"""
    ba_ab.assert_equal_runs(new, old, only=only, special={"/counts": _counts})


@pytest.fixture(scope="module")
def runs(synth, tmp_path_factory):
    """the scenarios by the speculating slot (this process) and by the old one"""
    new = {}
    _scenarios(synth, new)
    old = _old_slot(tmp_path_factory.mktemp("speculate"), "all")
    return new, old


def test_same_results_as_the_old_slot(runs):
    """3 plain windows + the five starts that reject trials, LM and GN, optimize(10) / optimize(1) / optimize(3) twice: trial and
    lambda histories identical, chi^2, poses and landmarks equal to the bit"""
    new, old = runs
    n = sum(1 for k in new if k.startswith("g") and k.endswith("/trials"))
    assert n == (len(PLAIN) + len(LM_REJECT_CASES)) * 2 * 4
    _assert_equal_runs(new, old, "g")
    for gi, (_, trials) in enumerate(LM_REJECT_CASES):     # the fixtures did reject (and so did the new slot)
        assert new["g%d/m0/a0/trials" % (len(PLAIN) + gi)].tolist() == trials


def test_reset_between_runs_and_stop_flag_before_a_run(runs):
    """optimize(5), reset_estimates(), optimize(5) = a fresh handle's optimize(5) (no record of the first run survives); a stop
    flag that is already up leaves the start untouched, and the run after it is the old slot's"""
    new, old = runs
    _assert_equal_runs(new, old, ("reset", "fresh", "stop"))
    for gi in range(len(PLAIN) + len(LM_REJECT_CASES)):
        for f in ("trials", "lambda", "chi2", "poses", "lms"):
            assert same_bits(new["reset/g%d/%s" % (gi, f)], new["fresh/g%d/%s" % (gi, f)]), (gi, f)
        # (the third count is the size of the record twin: a handle out of the pool may bring a larger one along)
        assert new["reset/g%d/counts" % gi][:2].tolist() == new["fresh/g%d/counts" % gi][:2].tolist()
    assert new["stop/before/counts"][:2].tolist() == [0, 0]


def test_stop_flag_during_a_run(synth, tmp_path):
    """a flag raised while the slots are running (the pattern of test_force_stop_flag): the run ends after some iteration k,
    with the estimate the old slot has after optimize(k)"""
    P, L = 50, 5000
    g = synth.ba_graph(P, L)
    o = opt(g)
    flag = np.zeros(1, np.uint8)
    o.setForceStopFlag(flag)

    def raise_it():
        time.sleep(0.002)
        flag[0] = 1
    t = threading.Thread(target=raise_it)
    t.start()
    k = o.optimize(60)
    t.join()
    assert 0 <= k <= 60 and (o.stats["stopped"] or k == 60)
    print("stopped after", k, "iterations")
    new = {}
    _record(o, new, "iters")
    if k == 0:
        assert np.array_equal(new["iters/poses"], g.poses)
        return
    old = _old_slot(tmp_path, "iters", P, L, k, LM)
    for f in ("trials", "lambda", "poses", "lms"):
        assert same_bits(new["iters/" + f], old["iters/" + f]), f
    assert same_bits(new["iters/chi2"][:k], old["iters/chi2"][:k])


def expected_linearisations(st, mode):
    """stand-alone linearisations a run needs, from the oracle's histories: the first trial, every rejected trial, every accept
    that is followed by another slot and whose new lambda is not bitwise lambda * (1/3) (lm_advance's expression).  The damping of
    an accepted trial is the one the iteration before left, doubled, quadrupled, ... by the iteration's own rejections; the very
    first one (lambda_0) is not in the histories, so the accept of iteration 0 is judged by its gain ratio instead:
    1 - (2 rho - 1)^3 <= 1/3."""
    trials, lam = st["trials_hist"], st["lambda_hist"]
    runs = 1 + sum(t - 1 for t in trials)
    if mode == GN:
        return runs
    rho = st["rho_log"]
    assert len(rho) == sum(trials)
    for i in range(len(trials) - 1):          # (the accept of the last iteration has no slot after it)
        if i == 0:
            r = rho[trials[0] - 1]
            hit = 1.0 - (2 * r - 1) ** 3 <= 1.0 / 3.0
        else:
            lt = lam[i - 1]
            for q in range(trials[i] - 1):
                lt *= 2.0 ** (q + 1)
            lt *= 1.0 / 3.0
            hit = lam[i] == lt
        runs += 0 if hit else 1
    return runs


def test_linearisation_counts_follow_from_the_oracle(oracle, synth):
    """runs = what the oracle's histories say a run needs, runs + skips = trial slots; ba_graph(50, 5000): 1 run, 9 skips"""
    for gi, g in enumerate(_graphs(synth)):
        for mode in (LM, GN):
            _, _, st = oracle.ba_optimize(g, 10, mode)
            o = opt(g)
            o.optimize(10, mode)
            runs, skips, twin = o.linearize_counts()
            print("graph", gi, "mode", mode, "trials", st["trials_hist"], "runs", runs, "skips", skips)
            assert o.stats["trials_hist"] == st["trials_hist"]
            assert runs == expected_linearisations(st, mode), (gi, mode, runs, skips)
            assert runs + skips == st["trials"] == sum(st["trials_hist"])
            assert twin > 0
            if mode == LM and gi == 2:
                assert (runs, skips) == (1, 9)

@pytest.mark.parametrize("mode", [LM, GN])
def test_30kf_2000_landmarks_match_oracle(oracle, synth, mode):
    """the assertions of test_lm_10_iterations_match_oracle on ba_graph(30, 2000), LM and GN"""
    g = synth.ba_graph(30, 2000)
    o = opt(g)
    assert o.optimize(10, mode) == 10
    p_ref, l_ref, st = oracle.ba_optimize(g, 10, mode)
    s = o.stats
    assert s["trials_hist"] == st["trials_hist"]
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0)
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0)
    assert s["chi2_init"] == pytest.approx(st["chi2_init"], rel=1e-12)
    assert s["chi2_final"] == pytest.approx(st["chi2_final"], rel=REL)
    poses, lms = o.estimates()
    pose_update_close(poses, p_ref, g.poses)
    dl = np.abs((lms - g.lms) - (l_ref - g.lms)).max()
    assert dl <= REL * np.abs(l_ref - g.lms).max()
    assert o.activeRobustChi2() == pytest.approx(s["chi2_final"], rel=1e-12)


def test_no_twin_records_for_a_window_that_only_ran_in_a_resident_batch(tmp_path):
    """the second record set is made by the first single-window run that speculates: windows that only ever ran in a resident
    batch (which borrows the first set's idle buffers) have none.  In a child without the handle pool, so that no handle
    brings buffers from an earlier life."""
    code = ("import json, os, sys; sys.path.insert(0, %r)\n"
            "from se2lam_amd import synth, capi\n"
            "from se2lam_amd.optimizer import SlamOptimizer, optimize_batch\n"
            "g = synth.ba_graph(8, 60)\n"
            "os.environ['SE2GPU_BA_RESIDENT'] = '1'\n"
            "opts = []\n"
            "for i in range(8):\n"
            "    o = SlamOptimizer(); o.load(g); o.initializeOptimization(0); opts.append(o)\n"
            "optimize_batch(opts, 10)\n"
            "path = int(capi.lib().se2gpu_ba_last_batch_path())\n"
            "twins = [o.linearize_counts()[2] for o in opts]\n"
            "opts[0].optimize(10)\n"
            "print(json.dumps({'path': path, 'twins': twins, 'after': opts[0].linearize_counts()[2], 'E': int(g.E), 'L': int(g.L)}))\n"
            ) % ROOT
    env = dict(os.environ)
    env["SE2GPU_BA_POOL"] = "0"
    env.pop("SE2GPU_BA_SPECULATE", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["path"] == 2
    assert got["twins"] == [0] * 8
    assert got["after"] >= 8 * (21 * got["E"] + 18 * got["L"])


if __name__ == "__main__":
    ba_ab.child_main(_child_scenarios, sys.argv[1:])
