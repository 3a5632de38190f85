"""The A/B harness of the bundle-adjustment kernel tests: a module runs its scenarios in this process, runs them again in child
processes with one environment switch flipped, and compares everything a run reports BIT FOR BIT.  A whole module:

    import os, sys, pytest, ba_ab
    from ba_cases import opt, no_odometry, thin                        # windows that reach the new kernel's branches
    pytestmark = pytest.mark.gpu
    SWITCHES = ("SE2GPU_BA_NEW", "SE2GPU_BA_SYNC")
    def _graphs(synth):
        return [("plain", synth.ba_graph(30, 2000)), ("no_odometry", no_odometry(synth)), ("thin", thin(synth))]
    def _scenarios(synth, out):
        for name, g in _graphs(synth):
            o = opt(g); ba_ab.system(o, out, name, 3.0e-2); o.optimize(10); ba_ab.record(o, out, name + "/n10", counts=2)
    @pytest.fixture(scope="module")
    def runs(synth, tmp_path_factory):
        assert not any(k in os.environ for k in SWITCHES)              # this process runs the defaults
        new, tmp = {}, tmp_path_factory.mktemp("new")
        _scenarios(synth, new)
        return [new] + [ba_ab.child(__file__, tmp, k, unset=SWITCHES, env_set={k: v}) for k, v in zip(SWITCHES, "01")]
    def test_equals_the_old_kernel(runs):
        ba_ab.assert_equal_runs(runs[0], runs[1])
    def test_synchronous_form_equals_the_old_kernel(runs):
        ba_ab.assert_equal_runs(runs[2], runs[1])
    if __name__ == "__main__":
        ba_ab.child_main(_scenarios, sys.argv[1:])

and a test that asserts, on the windows and on what the runs report, that each window did reach its branch.  No tests and no
fixtures here."""
import os
import subprocess
import sys

import numpy as np

import ba_cases  # noqa: F401  (puts the repository root on sys.path: a child process's script imports this module first)


def record(o, out, key, counts=None):
    """what the last optimize() of `o` reports, under key/...; counts = 2 or 3: that many of linearize_counts() as well (runs,
    skips; the third is the size of the record twin, and a handle out of the pool may bring a larger one along)"""
    s = o.stats
    poses, lms = o.estimates()
    out[key + "/trials"] = np.asarray(s["trials_hist"], np.int64)
    out[key + "/lambda"] = np.asarray(s["lambda_hist"], np.float64)
    out[key + "/chi2"] = np.asarray(s["chi2_hist"] + [s["chi2_init"], s["chi2_final"]], np.float64)
    out[key + "/poses"] = np.array(poses, np.float64)
    out[key + "/lms"] = np.array(lms, np.float64)
    if counts is not None:
        out[key + "/counts"] = np.asarray(o.linearize_counts()[:counts], np.int64)


def system(o, out, key, lam):
    """the reduced system of the handle's current state at damping `lam`, under key/S and key/bs"""
    S, bs = o.reduced_system(lam)
    out[key + "/S"], out[key + "/bs"] = np.array(S, np.float64), np.array(bs, np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equal_runs(new, old, *, only=None, skip=(), exempt_suffix=(), special=None):
    """the same keys on both sides, and every compared key the same bits; every key that differs is printed with its largest
    relative difference and named in the assertion.
        only           compare the keys with this prefix (or one of a tuple of prefixes)
        skip           keys not compared
        exempt_suffix  key endings not compared: what the two sides differ in by design
        special        {key ending: callable(key, new, old) holding its own assertion}, in place of the bit comparison"""
    assert sorted(new) == sorted(old)
    bad = []
    for k in sorted(new):
        if only is not None and not k.startswith(only):
            continue
        if k in skip or k.endswith(tuple(exempt_suffix)):
            continue
        rule = [f for s, f in (special or {}).items() if k.endswith(s)]
        if rule:
            rule[0](k, new[k], old[k])
            continue
        if same_bits(new[k], old[k]):
            continue
        d = float("nan")
        if new[k].shape == old[k].shape and new[k].dtype == np.float64:
            with np.errstate(all="ignore"):
                d = float(np.nanmax(np.abs(new[k] - old[k]) / np.maximum(np.abs(old[k]), 1e-300)))
        print("differs:", k, "max relative difference", d)
        bad.append(k)
    assert not bad, bad


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def child(script, tmp, name, *args, unset=(), env_set=None, timeout=600):
    """`python script tmp/name.npz args...` in a copy of this environment without the variables `unset` and with `env_set`, under
    its own time limit -> the arrays it saved"""
    path = str(tmp / (name + ".npz"))
    env = dict(os.environ)
    for k in unset:
        env.pop(k, None)
    env.update(env_set or {})
    r = subprocess.run([sys.executable, os.path.abspath(script), path] + [str(a) for a in args], capture_output=True, text=True,
                       env=env, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return load(path)


def child_main(scenarios, argv):
    """python script OUT.npz args...: scenarios(synth, out, *args), saved"""
    from se2lam_amd import synth
    out = {}
    scenarios(synth, out, *argv[1:])
    np.savez(argv[0], **out)
