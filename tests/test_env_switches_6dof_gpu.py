"""tests/test_env_switches_gpu.py runs an SE(2) script; this file puts the two 6-DoF pose models (pose graph, SE3-expmap on the
multi-launch path) under the switches that select other kernels or another order on the 6 x 6-block system.  The switches are
read when a handle is made and pooled handles keep theirs, so every case is a fresh interpreter.  The script holds each run to
its oracle (the bounds of tests/test_pg_gpu.py and tests/test_ba3_gpu.py) and writes histories and estimates to a file; the
test holds every switch's file to the defaults' file: to the bit where only the host side changes (the plan, graph capture, the
synchronous controller), to equal trials and 1e-9 relative - RTOL of tests/test_ba_window_se3_gpu.py, two paths of one model -
where the solve sums in another order."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9

SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
os.environ["SE2GPU_BA_RESIDENT"] = "0"
from oracle import oracle
from se2lam_amd import synth, optimizer as op
import pg_cases
REL = 1e-5
out = {}

def held(name, o, g, st, X, n_pose):
    s = o.stats
    assert s["trials_hist"] == st["trials_hist"], (name, s["trials_hist"], st["trials_hist"])
    assert np.allclose(s["chi2_hist"], st["chi2_hist"], rtol=REL, atol=0), name
    assert np.allclose(s["lambda_hist"], st["lambda_hist"], rtol=REL, atol=0), name
    T = np.stack([op.estimateVertexSE3(o, a) for a in range(g.P)])
    assert np.abs(T - X).max() <= max(REL * np.abs(X - g.poses).max(), 1e-9), name
    f = np.asarray(g.fixed, bool)
    assert np.array_equal(T[f], g.poses[f]) if n_pose else np.allclose(T[f], g.poses[f], atol=1e-12), name
    p, l = o.estimates()
    out[name + "/trials"] = np.asarray(s["trials_hist"], np.int64)
    out[name + "/chi2"] = np.asarray([s["chi2_init"]] + s["chi2_hist"])
    out[name + "/lambda"] = np.asarray(s["lambda_hist"])
    out[name + "/poses"] = p
    out[name + "/lms"] = l
    out[name + "/solver_path"] = np.asarray([o.solver_path()], np.int64)

for name, g in (("pg12", synth.pose_graph(12)), ("slots17", pg_cases.layout("slots", 17)), ("reject", pg_cases.rejecting(*pg_cases.REJECTING[1]))):
    o = op.SlamOptimizer(); op.load_pose_graph(o, g); o.initializeOptimization(0); o.optimize(10)
    X, ec, st = oracle.pg_optimize(g, 10)
    held(name, o, g, st, X, True)
    assert np.allclose(op.edgeChi2(o, g.O), ec, rtol=1e-4, atol=1e-7), name
    out[name + "/edge_chi2"] = op.edgeChi2(o, g.O)
assert max(out["reject/trials"]) > 1
for name, g in (("se3_8", synth.ba3_graph(8, 60, 0)), ("se3_21", synth.ba3_graph(21, 800, 4))):
    o = op.SlamOptimizer(); op.load_se3_graph(o, g); o.initializeOptimization(0); o.optimize(10)
    X, l_ref, ec, st = oracle.ba3_optimize(g, 10)
    held(name, o, g, st, X, False)
    assert np.abs(o.estimates()[1] - l_ref).max() <= REL * np.abs(l_ref - g.lms).max(), name
np.savez(sys.argv[1], **out)
print("OK")
""" % (ROOT, ROOT)

# switch -> whether the run must equal the defaults' to the bit
CASES = [
    ({"SE2GPU_BA_PLAN": "host"}, True),         # graph plan (the pose graph: the slot plan's device half) built on the host
    ({"SE2GPU_BA_GRAPH": "0"}, True),           # no hipGraph capture / replay
    ({"SE2GPU_BA_SYNC": "1"}, True),            # host-side LM controller
    ({"SE2GPU_BA_ND": "0"}, False),             # natural pose order in the dense solve
    ({"SE2GPU_BA_CHOL": "steps"}, False),       # one launch per block column
    ({"SE2GPU_BA_HOST_SOLVE": "1"}, False),     # dense solve on the host
]


def _run(env, path):
    r = subprocess.run([sys.executable, "-c", SCRIPT, path], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (env, r.stdout[-500:], r.stderr[-1500:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def defaults(tmp_path_factory):
    return _run({}, str(tmp_path_factory.mktemp("switches6") / "defaults.npz"))


def test_defaults_hold_to_the_oracles(defaults):
    assert max(defaults["reject/trials"]) > 1


@pytest.mark.parametrize("env,to_the_bit", CASES, ids=[",".join(f"{k}={v}" for k, v in e.items()) for e, _ in CASES])
def test_switch_keeps_6dof_results(defaults, tmp_path, env, to_the_bit):
    got = _run(env, str(tmp_path / "switch.npz"))
    assert set(got) == set(defaults)
    # se2gpu_ba_debug_solver_path: 0 the dataflow launch, 1 one launch per block column, 3 the host - the switch was taken
    path = {"SE2GPU_BA_CHOL": 1, "SE2GPU_BA_HOST_SOLVE": 3}.get(next(iter(env)), 0)
    for k, ref in defaults.items():
        if k.endswith("/solver_path"):
            assert ref[0] == 0 and got[k][0] == path, (env, k, got[k])
        elif to_the_bit or k.endswith("/trials"):
            assert np.array_equal(got[k], ref), (env, k)
        elif k.endswith("/chi2") or k.endswith("/lambda"):
            assert np.allclose(got[k], ref, rtol=RTOL, atol=0), (env, k, np.abs(got[k] / ref - 1).max())
