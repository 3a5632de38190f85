"""The dense pose solve with its dependency lists in depth order (csrc/ba.hip: solve_plan_build, d_chol_tiles) on the device.
synth.ba_graph(50, 5000) is the smallest synthetic graph that takes a permuted ring plan - two arcs and a separator, whose first
column waits for the last columns of BOTH arcs (neager = 2) and sums its products in another order than the column order;
ba_graph(21, 600) keeps the natural order (ascending lists, the right-hand-side row inside the last diagonal tile).
The bound is the project's: 1e-9 * max|x| against a host Cholesky refined in extended precision."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ba_cases import opt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (30.0, 3.0)


def _refined(S, bs):
    c = np.linalg.cholesky(S)
    solve = lambda r: np.linalg.solve(c.T, np.linalg.solve(c, r))
    x = solve(bs).astype(np.longdouble)
    for _ in range(3):
        x = x + solve((bs.astype(np.longdouble) - S.astype(np.longdouble) @ x).astype(np.float64))
    return x.astype(np.float64)


_ref = {}


def _reference(o, key, lam):
    """the refined host solution of the handle's reduced system: computed once per (graph, lambda), shared, never modified"""
    if (key, lam) not in _ref:
        S, bs = o.reduced_system(lam)
        x = _refined(S, bs)
        x.setflags(write=False)
        _ref[(key, lam)] = x
    return _ref[(key, lam)]


def _check_solves(o, key):
    for lam in LAMBDAS:
        want = _reference(o, key, lam)
        for _ in range(2):                              # twice: the flags carry the solve's epoch
            x, ok = o.solve(lam)
            err = np.abs(x - want).max()
            print(f"{key} lambda {lam}: max|x - x_ref| = {err:.3e}, bound {1e-9 * np.abs(want).max():.3e}")
            assert ok
            assert err <= 1e-9 * np.abs(want).max()


def test_ring_plan_is_permuted_and_has_a_two_way_junction(synth):
    o = opt(synth.ba_graph(50, 5000))
    nsys, permuted, ne = o.plan_neager()
    assert o.solver_path() == 0
    assert permuted and nsys > 150 and nsys % 32 == 0
    assert ne.max() >= 2 and ne.min() >= 0


def test_ring_plan_solve_matches_refined_host_cholesky(synth):
    o = opt(synth.ba_graph(50, 5000))
    assert o.plan_neager()[1] and o.plan_neager()[2].max() >= 2
    _check_solves(o, "ring 50")
    assert o.solver_path() == 0                         # no time-out, no fallback to the column launches


def test_two_fresh_handles_agree_to_the_bit(synth):
    g = synth.ba_graph(50, 5000)
    a, b = opt(g), opt(g)
    for lam in LAMBDAS:
        xa, oka = a.solve(lam)
        xb, okb = b.solve(lam)
        assert oka and okb and np.array_equal(xa, xb)
    a.optimize(10)
    b.optimize(10)
    assert a.stats == b.stats
    assert np.array_equal(a.estimates()[0], b.estimates()[0]) and np.array_equal(a.estimates()[1], b.estimates()[1])
    assert a.solver_path() == 0 and b.solver_path() == 0


def test_unpermuted_plan_with_the_rhs_row_inside_the_last_diagonal_tile(synth):
    o = opt(synth.ba_graph(21, 600))
    nsys, permuted, ne = o.plan_neager()
    assert not permuted and nsys == 63 and nsys // 32 == (nsys - 1) // 32       # row 63 = the last row of diagonal tile 1
    assert ne.max() == 1
    _check_solves(o, "natural 21")
    assert o.solver_path() == 0


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from se2lam_amd import synth
import test_ba_solve_order_gpu as t
mode = sys.argv[1]
o = t.opt(synth.ba_graph(50, 5000))
nsys, permuted, ne = o.plan_neager()
if mode == "natural":
    assert not permuted and nsys == 150 and ne.max() == 1, (nsys, permuted, ne.max())
    t._check_solves(o, "ring 50, natural order")
else:
    assert permuted and ne.max() >= 2
    o.optimize(10)
    bad, checked, rec = o.chol_verify()
    print("handoffs", checked, "mismatches", bad)
    assert checked > 0 and bad == 0, (checked, bad, rec)
assert o.solver_path() == 0
print("OK")
""" % (ROOT, os.path.join(ROOT, "tests"))


def _child(mode, env):
    r = subprocess.run([sys.executable, "-c", CHILD, mode], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (mode, r.stdout[-500:], r.stderr[-1500:])


def test_natural_order_switch_meets_the_same_bound():
    """SE2GPU_BA_ND=0 (read once per process): the same graph in the natural order"""
    _child("natural", {"SE2GPU_BA_ND": "0"})


def test_every_hand_off_of_the_ring_plan_verifies():
    """SE2GPU_BA_CHOL_VERIFY=1: every published half-slab travels with a checksum, every consumer checks its loads"""
    _child("verify", {"SE2GPU_BA_CHOL_VERIFY": "1"})
