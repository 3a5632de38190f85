"""CPU tests of tests/scaled_parity.py: the scaled distance has teeth where the unscaled one is blind, the oracle passes it
against its own reordering, and an extended-precision assembly from the compiled reference's edges says how far the oracle's
SE(2) system itself lies from the exact sums (the yardstick of tests/test_scaled_parity_gpu.py)."""
import numpy as np
import pytest

import scaled_parity as sp
from oracle import ref


# ---- the three systems of the gap: (model, graph, lambda, unscaled bound of the GPU tests) --------------------------------------
def _se2(oracle, g, lam):
    r = oracle.ba_reduced_system(g, lam)
    return r["S"], r["bs"]


SYSTEMS = {
    "se2": (sp.SE2, lambda synth: synth.ba_graph(50, 5000), 17.5, sp.OLD_SE2, _se2),
    "se3": (sp.SE3, lambda synth: synth.ba3_graph(50, 5000, 0), 2.5, sp.OLD_6DOF, lambda oracle, g, lam: oracle.ba3_reduced_system(g, lam)),
    "pg": (sp.PG, lambda synth: synth.pose_graph(200), 0.7, sp.OLD_6DOF, lambda oracle, g, lam: oracle.pg_system(g, lam)),
}
# the mutations the unscaled expression does see: a quarter of the pose graph's non-zeros is more than the 3 % under its bound
OLD_SEES = {("pg", "zero")}


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_scaled_distance_has_teeth_where_the_unscaled_bound_is_blind(oracle, synth, name):
    model, make, lam, old, system = SYSTEMS[name]
    g = make(synth)
    A, b = system(oracle, g, lam)
    tol = sp.bound(system(oracle, g, 0.0)[0])
    assert 1e-11 <= tol <= 2.2e-10                      # kappa 4.8e2 ... 8.7e3 on these graphs
    mutants = {"couplings": sp.scale_translation_couplings(A, model), "zero": sp.zero_smallest(A)}
    for what, M in mutants.items():
        assert not np.array_equal(M, A)
        d, d_old = sp.scaled_distance(M, A), sp.old_distance(M, A)
        print(f"{name} {what}: scaled {d:.2e} (bound {tol:.2e}), unscaled {d_old:.2e} (bound {old:.0e})")
        assert d > tol                                     # the scaled measure sees it, by orders of magnitude
        assert d > 1e3 * tol
        assert (d_old > old) == ((name, what) in OLD_SEES)     # the gap: the unscaled assertion lets it pass
    # the oracle against its own reordering passes, with orders to spare
    fA, fb = sp.reorder_floor(lambda q: system(oracle, q, lam), g)
    print(f"{name}: reorder floor {fA:.2e} / {fb:.2e}")
    assert 0 < fA <= 1e-3 * tol and fb <= 1e-3 * tol


def test_measures_on_a_hand_made_system():
    A = np.array([[4.0, 2.0, 0.0], [2.0, 1e8, 1e3], [0.0, 1e3, 0.0]])
    B = A.copy()
    B[0, 1] += 2e-4                                        # / (2 * 1e4)
    B[2, 1] += 3e-5                                        # / (1 * 1e4): the zero diagonal scales as 1
    assert np.array_equal(sp.jacobi(A), [2.0, 1e4, 1.0])
    assert sp.scaled_distance(B, A) == pytest.approx(1e-8, rel=1e-6)
    assert sp.scaled_asymmetry(B, A) == pytest.approx(1e-8, rel=1e-6)
    assert sp.scaled_rhs_distance([2.0, 1e4, 3.0], [2.0, 1e4 + 1.0, 3.0], A) == pytest.approx(1e-4 / 3.0)
    S = np.array([[4.0, 1.0], [1.0, 1e8]])
    assert sp.kappa_scaled(S) == pytest.approx((1 + 0.5e-4) / (1 - 0.5e-4), rel=1e-9)
    assert sp.bound(S) == pytest.approx(1e-7, rel=1e-3)
    p = sp.step_distance(np.array([1.0, 2.0, 1e-3, 3.0, 4.0, 2e-3 + 2e-9]), np.array([1.0, 2.0, 1e-3, 3.0, 4.0, 2e-3]), 3)
    assert p == pytest.approx(1e-6)                        # theta against its own maximum, not against the millimetres


# ---- the extended-precision adjudicator for SE(2) ------------------------------------------------------------------------------
# the oracle's scaled distance (S, b) to the extended-precision assembly, measured on the CPU; asserted within 4 x (libm and
# compiler differences between hosts)
ORACLE_TO_EXT = {(8, 60, 0.0): (7.2e-14, 1.5e-14), (8, 60, 3.0): (1.0e-14, 2.3e-14),
                 (21, 800, 0.0): (8.0e-14, 2.2e-14), (21, 800, 3.0): (6.3e-15, 1.8e-14)}


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built and the reference's sources are not here")
@pytest.mark.parametrize("P,L", [(8, 60), (21, 800)])
def test_oracle_against_the_extended_precision_assembly(oracle, synth, P, L):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63      # the adjudicator needs a longdouble wider than double
    g = synth.ba_graph(P, L)
    edges = sp.reference_edges(g)
    for lam in (0.0, 3.0):
        Se, be = sp.se2_system_from_reference_edges(g, lam, np.longdouble, edges)
        Sd, bd = sp.se2_system_from_reference_edges(g, lam, np.float64, edges)
        So, bo = _se2(oracle, g, lam)
        dS, db = sp.scaled_distance(So, Se), sp.scaled_rhs_distance(bo, be, Se)
        nS, nb = sp.scaled_distance(Sd, Se), sp.scaled_rhs_distance(bd, be, Se)
        print(f"{P}/{L} lambda {lam}: oracle to extended {dS:.2e} / {db:.2e}, double-precision numpy to extended {nS:.2e} / {nb:.2e}")
        wS, wb = ORACLE_TO_EXT[(P, L, lam)]
        assert dS <= 4 * wS and db <= 4 * wb
        assert nS <= 4 * 8e-14 and nb <= 4 * 4e-14           # the same assembly in double: 3.2e-14 ... 8e-14 at lambda 0
        assert max(dS, db, nS, nb) <= 1e-2 * sp.bound(_se2(oracle, g, 0.0)[0])
