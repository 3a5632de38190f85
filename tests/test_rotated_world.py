"""CPU preconditions of test_rotated_world_gpu.py: the moved problems are the same problems (both numpy models give the same cost
to 1e-10), and their vertices are general rotations (all four branches of the matrix-to-quaternion conversion among the key
frames of every case, no entry of a vertex rotation below 0.02).  If one of these fails the transform or the choice of G is wrong,
not a kernel."""
import numpy as np
import pytest

import pg_model
import world_cases as wc
from independent import BA3ProblemNumpy


@pytest.mark.parametrize("name", wc.PG_CASES)
def test_pose_graph_cost_is_invariant_and_the_vertices_are_general(name):
    g = wc.pg_case(name)
    h = wc.move_pose_graph(g)
    c0, e0 = pg_model.cost(g, g.poses)
    c1, e1 = pg_model.cost(h, h.poses)
    assert abs(c1 - c0) <= 1e-10 * c0
    assert np.allclose(e1, e0, rtol=1e-9, atol=1e-10 * c0)
    assert np.allclose(wc.pose_graph_back(h.poses), g.poses, rtol=0, atol=1e-9)
    n, small = wc.census(h.poses)
    assert (n > 0).all(), n
    assert small >= 0.02, small
    assert wc.census(g.poses)[1] < 1e-3          # what the generator's world has: entries that are zero to the noise


@pytest.mark.parametrize("name", wc.BA3_CASES)
def test_se3_window_cost_is_invariant_and_the_vertices_are_general(name):
    g = wc.ba3_case(name)
    h = wc.move_ba3(g)
    c0 = BA3ProblemNumpy(g).cost(g.poses, g.lms)
    c1 = BA3ProblemNumpy(h).cost(h.poses, h.lms)
    assert abs(c1 - c0) <= 1e-10 * c0
    assert np.linalg.eigvalsh(h.o_info).min() > 0
    p, l = wc.ba3_back(h.poses, h.lms)
    assert np.allclose(p, g.poses, rtol=0, atol=1e-8) and np.allclose(l, g.lms, rtol=0, atol=1e-8)
    n, small = wc.census(h.poses)
    assert (n > 0).all(), n
    assert small >= 0.02, small
    assert wc.census(g.poses)[1] < 1e-3


def test_the_oracle_agrees_that_the_moved_problems_are_the_same(oracle):
    """the C++ restatements on both sides of the move (their own sums, g2o's logarithm and its quaternion renormalisation, which
    the numpy models above do not have): 1e-9"""
    for name in wc.PG_CASES:
        g = wc.pg_case(name)
        assert oracle.pg_chi2(wc.move_pose_graph(g))[0] == pytest.approx(oracle.pg_chi2(g)[0], rel=1e-9)
    for name in wc.BA3_CASES:
        g = wc.ba3_case(name)
        assert oracle.ba3_chi2(wc.move_ba3(g))[0] == pytest.approx(oracle.ba3_chi2(g)[0], rel=1e-9)


def test_seam_ring_crosses_pi():
    g, head = wc.seam_ring()
    assert g.P == 6 and head[2] < np.pi < head[3] and np.abs(head - np.pi).max() < 0.7
    from scipy.spatial.transform import Rotation
    from se2lam_amd import synth
    Tcb = wc.inv(synth.tbc44())
    yaw = np.array([Rotation.from_matrix((T @ Tcb)[:3, :3]).as_rotvec()[2] for T in g.poses])
    assert (yaw[:3] > 2.4).all() and (yaw[3:] < -2.4).all()        # the body's yaw jumps by 2 pi between neighbours
    c, ec = pg_model.cost(g, g.poses)
    assert np.isfinite(c) and (ec < 1e3).all()                     # and no edge sees that jump
