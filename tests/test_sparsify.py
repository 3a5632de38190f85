"""Sparsifier::DoMarginalizeSE3XYZ (/root/reference/src/sparsifier.cpp:105-275): the oracle restatement
against an independent numpy model (central-difference Jacobians of the same minimal parametrisation with scipy's
quaternions, dense Schur complement, numpy's inverse and eigh), and the batched HIP kernel against the oracle."""
import numpy as np
import pytest


import independent as ind
from independent import sparsify_numpy_model as _numpy_model


@pytest.mark.parametrize("N,seed", [(12, 0), (80, 1), (200, 2)])
def test_oracle_against_the_numpy_model(oracle, synth, N, seed):
    kf, mp, m_kf, m_mp, m_info = synth.kf_pair(N, seed)
    z, info, Hm = oracle.sparsify(kf, mp, m_kf, m_mp, m_info)
    zn, infon, Hmn = _numpy_model(kf, mp, m_kf, m_mp, m_info)
    assert np.allclose(z, zn, atol=1e-9)
    # forward differences (delta 1e-6, the reference's) against central ones: agreement to ~1e-5 of the largest entry
    assert np.abs(Hm - Hmn).max() <= 2e-4 * np.abs(Hmn).max()
    lam = np.linalg.eigvalsh(info)
    assert np.abs(info - info.T).max() == 0 and lam.min() >= 1e-6 * (1 - 1e-9) and lam.max() <= 1e4 * (1 + 1e-9)
    # The step from H_marginal to the information is ill-conditioned BY CONSTRUCTION in the reference: two key frames and
    # their points have six gauge freedoms that only the 1e-6 I regulariser fixes, so H^-1 carries 1e6 in directions
    # the 6 x 12 Jacobian annihilates only as well as it is accurate - its forward-difference error (1e-7 relative) moves
    # the small (translation) eigenvalues of the result by tens of per cent against the central-difference model.  The
    # rotation eigenvalues sit at the 1e4 clamp on both sides; the translation ones agree in magnitude.
    ln = np.sort(np.linalg.eigvalsh(infon))
    lo = np.sort(lam)
    assert np.allclose(lo[3:], 1e4, rtol=1e-6) and np.allclose(ln[3:], 1e4, rtol=1e-6)
    assert np.all(lo[1:3] > 0.5 * ln[1:3]) and np.all(lo[1:3] < 2.0 * ln[1:3]) and 1e-6 <= lo[0] < lo[1]   # (the weakest direction: order of magnitude only)


def test_degenerate_inputs(oracle, synth):
    kf, mp, m_kf, m_mp, m_info = synth.kf_pair(12, 3)
    # measurements of a third key frame id are ignored (sparsifier.cpp:117-119), points without measurements drop out
    z0, i0, _ = oracle.sparsify(kf, mp, m_kf, m_mp, m_info)
    z1, i1, _ = oracle.sparsify(kf, np.r_[mp, [[1.0, 2.0, 3.0]]], np.r_[m_kf, 2], np.r_[m_mp, 12], np.concatenate([m_info, np.eye(3)[None]]))
    assert np.array_equal(z0, z1) and np.array_equal(i0, i1)


@pytest.mark.gpu
def test_hip_batch_matches_oracle(oracle, synth):
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ_batch
    # (the 220-point pair: found by tools/fuzz_gpu.py - with the points of a lane pre-summed, i.e. H11 added up in another
    # order than the reference's, its clamped spectrum came out 99 % off; H11 is regular only through the 1e-6 I)
    pairs = [synth.kf_pair(N, s, b) for N, s, b in ((12, 0, 400.0), (80, 1, 250.0), (200, 2, 800.0), (10, 4, 100.0), (150, 5, 600.0),
                                                     (220, 196366, 484.40666147511246), (249, 77, 120.0))]
    got = DoMarginalizeSE3XYZ_batch(pairs)
    for (kf, mp, m_kf, m_mp, m_info), (z, info) in zip(pairs, got):
        zr, ir, _ = oracle.sparsify(kf, mp, m_kf, m_mp, m_info)
        assert np.allclose(z, zr, atol=1e-12)
        assert np.abs(info - ir).max() <= 1e-5 * np.abs(ir).max()      # BASELINE's BA tolerance
        assert np.abs(info - info.T).max() == 0
        # (the reference itself is noise in the relative measure on these mm-scale pairs - one ulp of its inputs moves it by
        # per cent - so the figure is printed, and recorded in profiles/system_parity.md, not asserted)
        print("N = %d: |info - ref| / max %.2e, relative information distance %.2e" % (len(mp), np.abs(info - ir).max() / np.abs(ir).max(), ind.info_distance(info, ir)))


# ---- pairs on which the relative information distance is a measurement --------------------------------------------------------
# The bound above is 1e-5 of the largest entry: every pair above has its rotation eigenvalues at the 1e4 clamp, so it is 0.1
# absolute, over translation eigenvalues of 4e-5 ... 3.7.  With m_info scaled down the rotation eigenvalues come off the clamp
# (230, 2578, 3970; 658, 3071; 2300), one eigenvalue sits at the 1e-6 floor, and the restatement's own one-ulp floor in the
# relative measure is small enough to assert against.  The two- and one-point pairs have two and three eigenvalues at the floor.
WELL_CONDITIONED = [(80, 1, 250.0, 1e-5), (200, 2, 800.0, 1e-5), (80, 1, 250.0, 1e-4)]
FEW_POINTS = [((2, 9, 300.0), 2), ((1, 9, 300.0), 3)]


def _scaled_pair(synth, N, seed, baseline, f):
    kf, mp, m_kf, m_mp, m_info = synth.kf_pair(N, seed, baseline)
    return kf, mp, m_kf, m_mp, m_info * f


@pytest.mark.parametrize("N,seed,baseline,f", WELL_CONDITIONED)
def test_oracle_on_well_conditioned_pairs(oracle, synth, N, seed, baseline, f):
    """the restatement against the numpy model (z, symmetry and clamp only: forward against central differences), and the
    regime itself: a rotation eigenvalue inside the clamp, one eigenvalue at the floor, a one-ulp floor far below 1"""
    pair = _scaled_pair(synth, N, seed, baseline, f)
    z, info, _ = oracle.sparsify(*pair)
    ind.check_sparsify(pair, z, info, spectrum=False)
    lam = np.sort(np.linalg.eigvalsh(info))
    assert ((lam[3:] > 1e-6 * (1 + 1e-6)) & (lam[3:] < 1e4 * (1 - 1e-6))).any(), lam
    if f == 1e-5:
        assert lam[0] <= 1e-6 * (1 + 1e-6) < lam[1]          # one eigenvalue at the floor (the 1e-4 pair's weakest: 2.1e-6)
    floor = ind.sparsify_ulp_floor(oracle.sparsify, pair)
    print("N = %d, m_info x %g: eigenvalues %s, one-ulp floor %.2e" % (N, f, ["%.4g" % x for x in lam], floor))
    assert floor <= 1e-3                                    # measured 3.0e-5 / 2.9e-4 / 1.1e-4
    ind.check_sparsify_relative(z, info, z, info, floor)    # (the check itself, on the restatement)


@pytest.mark.parametrize("args,at_floor", FEW_POINTS)
def test_oracle_on_pairs_with_few_points(oracle, synth, args, at_floor):
    pair = synth.kf_pair(*args)
    z, info, _ = oracle.sparsify(*pair)
    ind.check_sparsify(pair, z, info, spectrum=False)
    lam = np.sort(np.linalg.eigvalsh(info))
    assert (lam <= 1e-6 * (1 + 1e-6)).sum() == at_floor, lam


@pytest.mark.gpu
def test_hip_batch_on_well_conditioned_and_few_point_pairs(oracle, synth):
    """DoMarginalizeSE3XYZ_batch on the pairs above, in one batch: the well-conditioned ones within 64 x the restatement's
    one-ulp floor in the relative information distance, the few-point ones at the suite's present assertion"""
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ_batch
    pairs = [_scaled_pair(synth, *c) for c in WELL_CONDITIONED] + [synth.kf_pair(*a) for a, _ in FEW_POINTS]
    got = DoMarginalizeSE3XYZ_batch(pairs)
    for k, (pair, (z, info)) in enumerate(zip(pairs, got)):
        zr, ir, _ = oracle.sparsify(*pair)
        ind.check_sparsify(pair, z, info, spectrum=False)
        if k < len(WELL_CONDITIONED):
            ind.check_sparsify_relative(z, info, zr, ir, ind.sparsify_ulp_floor(oracle.sparsify, pair))
        else:
            ind.check_sparsify_equals(z, info, zr, ir)
            assert np.abs(info - info.T).max() == 0
