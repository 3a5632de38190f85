"""Sparsifier::DoMarginalizeSE3XYZ (/root/reference/src/sparsifier.cpp:105-275): the oracle restatement
against an independent numpy model (central-difference Jacobians of the same minimal parametrisation with scipy's
quaternions, dense Schur complement, numpy's inverse and eigh), and the batched HIP kernel against the oracle."""
import numpy as np
import pytest


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
