"""The SE(2) reduced system of the HIP kernels against an EXTENDED-PRECISION assembly of the same sums (tests/scaled_parity.py:
se2_system_from_reference_edges in np.longdouble, from the compiled reference's per-edge residuals and Jacobians), in the
system's own scale.  The oracle is a double-precision assembly too; its distance to the extended one is the yardstick: the
kernels associate differently (8-lane groups, the group records of k_reduce2) and use the Cholesky form Hll + lambda I = G G'
where the oracle inverts explicitly, which the factor 32 covers - an order of magnitude, not a tolerance of its own.

`python tests/test_scaled_parity_gpu.py [file]` measures every system the parity tests compare and writes
profiles/system_parity.md (or `file`)."""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import scaled_parity as sp
from ba_cases import env, opt, opt3, pg
from oracle import ref

MARGIN = 32.0
FLOOR = 2.0 ** -50        # no bound under four ulps of the unit diagonal


def _ext_distances(oracle, g, lam, edges):
    """-> ((kernel to extended: matrix, right-hand side), (oracle to extended: ...)), in the extended system's scale"""
    Se, be = sp.se2_system_from_reference_edges(g, lam, np.longdouble, edges)
    S, bs = opt(g).reduced_system(lam)
    r = oracle.ba_reduced_system(g, lam)
    return ((sp.scaled_distance(S, Se), sp.scaled_rhs_distance(bs, be, Se)),
            (sp.scaled_distance(r["S"], Se), sp.scaled_rhs_distance(r["bs"], be, Se)))


@pytest.mark.gpu
@pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built and the reference's sources are not here")
@pytest.mark.parametrize("chol", [None, "steps"])
@pytest.mark.parametrize("P,L", [(8, 60), (21, 800)])
def test_kernels_are_as_close_to_the_extended_precision_system_as_the_oracle(oracle, synth, P, L, chol):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    g = synth.ba_graph(P, L)
    edges = sp.reference_edges(g)
    for lam in (0.0, 3.0):
        with env(SE2GPU_BA_RESIDENT="0", SE2GPU_BA_CHOL=chol):     # the multi-launch kernels; `steps` forms the system anew
            (kS, kb), (oS, ob) = _ext_distances(oracle, g, lam, edges)
        print(f"{P}/{L} lambda {lam} chol {chol}: kernels to extended {kS:.2e} / {kb:.2e}, oracle to extended {oS:.2e} / {ob:.2e}")
        assert kS <= max(MARGIN * oS, FLOOR) and kb <= max(MARGIN * ob, FLOOR)


# ---- the record ---------------------------------------------------------------------------------------------------------------
def _row(name, lam, A, b, Ar, br, A0, floor, ext=None):
    k = sp.kappa_scaled(A0)
    cells = [name, f"{lam:g}", f"{sp.old_distance(A, Ar):.1e}", f"{sp.old_distance(b, br):.1e}", f"{sp.scaled_distance(A, Ar):.1e}",
             f"{sp.scaled_rhs_distance(b, br, Ar):.1e}", f"{sp.scaled_asymmetry(A, Ar):.1e}", f"{floor[0]:.1e} / {floor[1]:.1e}",
             f"{k:.1e}", f"{sp.STEP_SHARE / k:.1e}"]
    cells.append("" if ext is None else "%.1e / %.1e; %.1e / %.1e" % (ext[0] + ext[1]))
    return "| " + " | ".join(cells) + " |"


def write_record(path):
    import datetime
    import independent as ind
    import off_axis_cases as oa
    import test_sparsify as ts
    from oracle import oracle
    from se2lam_amd import synth
    from se2lam_amd.sparsifier import DoMarginalizeSE3XYZ_batch
    oracle.lib()
    se2 = lambda q, lam: (lambda r: (r["S"], r["bs"]))(oracle.ba_reduced_system(q, lam))
    rows = []
    have_ref = ref.available()
    with env(SE2GPU_BA_RESIDENT="0", SE2GPU_BA_CHOL=None):
        cases = [("SE(2) ba_graph(%d, %d)" % c, synth.ba_graph(*c), lams, c in ((8, 60), (21, 800)))
                 for c, lams in (((8, 60), (0.0, 3.0)), ((21, 800), (0.0, 3.0)), ((50, 5000), (0.0, 17.5)))]
        cases += [("SE(2) off-axis (%d, %d)" % c, oa.graph(*c), (0.0, 3.0), False) for c in oa.SIZES]
        for name, g, lams, with_ext in cases:
            A0 = se2(g, 0.0)[0]
            edges = sp.reference_edges(g) if with_ext and have_ref else None
            for lam in lams:
                A, b = opt(g).reduced_system(lam)
                Ar, br = se2(g, lam)
                ext = _ext_distances(oracle, g, lam, edges) if edges is not None else None
                rows.append(_row(name, lam, A, b, Ar, br, A0, sp.reorder_floor(lambda q: se2(q, lam), g), ext))
        for c in ((8, 60, 0), (21, 800, 0), (21, 800, 4), (50, 5000, 0)):
            g = synth.ba3_graph(*c)
            A0 = oracle.ba3_reduced_system(g, 0.0)[0]
            for lam in (0.0, 2.5):
                A, b = opt3(g).reduced_system(lam)
                Ar, br = oracle.ba3_reduced_system(g, lam)
                rows.append(_row("SE3 ba3_graph(%d, %d, %d)" % c, lam, A, b, Ar, br, A0, sp.reorder_floor(lambda q: oracle.ba3_reduced_system(q, lam), g)))
        for P in (12, 60, 200):
            g = synth.pose_graph(P)
            A0 = oracle.pg_system(g, 0.0)[0]
            for lam in (0.0, 0.7):
                A, b = pg(g).reduced_system(lam)
                Ar, br = oracle.pg_system(g, lam)
                rows.append(_row("pose_graph(%d)" % P, lam, A, b, Ar, br, A0, sp.reorder_floor(lambda q: oracle.pg_system(q, lam), g)))
    old = [(12, 0, 400.0), (80, 1, 250.0), (200, 2, 800.0), (10, 4, 100.0), (150, 5, 600.0), (220, 196366, 484.40666147511246), (249, 77, 120.0)]
    pairs = ([("kf_pair(%d, %d, %g)" % c[:3], synth.kf_pair(*c), False) for c in old]
             + [("kf_pair(%d, %d, %g), m_info x %g" % c, ts._scaled_pair(synth, *c), True) for c in ts.WELL_CONDITIONED]
             + [("kf_pair(%d, %d, %g)" % a, synth.kf_pair(*a), False) for a, _ in ts.FEW_POINTS])
    srows = []
    for (name, pair, asserted), (z, info) in zip(pairs, DoMarginalizeSE3XYZ_batch([p for _, p, _ in pairs])):
        _, ir, _ = oracle.sparsify(*pair)
        lam = np.sort(np.linalg.eigvalsh(ir))
        srows.append("| %s | %.1e | %.1e | %.1e | %s | %s |" % (name, sp.old_distance(info, ir), ind.info_distance(info, ir),
                     ind.sparsify_ulp_floor(oracle.sparsify, pair), ", ".join("%.3g" % x for x in lam),
                     "distance <= 64 x floor" if asserted else "max-entry bound 1e-5 (distance recorded only)"))
    text = open(path).read() if os.path.exists(path) else "# Parity of the linear systems in their own scale\n\n<!-- tables -->\n"
    head, _, _ = text.partition("<!-- tables -->")
    out = [head + "<!-- tables -->", "Measured %s on one AMD Instinct MI355X (gfx950) by `python tests/test_scaled_parity_gpu.py`; the compiled reference "
           "for the extended-precision column was %s." % (datetime.date.today().isoformat(), "present" if have_ref else "absent"), "",
           "| system | lambda | old: S | old: b | scaled: S | scaled: b | scaled asymmetry | reorder floor S / b | kappa (lambda 0) | bound | to S_ext: kernels S / b; oracle S / b |",
           "|---|---|---|---|---|---|---|---|---|---|---|"] + rows + ["",
           "| sparsifier pair | old: max-entry | relative information distance | one-ulp floor of the oracle | eigenvalues (oracle) | asserted |",
           "|---|---|---|---|---|---|"] + srows
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    write_record(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "system_parity.md"))
