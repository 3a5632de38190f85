"""CPU tests that hold the cases of tests/pg_cases.py to their conditions, and the pose-graph restatement (oracle/pg_ref.cpp)
to the independent model of tests/pg_model.py on every one of them - so that a failure of tests/test_pg_layouts_gpu.py means
the kernels and not the case or the oracle.

`python tests/test_pg_model.py` writes profiles/pg_layouts.md: condition numbers, and the distance between the oracle's normal
equations and the model's.  The recorded bound of a row is the measured distance (at least eps / h = 2.2e-13, the round-off of
the difference quotient) doubled and rounded up to a power of ten: the model's error is round-off of a difference quotient,
which changes by about its own size with the order in which a processor's BLAS sums a 4 x 4 product.  The test below holds
the measurement under the bound, and the GPU test adds its oracle tolerance to the same bound."""
import dataclasses
import math
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pg_cases
import pg_model
from pg_cases import RECORD, recorded, recorded_scaled

SIZES = (6, 17)
COND_MAX = 1e12
# (the sizes the GPU tests add - 2, 3 and `complete` at 40 - are held to the same conditions: their rows are read there too)
LAYOUTS = [(k, P) for P in (2, 3) + SIZES for k in pg_cases.kinds_at(P)] + [("complete", 40)]


def _bound(x):
    """(no bound under the round-off of the difference quotient itself, eps / h relative to the error it differences)"""
    return 10.0 ** math.ceil(math.log10(2.0 * max(x, np.finfo(float).eps / pg_model.H_STEP)))


def _measure(oracle, kind, P):
    g = pg_cases.layout(kind, P)
    H, b = oracle.pg_system(g, 0.0)
    Hm, bm = pg_model.system(g, g.poses)
    f = pg_model.free_mask(g)
    ev = np.linalg.eigvalsh(H[f][:, f])
    return g, ev, pg_model.distance(g, H, b, Hm, bm), pg_model.scaled_distance(g, H, b, Hm, bm)


@pytest.mark.parametrize("kind,P", LAYOUTS)
def test_layout_is_well_posed_and_the_oracle_equals_the_model(oracle, kind, P):
    g, ev, (dH, db), (sH, sb) = _measure(oracle, kind, P)
    assert ev.min() > 0                                       # SPD on the free key frames
    assert ev.max() / ev.min() < COND_MAX
    c, ec = oracle.pg_chi2(g)
    cm, ecm = pg_model.cost(g, g.poses)
    assert c == pytest.approx(cm, rel=1e-10) and np.allclose(ec, ecm, rtol=1e-9, atol=1e-12)     # as test_pg_oracle.py
    bH, bb = recorded()[(kind, P)]
    print(f"{kind} P={P}: cond {ev.max() / ev.min():.2e}, |H-Hm|/max {dH:.2e} (recorded bound {bH:.0e}), |b-bm|/max {db:.2e} ({bb:.0e})")
    assert dH <= bH and db <= bb
    cH, cb = recorded_scaled()[(kind, P)]
    print(f"{kind} P={P}: in the system's own scale {sH:.2e} (recorded bound {cH:.0e}), {sb:.2e} ({cb:.0e})")
    assert sH <= cH and sb <= cb
    X, _, st = oracle.pg_optimize(g, 8)                       # a clean run: eight iterations, none given up
    assert st["iterations"] == 8 and not st["terminated"] and np.isfinite(st["chi2_hist"]).all()
    assert st["chi2_final"] == pytest.approx(pg_model.cost(g, X)[0], rel=1e-9)


def test_every_layout_has_what_its_row_promises():
    for P in SIZES:
        g = pg_cases.layout("multi_fixed", P)
        fx = g.fixed.astype(bool)
        assert fx.sum() == 3
        both = fx[g.o_i] & fx[g.o_j]
        assert both.any() and (fx[g.o_i] & ~fx[g.o_j] & (g.o_i > 0)).any() and (~fx[g.o_i] & fx[g.o_j] & (g.o_j > 0)).any()
        g = pg_cases.layout("slots", P)
        key = [(min(a, b), max(a, b)) for a, b in zip(g.o_i, g.o_j)]
        sizes = {k: key.count(k) for k in set(key)}
        assert {2, 3, 4} <= set(sizes.values()) and max(sizes.values()) == 4 and sizes[(0, 1)] == 4
        mixed = {n for k, n in sizes.items() if len({(int(a), int(b)) for a, b in zip(g.o_i, g.o_j) if (min(a, b), max(a, b)) == k}) == 2}
        assert {2, 4} <= mixed                                # both orientations inside a two-edge and a four-edge slot
        assert (pg_cases.layout("upper_only", P).o_i < pg_cases.layout("upper_only", P).o_j).all()
        assert not pg_cases.layout("star", P).has_prior.any() and not pg_cases.layout("chain_no_priors", P).has_prior.any()
        sp = pg_cases.layout("sparse_priors", P).has_prior
        assert sp.any() and not sp.all()
        g = pg_cases.layout("components", P)
        assert not ((g.o_i < P // 2) ^ (g.o_j < P // 2)).any()
        assert pg_cases.layout("complete", P).O == P * (P - 1) // 2
        s, base = pg_cases.layout("shuffled", P), pg_cases.synth.pose_graph(P)
        assert s.O == base.O and not np.array_equal(s.o_i, base.o_i)
        for kind in pg_cases.kinds_at(P):                     # no key frame is held by its prior alone
            g = pg_cases.layout(kind, P)
            assert np.bincount(np.r_[g.o_i, g.o_j], minlength=P).min() > 0, kind


@pytest.mark.parametrize("case", pg_cases.REJECTING, ids=lambda c: "P%d-nbad%d-seed%d" % c)
def test_rejecting_starts_reject_and_stay_clear_of_a_decision(oracle, case):
    """A start stands in pg_cases.REJECTING only if LM rejects a trial on it, no gain ratio of the run comes near the sign
    change that decides a trial, and the history survives perturbations of the start far above what separates two correct
    implementations."""
    g = pg_cases.rejecting(*case)
    _, _, st = oracle.pg_optimize(g, 10)
    print(case, st["trials_hist"], "min |rho| %.2e" % np.abs(st["rho_log"]).min())
    assert max(st["trials_hist"]) > 1
    assert np.abs(st["rho_log"]).min() > 1e-3
    rng = np.random.default_rng(99)
    for _ in range(3):
        poses = g.poses.copy()
        for a in range(1, g.P):
            t = np.abs(poses[a][:3, 3]).max()
            poses[a] = poses[a] @ pg_model.from_mqt(1e-9 * rng.normal(size=6) * np.array([t, t, t, 1, 1, 1]))
        _, _, sp = oracle.pg_optimize(dataclasses.replace(g, poses=poses), 10)
        assert sp["trials_hist"] == st["trials_hist"]


def write_record():
    from oracle import oracle
    oracle.lib()
    rows, scaled = [], []
    for P in (2, 3) + SIZES + (40,):
        for kind in pg_cases.kinds_at(P):
            if P == 40 and kind != "complete":
                continue
            g, ev, (dH, db), (sH, sb) = _measure(oracle, kind, P)
            rows.append(f"| {kind} | {P} | {g.O} | {ev.max() / ev.min():.1e} | {dH:.1e} | {db:.1e} | {_bound(dH):.0e} | {_bound(db):.0e} |")
            scaled.append(f"| {kind} | {P} | {sH:.1e} | {sb:.1e} | {_bound(sH):.0e} | {_bound(sb):.0e} |")
    text = open(RECORD).read() if os.path.exists(RECORD) else "# Pose-graph layouts\n\n<!-- table -->\n"
    head, _, _ = text.partition("<!-- table -->")
    table = ["<!-- table -->", "| kind | P | edges | cond(H free, lambda 0) | dist H | dist b | bound H | bound b |", "|---|---|---|---|---|---|---|---|"]
    table2 = ["", "The same distances in the system's own scale (`pg_model.scaled_distance`):", "",
              "| kind | P | scaled H | scaled b | bound sH | bound sb |", "|---|---|---|---|---|---|"]
    with open(RECORD, "w") as f:
        f.write(head + "\n".join(table + rows + table2 + scaled) + "\n")


if __name__ == "__main__":
    write_record()
