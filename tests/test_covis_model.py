"""The set model of the covisibility calls (tests/covis_model.py) held to hand-worked cases (tests/covis_cases.py), and the
header's host functions (include/se2lam_amd/Covisibility.h, through tests/cpp_covis.cpp) held to the model on the same cases
and on seeded random maps.  Everything is an integer or a single IEEE operation: every comparison is exact."""
import numpy as np
import pytest

import covis_cases as cc
import covis_model as cm

HAND = cc.hand_cases()


def _run(model, call):
    if call[0] == "pairs":
        o = model.pairs([call[1]], [call[2]], 0.3, 0.1, list_cap=64)
        return dict(out=tuple(o["out"][0]), ratio=o["ratio"][0], common=[int(p) for p in o["common"][0, :, 0] if p != cm.ISENT])
    o = model.refset([call[1]], [0, len(call[2])], call[2], call[3], 0.8)
    return dict(out=tuple(o["out"][0]), ratio=o["ratio"][0], ret=model.refset_points(call[1], call[2], call[3])[0])


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case_against_the_model(name):
    t, call, want = HAND[name]
    got = _run(cm.Model(*cc.tables(t)), call)
    assert got["out"] == want["out"]
    assert cm.same_floats(np.asarray(got["ratio"]), np.asarray(want["ratio"], np.float32 if call[0] == "pairs" else np.float64))
    for k in ("common", "ret"):
        if k in want:
            assert got[k] == want[k]


def test_the_roundings_the_hand_cases_rest_on():
    assert np.float32(0.3) * np.float32(10) == np.float32(3)          # a tie, to even
    assert np.float32(0.3) * np.float32(3) < np.float32(1)
    assert 0.1 * 30.0 == 3.0 and 4.0 / 5.0 == 0.8                  # 0.1 * 30 = 3 + 1.7e-16 rounds to 3.0: 3 > 3 is false
    # the double product would have decided the first case the other way: the float arithmetic is what is tested
    assert float(np.float32(0.3)) * 10.0 > 3.0


def test_frame_listed_twice_counts_once_and_keeps_its_first_entry():
    t = HAND["frame_twice"][0]
    m = cm.Model(*cc.tables(t))
    assert m.size_obs().tolist() == [2, 2] and len(t["obs_frame"]) == 5
    o = m.pairs([0], [1], list_cap=4)
    assert o["common"][0, :2].tolist() == [[0, 0, 1], [1, 3, 4]] and (o["common"][0, 2:] == cm.ISENT).all()


def test_model_rules_on_an_irregular_map():
    t = cc.random_map(3, 5, 129)
    m = cm.Model(*cc.tables(t))
    assert (np.diff(t["mp_ptr"]) < 0).any() and (t["obs_frame"] < 0).any() and (t["obs_frame"] >= 5).any()
    b = m.bits()
    assert b.shape == (7, 3)
    assert [sum(bin(int(w)).count("1") for w in row) for row in b[:5]] == m.size_obs().tolist()
    assert (b[:, -1] >> np.uint64(1)).max() == 0                      # bits past m = 129 are zero
    pa, pb = cc.pair_list(0, 5)
    o = m.pairs(pa, pb, list_cap=3)
    assert o["out"][-4:].tolist() == [[-1, 0, 0, 0]] * 4 and (o["ratio"][-4:] == cm.SENT).all() and (o["common"][-4:] == cm.ISENT).all()
    for i in range(5):                                                # (a, a): the not-null points of a
        assert o["out"][6 * i, 0] == len([p for p in m.sets[i] if p in m.notnull]) and o["out"][6 * i, 1] == o["out"][6 * i, 2]
    assert (o["out"][:-4, 0] > 3).any()                               # truncation happens
    kf, rp, ri = cc.job_list(1, 5, 12, 9)
    r = m.refset(kf, rp, ri, 2, 0.8)
    assert r["out"][-2:].tolist() == [[-1, 0, 0]] * 2 and (r["ratio"][-2:] == cm.SENT).all()
    assert r["out"][0, 0] == 0                                        # an empty reference list


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return cc.cpp_build(tmp_path_factory.mktemp("covis"))


def test_header_host_functions_equal_the_model(program, tmp_path):
    jobs = [(t, [call]) for t, call, _ in HAND.values()]
    for seed, (nf, m, irregular) in enumerate([(2, 1, False), (5, 65, True), (5, 129, True), (8, 60, False), (70, 300, True)]):
        t = cc.random_map(seed, nf, m, irregular=irregular)
        rng = np.random.default_rng(100 + seed)
        calls = [("pairs", int(a), int(b)) for a, b in rng.integers(0, nf, (12, 2))] + [("pairs", nf - 1, nf - 1)]
        for k in (1, 2, 3, 7):
            for _ in range(3):
                calls.append(("refset", int(rng.integers(0, nf)), [int(x) for x in rng.integers(-1, nf + 1, rng.integers(0, 12))], k))
        jobs.append((t, calls))
    assert cc.against_header(program, tmp_path / "cases.txt", jobs) == len(HAND) + 5 * 25
