"""tests/ba_ab.py's comparator and tests/ba_cases.py's env(): they guard every A/B module of the BA kernels, so that they fail
when they must is pinned here, on hand-made arrays (no device, no library)."""
import os

import numpy as np
import pytest

from ba_ab import assert_equal_runs
from ba_cases import env


def _run():
    return {"a/chi2": np.array([1.5, np.nan, -0.0]), "a/trials": np.array([1, 2, 3], np.int64), "a/grid": np.array([4, 4, 4], np.int64),
            "b/chi2": np.array([[2.0, 3.0]]), "batch/path": np.array([1], np.int64)}


CHANGES = {
    "a missing key": lambda r: r.pop("b/chi2"),
    "a shape change": lambda r: r.update({"b/chi2": r["b/chi2"].reshape(2, 1)}),
    "a dtype change": lambda r: r.update({"a/trials": r["a/trials"].astype(np.int32)}),
    "0.0 against -0.0": lambda r: r["a/chi2"].__setitem__(2, 0.0),
    "one mantissa bit": lambda r: r["a/chi2"].__setitem__(0, np.nextafter(1.5, 2.0)),     # 1.5 + 2^-52: the lowest bit flipped
}


@pytest.mark.parametrize("what", list(CHANGES))
def test_comparator_raises_on(what):
    new, old = _run(), _run()
    assert_equal_runs(new, old)                      # equal NaNs (the same payload) included
    CHANGES[what](new)
    if what == "a dtype change":
        assert np.array_equal(new["a/trials"], old["a/trials"])
    if what == "0.0 against -0.0":
        assert new["a/chi2"][2] == old["a/chi2"][2]
    for a, b in ((new, old), (old, new)):
        with pytest.raises(AssertionError):
            assert_equal_runs(a, b)


def test_comparator_lists_every_differing_key(capsys):
    new, old = _run(), _run()
    new["a/chi2"][0] = 3.0
    new["b/chi2"][0, 1] = 4.0
    with pytest.raises(AssertionError) as e:
        assert_equal_runs(new, old)
    assert "a/chi2" in str(e.value) and "b/chi2" in str(e.value)
    out = capsys.readouterr().out
    assert "differs: a/chi2 max relative difference 1.0" in out and "differs: b/chi2" in out


def test_comparator_leaves_out_what_it_is_told_to():
    old = _run()
    new = _run()
    new["batch/path"][0] = 0
    assert_equal_runs(new, old, skip=("batch/path",))
    new = _run()
    new["a/grid"][1] = 3
    assert_equal_runs(new, old, exempt_suffix=("/grid",))
    new = _run()
    new["b/chi2"][0, 0] = 7.0
    assert_equal_runs(new, old, only="a")
    assert_equal_runs(new, old, only=("a", "batch"))
    for kw in ({"skip": ("a/grid",)}, {"exempt_suffix": ("/grid",)}, {"only": "b"}, {"only": ("batch", "b")}):
        with pytest.raises(AssertionError):
            assert_equal_runs(new, old, **kw)
    with pytest.raises(AssertionError):              # the key sets are compared whatever is left out
        assert_equal_runs({**new, "c/x": np.zeros(1)}, old, only="a")


def test_comparator_hands_special_keys_to_their_rule():
    new, old = _run(), _run()
    new["a/trials"][0] = 9
    seen = []
    assert_equal_runs(new, old, special={"/trials": lambda *a: seen.append(a)})
    assert len(seen) == 1
    k, n, o = seen[0]
    assert k == "a/trials" and n is new["a/trials"] and o is old["a/trials"]

    def rule(k, n, o):
        assert n[0] == o[0], k
    with pytest.raises(AssertionError):
        assert_equal_runs(new, old, special={"/trials": rule})
    assert_equal_runs(new, old, special={"/trials": rule}, only="b")        # a key outside `only` does not reach its rule


@pytest.mark.parametrize("raises", [False, True])
def test_env_restores(monkeypatch, raises):
    monkeypatch.setenv("BA_AB_TEST_SET", "before")
    monkeypatch.setenv("BA_AB_TEST_SET2", "before2")
    monkeypatch.delenv("BA_AB_TEST_UNSET", raising=False)
    try:
        with env(BA_AB_TEST_SET="inside", BA_AB_TEST_SET2=None, BA_AB_TEST_UNSET="x"):
            assert os.environ["BA_AB_TEST_SET"] == "inside" and os.environ["BA_AB_TEST_UNSET"] == "x"
            assert "BA_AB_TEST_SET2" not in os.environ
            if raises:
                raise KeyError("from the body")
    except KeyError:
        assert raises
    else:
        assert not raises
    assert os.environ["BA_AB_TEST_SET"] == "before" and os.environ["BA_AB_TEST_SET2"] == "before2"
    assert "BA_AB_TEST_UNSET" not in os.environ
