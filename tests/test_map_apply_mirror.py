"""include/se2lam_amd/MapUpdate.h's host mirror (applyObservations) against tests/map_apply_model.py on every hand-stated case
and on the reference's eleven transitions: integers exact, floats bit for bit.  tests/cpp_map_apply.cpp is compiled with the
host compiler, once as it is and once with -fsanitize=address,undefined (on machines without a device); it has its own main
and loads nothing else."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_apply_cases as mc   # noqa: E402
import map_apply_golden as mg  # noqa: E402
import map_apply_model as mm   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra):
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_map_apply.cpp"), "-o", exe] + extra)
    return exe


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """every case on disk, with the model's answer"""
    tmp = tmp_path_factory.mktemp("map_apply")
    cases = [(name, make()) for name, make in mc.CASES.items()]
    g = mg.Golden()
    c = g.first_case()
    for t in g.transitions:
        c = g.add_case(c, t)
        o = mm.apply(c)
        cases.append(("golden_add_%d" % t["index"], c))
        c = g.erase_case(c, o, t)
        cases.append(("golden_erase_%d" % t["index"], c))
        c = mm.next_case(c, mm.apply(c))
    for name, c in cases:
        mc.dump(c, str(tmp / (name + ".in")))
    return tmp, cases


def _run_all(exe, tmp, cases):
    args = [exe]
    for name, _ in cases:
        args += [str(tmp / (name + ".in")), str(tmp / (name + ".out"))]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout + r.stderr
    assert "%d cases" % len(cases) in r.stdout
    for name, c in cases:
        mc.compare(mc.load_out(c, str(tmp / (name + ".out"))), mm.apply(c), name)


def test_the_mirror_equals_the_model_to_the_bit(dumped):
    tmp, cases = dumped
    assert len(cases) == len(mc.CASES) + 22
    _run_all(_build(tmp, "cpp_map_apply", []), tmp, cases)


def test_the_mirror_is_clean_under_address_and_undefined_behaviour_sanitizers(dumped):
    from se2lam_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible: the sanitizer build of host code runs on machines without a device")
    tmp, cases = dumped
    _run_all(_build(tmp, "cpp_map_apply_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp, cases)
