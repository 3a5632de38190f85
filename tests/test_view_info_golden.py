"""calcSE3toXYZInfo against the reference itself: tests/golden/view_info_ref.npz holds 200 inputs (depth 0.8-30, 0.5-35 degrees
off the axis, baselines 0.05-1.5, identity and general poses, several fx) and the two informations the reference's own
Track::calcSE3toXYZInfo returned for them (tools/gen_view_info_golden.cpp, linked against the oracle's build of Track.cpp).
The cv::Mat arithmetic behind the fixture is the stand-in's of oracle/_shim, not OpenCV's.  The test reads only the fixture.

The header's host function repeats the reference's operations with the same C library, compiled without contraction as the
reference is: it must equal the fixture to the bit.  The float32 restatement may differ by numpy's arcsin / sin / cos alone: a
few units of 2^-24 on the rotation, bounded here by 1e-6 of a matrix's largest entry (measured 2.2e-7, 141 of 200 cases
equal to the bit).  The FP64 layer is held to the fixture by 1e-5: float rounding times
the 1 / sinParallax of the narrowest case (0.05 over 30)."""
import os
import subprocess

import numpy as np
import pytest

import new_kf_model as nk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "view_info_ref.npz"))
    assert len(z["fx"]) == 200 and z["info1"].dtype == np.float64
    assert np.isfinite(z["info1"]).all() and np.isfinite(z["info2"]).all()
    return z


def _args(z, i):
    return z["xyz1"][i], z["Twc1"][i], z["Tcw2"][i], z["Twc2"][i], z["fx"][i]


@pytest.mark.parametrize("L,bound", [(nk.L32, 1e-6), (nk.L64, 1e-5)])
def test_model_equals_the_reference(golden, L, bound):
    worst = 0.0
    for i in range(200):
        a, b, _ = L.se3_to_xyz_info(*_args(golden, i))
        worst = max(worst, nk.rel_err_mat(a.ravel(), golden["info1"][i])[0], nk.rel_err_mat(b.ravel(), golden["info2"][i])[0])
    print("worst", worst)
    assert worst <= bound


def test_information_is_symmetric_and_positive(golden):
    for k in ("info1", "info2"):
        M = golden[k].reshape(-1, 3, 3)
        assert np.abs(M - M.transpose(0, 2, 1)).max() <= 1e-5 * np.abs(M).max()
        assert (np.linalg.eigvalsh((M + M.transpose(0, 2, 1)) / 2) > 0).all()


def test_host_function_equals_the_reference(golden, tmp_path):
    out = str(tmp_path / "cpp_find_correspd")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_find_correspd.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()
    lines = []
    for i in range(200):
        x, w1, t2, w2, fx = _args(golden, i)
        lines.append("I " + " ".join(map(str, bits(x) + bits(w1) + bits(t2) + bits(w2) + bits([fx]) + bits([0, 0, 1]) + [0, 0] + bits([0, 1]))))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([out, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = r.stdout.splitlines()
    assert len(rows) == 200
    got = np.array([[int(v) for v in ln.split()[:18]] for ln in rows], np.uint32).view(np.float32)
    # the fixture holds the reference's floats widened to double: equal to the bit means equal after the same widening
    assert np.array_equal(got[:, :9].astype(np.float64), golden["info1"]) and np.array_equal(got[:, 9:].astype(np.float64), golden["info2"])
