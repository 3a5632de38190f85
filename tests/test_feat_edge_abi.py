"""se2gpu_feat_edge_batch without a device: the exported symbol, every argument refusal (they come before the first use of a
device), and the C++ mirror include/se2lam_amd/FeatEdge.h as plain C++17 with the reference's constants."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import feat_edge_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_in_the_table():
    from se2lam_amd import capi
    assert "se2gpu_feat_edge_batch" in capi.SYMBOLS
    assert hasattr(capi.lib(), "se2gpu_feat_edge_batch")
    with open(os.path.join(ROOT, "include", "se2gpu.h")) as f:
        assert "int se2gpu_feat_edge_batch(" in f.read()


ARGS = ("npairs", "mode", "iters", "min_points", "kf12", "Tbc12", "xrot", "yrot", "zinfo", "mp_ptr", "mp_xyz", "m_z", "m_info",
        "huber_delta", "outlier_chi2", "kf12_out", "mp_xyz_out", "outlier", "edge_chi2", "info4", "stats", "z_out12", "info_out36")


@pytest.fixture(scope="module")
def valid():
    from se2lam_amd import capi, feat_edge as fe
    pairs = [fc.as_tuple(fc.make_pair(4, 0)), fc.as_tuple(fc.make_pair(3, 1))]
    kf, mp_ptr, mp, z, info = fe.flatten(pairs)
    keep = dict(kf12=kf, Tbc12=fe.Tbc12(), mp_ptr=mp_ptr, mp_xyz=mp, m_z=z, m_info=info, kf12_out=np.zeros((2, 24)),
                mp_xyz_out=np.zeros((7, 3)), outlier=np.zeros(7, np.uint8), edge_chi2=np.zeros((7, 2)), info4=np.zeros((2, 4), np.int32),
                stats=np.zeros(2 * 1400, np.uint8), z_out12=np.zeros((2, 12)), info_out36=np.zeros((2, 36)))
    a = dict(npairs=2, mode=fe.MATCH, iters=30, min_points=3, xrot=1e6, yrot=1e6, zinfo=1.0, huber_delta=5.99, outlier_chi2=5.0)
    a.update({k: v.ctypes.data for k, v in keep.items()})
    return a, keep


def _call(a, **over):
    from se2lam_amd import capi
    b = dict(a)
    b.update(over)
    return capi.lib().se2gpu_feat_edge_batch(*[b[k] for k in ARGS])


def test_arguments_are_refused_before_any_device_use(valid):
    from se2lam_amd import capi
    a, keep = valid
    for name in ("kf12", "Tbc12", "mp_ptr", "mp_xyz", "m_z", "m_info", "kf12_out", "mp_xyz_out", "outlier", "edge_chi2", "info4",
                 "z_out12", "info_out36"):
        assert _call(a, **{name: None}) == capi.ERR_INVALID, name
    assert _call(a, npairs=-1) == capi.ERR_INVALID
    assert _call(a, mode=2) == capi.ERR_INVALID
    for iters in (0, -3, 65):
        assert _call(a, iters=iters) == capi.ERR_INVALID
    for ptr in ([1, 4, 7], [0, 4, 3]):                  # not starting at 0; decreasing
        bad = np.array(ptr, np.int32)
        assert _call(a, mp_ptr=bad.ctypes.data) == capi.ERR_INVALID
    assert _call(a, npairs=65536) == capi.ERR_CAPACITY   # refused before mp_ptr is walked
    assert b"65535" in capi.lib().se2gpu_last_error()


def test_valid_arguments_reach_the_device_check(valid):
    """with nothing to refuse the call needs a device: without one it says so (stats may be NULL), with one it runs"""
    from se2lam_amd import capi
    a, keep = valid
    rc = _call(a, stats=None)
    if capi.device_count() > 0:
        assert rc == capi.OK and keep["info4"][:, 0].tolist() == [0, 0]
    else:
        assert rc == capi.ERR_NO_DEVICE
        assert _call(a, npairs=0) == capi.ERR_NO_DEVICE


def test_python_mirror_has_the_reference_defaults():
    from se2lam_amd import feat_edge as fe
    assert (fe.COVIS_ITERS, fe.COVIS_MIN_POINTS, fe.MATCH_ITERS, fe.MATCH_MIN_POINTS, fe.HUBER_DELTA, fe.OUTLIER_CHI2) == (15, 10, 30, 3, 5.99, 5.0)


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_feat_edge")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_feat_edge_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
