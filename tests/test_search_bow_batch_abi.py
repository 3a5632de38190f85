"""se2gpu_search_by_bow_batch_device at the ABI level, without a device: the symbol, its refusal of a NULL handle, and the C++
mirror (DeviceFrameSet, DeviceFeatureVectorSet, ORBmatcher::SearchByBoWBatchDevice) as plain C++17."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_in_the_table():
    from se2lam_amd import capi
    assert "se2gpu_search_by_bow_batch_device" in capi.SYMBOLS
    assert hasattr(capi.lib(), "se2gpu_search_by_bow_batch_device")


def test_null_handle_is_refused():
    from se2lam_amd import capi
    rc = capi.lib().se2gpu_search_by_bow_batch_device(None, None, None, None, 1024, 6, None, None, None, None, None, None, None,
                                                      1, 0, 0.6, 1, None, None)
    assert rc == capi.ERR_INVALID


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_search_bow_batch")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_search_bow_batch_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
