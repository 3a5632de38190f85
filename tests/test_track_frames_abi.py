"""se2gpu_track_frames_batch_device without a device: the exported symbol, every argument check, and the C++ mirror
(TrackGeometry::TrackFramesBatchDevice and needNewKFByCounts of include/se2lam_amd/Track.h) as plain C++17."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ("d_kps_un", "d_counts", "d_pair_ref", "d_pair_cur", "d_Trc", "d_P", "P_ref", "d_matches12", "d_matched12", "d_local_pos",
            "d_good_prl", "d_info")


def test_symbol_is_exported_and_in_the_table():
    from se2lam_amd import capi, track
    assert "se2gpu_track_frames_batch_device" in capi.SYMBOLS
    assert hasattr(capi.lib(), "se2gpu_track_frames_batch_device")
    assert len(track.TRACK_FRAMES_INFO) == 8 and hasattr(track.Track, "track_frames_batch_device")


def _call(h, ptr, cap=512, nframes=4, npairs=3, kf_observed=None, view_pos=None, flags=None, min_degree=2, **nulls):
    """the entry point with `ptr` for every required pointer except those named in `nulls`"""
    from se2lam_amd import capi
    a = {name: ptr for name in REQUIRED}
    a.update(nulls)
    return capi.lib().se2gpu_track_frames_batch_device(h, a["d_kps_un"], a["d_counts"], cap, nframes, kf_observed, view_pos,
                                                       a["d_pair_ref"], a["d_pair_cur"], npairs, a["d_Trc"], a["d_P"], flags,
                                                       a["P_ref"], a["d_matches12"], 500.0, 8000.0, min_degree, a["d_matched12"],
                                                       a["d_local_pos"], a["d_good_prl"], a["d_info"])


def test_arguments_are_refused_before_anything_is_touched():
    """The checks come before the first use of the handle or of a device, so a stand-in address serves for both here; no call
    below gets past them."""
    from se2lam_amd import capi
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert _call(None, p) == capi.ERR_INVALID
    for name in REQUIRED:
        assert _call(p, p, **{name: None}) == capi.ERR_INVALID, name
    assert _call(p, p, kf_observed=p) == capi.ERR_INVALID                 # d_kf_observed without d_view_pos
    assert _call(p, p, npairs=0) == capi.ERR_INVALID
    assert _call(p, p, cap=0) == capi.ERR_INVALID
    assert _call(p, p, nframes=0) == capi.ERR_INVALID
    assert _call(p, p, npairs=-3) == capi.ERR_INVALID
    for deg in (0, 5, -1):
        assert _call(p, p, min_degree=deg) == capi.ERR_INVALID
    assert _call(p, p, npairs=65536) == capi.ERR_CAPACITY                 # the limits of the loop-verification call
    assert _call(p, p, cap=65537) == capi.ERR_CAPACITY
    assert _call(p, p, kf_observed=p, view_pos=p, flags=p, cap=65537) == capi.ERR_CAPACITY
    assert _call(p, p, cap=65537, min_degree=9) == capi.ERR_INVALID
    assert b"track_frames_batch" in capi.lib().se2gpu_last_error()


def test_cpp_mirror_compiles_and_runs(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    out = str(tmp_path / "cpp_track_frames")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_track_frames_compile.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
