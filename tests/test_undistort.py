"""Camera undistortion in front of the extractor: the first step of Frame::Frame (cv::undistort) on the device, and its host
companions cv::undistortPoints and Frame::computeBoundUn.

The expected values come from tests/undistort_model.py, a numpy model written from the arithmetic DESIGN.md states
("Camera undistortion"), independently of the C++.  The host functions need no device; the GPU tests hold the remap kernel
to the model exactly, on uniform noise (no two neighbours alike: the worst case for interpolation weights).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import undistort_model as um

SIZES = [(120, 160), (93, 157), (480, 640)]     # stripes of 25, 26 and 6 rows, each with a partial last stripe
DISTS = {
    "D0": [0.0, 0.0, 0.0, 0.0],
    "D4": [-0.28, 0.07, 1.2e-4, -2.3e-5],
    "D5": [-0.30, 0.10, 5e-4, -4e-4, -0.015],
    "D8": [0.12, -0.2, 1e-3, 1e-3, 0.05, 0.01, -0.02, 0.003],
}


def camera(rows, cols, name):
    """fx about 0.82 cols, the principal point near (not at) the centre; every value rounded to float once, here"""
    return um.Camera(0.82 * cols, 0.83 * cols, 0.5 * cols + 1.7, 0.5 * rows - 2.3, DISTS[name])


def noise(rows, cols, seed, n=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, cols) if n is None else (n, rows, cols), dtype=np.uint8)


# model results are computed once per (size, coefficients) and shared; nothing modifies them
_cache = {}


def model_map(rows, cols, name):
    key = (rows, cols, name)
    if key not in _cache:
        cam = camera(rows, cols, name)
        _cache[key] = (cam,) + um.undistort_map(cam, rows, cols)
    return _cache[key]


def model_undistort(rows, cols, name, img):
    _, xy, frac = model_map(rows, cols, name)
    return um.remap(img, xy, frac)


# ---------------------------------------------------------------------------------------------------------------
# host functions (no device)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DISTS))
@pytest.mark.parametrize("rows,cols", SIZES)
def test_map_equals_the_model(rows, cols, name):
    from se2lam_amd import orb
    cam, xy, frac = model_map(rows, cols, name)
    got_xy, got_frac = orb.undistort_map(cam.K, cam.D, rows, cols)
    assert got_xy.dtype == np.int16 and got_frac.dtype == np.uint16
    assert np.array_equal(got_xy, xy) and np.array_equal(got_frac, frac)


@pytest.mark.parametrize("rows,cols", SIZES)
def test_zero_distortion_is_the_identity_map(rows, cols):
    from se2lam_amd import orb
    cam = camera(rows, cols, "D0")
    xy, frac = orb.undistort_map(cam.K, cam.D, rows, cols)
    iu = xy[..., 0].astype(np.int64) * 32 + (frac & 31)
    iv = xy[..., 1].astype(np.int64) * 32 + (frac >> 5)
    assert np.array_equal(iu, np.broadcast_to(32 * np.arange(cols)[None, :], (rows, cols)))
    assert np.array_equal(iv, np.broadcast_to(32 * np.arange(rows)[:, None], (rows, cols)))


@pytest.mark.parametrize("name", list(DISTS))
@pytest.mark.parametrize("rows,cols", SIZES)
def test_map_is_the_rounded_definition(rows, cols, name):
    """every entry within half a quantisation step (1/64 px) of the FP64 definition fed the same float-rounded K and D"""
    from se2lam_amd import orb
    cam = camera(rows, cols, name)
    xy, frac = orb.undistort_map(cam.K, cam.D, rows, cols)
    u, v = um.definitional_map(cam, rows, cols)
    assert np.abs(u).max() < 32000 and np.abs(v).max() < 32000      # no entry was narrowed
    iu = xy[..., 0].astype(np.float64) * 32 + (frac & 31)
    iv = xy[..., 1].astype(np.float64) * 32 + (frac >> 5)
    eu, ev = np.abs(iu / 32 - u).max(), np.abs(iv / 32 - v).max()
    print("max |map - definition| px:", eu, ev)
    assert eu <= 1 / 64 + 1e-9 and ev <= 1 / 64 + 1e-9


@pytest.mark.parametrize("name", list(DISTS))
def test_points_and_bounds_equal_the_model(name):
    from se2lam_amd import orb
    for rows, cols in SIZES:
        cam = camera(rows, cols, name)
        rng = np.random.default_rng(rows)
        pts = np.concatenate([rng.uniform(-20, cols + 20, (200, 1)), rng.uniform(-20, rows + 20, (200, 1))], 1).astype(np.float32)
        pts = np.concatenate([pts, np.array([[0, 0], [cols, 0], [0, rows], [cols, rows], [cam.cx, cam.cy]], np.float32)])
        got = orb.undistort_points(cam.K, cam.D, pts)
        want = um.undistort_points(cam, pts)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        b = orb.frame_bounds_un(cam.K, cam.D, rows, cols)
        got_b = np.array([b.min_x, b.min_y, b.max_x, b.max_y], np.float32)
        assert np.array_equal(got_b.view(np.uint32), um.frame_bounds_un(cam, rows, cols).view(np.uint32))
        if name == "D0":
            assert np.array_equal(got_b, np.array([0, 0, cols, rows], np.float32))
        else:
            assert not np.array_equal(got_b, np.array([0, 0, cols, rows], np.float32))


def test_bounds_shortcut_looks_at_k1_only():
    """Frame::computeBoundUn returns the image rectangle when D[0] == 0, whatever the other coefficients are"""
    from se2lam_amd import orb
    cam = um.Camera(131.2, 132.8, 81.7, 57.7, [0.0, 0.07, 1e-3, -1e-3, 0.02])
    b = orb.frame_bounds_un(cam.K, cam.D, 120, 160)
    assert (b.min_x, b.min_y, b.max_x, b.max_y) == (0.0, 0.0, 160.0, 120.0)
    assert np.array_equal(um.frame_bounds_un(cam, 120, 160), np.array([0, 0, 160, 120], np.float32))
    # ... while the points themselves do move
    p = orb.undistort_points(cam.K, cam.D, [[0, 0]])
    assert np.array_equal(p, um.undistort_points(cam, [[0, 0]])) and abs(p[0, 0]) > 0.05


def test_refusals():
    from se2lam_amd import capi
    lib = capi.lib()
    K = camera(120, 160, "D4").K
    xy = np.zeros((120, 160, 2), np.int16)
    fr = np.zeros((120, 160), np.uint16)
    pts = np.zeros((4, 2), np.float32)
    b = capi.FrameBounds()

    def calls(cam):
        c = None if cam is None else C.byref(cam)
        return [lib.se2gpu_undistort_map(c, 120, 160, xy.ctypes.data, fr.ctypes.data),
                lib.se2gpu_undistort_points(c, pts.ctypes.data, 4, pts.ctypes.data),
                lib.se2gpu_frame_bounds_un(c, 120, 160, C.byref(b))]
    good = capi.Camera.from_KD(K, DISTS["D4"])
    assert calls(good) == [capi.OK] * 3
    for nd in (0, 1, 3, 6, 7, 9, 12, 14, -4):
        bad = capi.Camera.from_KD(K, DISTS["D4"])
        bad.nd = nd
        assert calls(bad) == [capi.ERR_INVALID] * 3, nd
    bad = capi.Camera.from_KD(K, DISTS["D4"])
    bad.fx = 0.0
    assert calls(bad) == [capi.ERR_INVALID] * 3
    assert calls(None) == [capi.ERR_INVALID] * 3
    for i, v in ((0, np.nan), (3, np.inf), (1, -np.inf)):      # a coefficient that is no number never reaches the rounding
        bad = capi.Camera.from_KD(K, DISTS["D4"])
        bad.d[i] = v
        assert calls(bad) == [capi.ERR_INVALID] * 3, (i, v)
    bad = capi.Camera.from_KD(K, DISTS["D4"])
    bad.cx = np.nan
    assert calls(bad) == [capi.ERR_INVALID] * 3
    ok = capi.Camera.from_KD(K, DISTS["D4"])
    ok.d[6] = np.nan                                           # beyond nd: not part of the camera
    assert calls(ok) == [capi.OK] * 3
    g = C.byref(good)
    assert lib.se2gpu_undistort_map(g, 120, 160, None, fr.ctypes.data) == capi.ERR_INVALID
    assert lib.se2gpu_undistort_map(g, 120, 160, xy.ctypes.data, None) == capi.ERR_INVALID
    assert lib.se2gpu_undistort_points(g, None, 4, pts.ctypes.data) == capi.ERR_INVALID
    assert lib.se2gpu_undistort_points(g, pts.ctypes.data, 4, None) == capi.ERR_INVALID
    assert lib.se2gpu_frame_bounds_un(g, 120, 160, None) == capi.ERR_INVALID
    assert lib.se2gpu_orb_set_camera(None, g) == capi.ERR_INVALID
    from se2lam_amd import orb
    for rows, cols in ((0, 160), (120, 0), (-1, 160)):
        with pytest.raises(ValueError):
            orb.undistort_map(K, DISTS["D4"], rows, cols)
        assert lib.se2gpu_undistort_map(g, rows, cols, xy.ctypes.data, fr.ctypes.data) == capi.ERR_INVALID


def _cpp_binary(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "se2lam_amd", "lib")
    exe = str(tmp_path / "cpp_undistort")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_undistort_compile.cpp"), "-o", exe, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    return exe


def _run_cpp(tmp_path):
    r = subprocess.run([_cpp_binary(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("BOUNDS")][0]
    got = np.array(line.split()[1:], np.float32)
    assert np.array_equal(got, um.frame_bounds_un(camera(480, 640, "D5"), 480, 640))
    return r.stdout


def test_cpp_mirrors_compile_and_run(tmp_path):
    """include/se2lam_amd/Frame.h (computeBoundUn, undistortPoints) and ORBextractor::setCamera: the bounds equal the model's"""
    _run_cpp(tmp_path)


# ---------------------------------------------------------------------------------------------------------------
# the remap kernel in front of the pyramid
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """one extractor for the small sizes (4 levels, so that 93 x 157 still has a valid top level)"""
    from se2lam_amd import orb
    return orb.ORBextractor(nfeatures=300, nlevels=4, max_rows=120, max_cols=160, max_batch=3)


def _level0(ex, rows, cols, name, seed):
    cam = camera(rows, cols, name)
    img = noise(rows, cols, seed)
    ex.set_camera(cam.K, cam.D)
    ex(img)
    return ex.debug_level(0, 0), model_undistort(rows, cols, name, img)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D4", "D5", "D8"])
@pytest.mark.parametrize("rows,cols", SIZES[:2])       # 93 x 157: the unaligned path of k_level0, rows that are no multiple of 4
def test_level0_is_the_undistorted_image(small, rows, cols, name):
    got, want = _level0(small, rows, cols, name, seed=rows + len(name))
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
def test_level0_is_the_undistorted_image_vga():
    from se2lam_amd import orb
    got, want = _level0(orb.ORBextractor(), 480, 640, "D5", seed=5)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SIZES[:2])
def test_border_is_exercised(small, rows, cols):
    """D8 pulls the corners in: part of the output maps outside the source (constant 0) and part straddles its edge"""
    _, xy, _ = model_map(rows, cols, "D8")
    sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
    outside = (sx < -1) | (sx >= cols) | (sy < -1) | (sy >= rows)      # all four neighbours outside the image
    assert outside.mean() >= 0.01, outside.mean()
    assert ((sx == -1) | (sy == -1)).any() and ((sx == cols - 1) | (sy == rows - 1)).any()
    got, want = _level0(small, rows, cols, "D8", seed=8)
    assert np.array_equal(got, want)
    assert not got[outside].any() and got[~outside].any()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SIZES[:2])       # 93 x 157: frames of a batch whose rows are padded (cols % 4 != 0)
def test_batch_path_composes_undistort_and_extract(rows, cols):
    """three distinct raw frames, one camera: level 0 of each is the model's image, and key points / descriptors are those of
    a camera-less extractor fed the model's undistorted images - the composition Frame::Frame performs"""
    from se2lam_amd import orb
    name = "D5"
    cam = camera(rows, cols, name)
    rng = np.random.default_rng(3)
    # blocks of 4 x 4 pixels of noise: corners for FAST (per-pixel noise has hardly any 9-arcs), still no flat area
    raw = np.stack([np.kron(rng.integers(0, 256, ((rows + 3) // 4, (cols + 3) // 4), dtype=np.uint8),
                            np.ones((4, 4), np.uint8))[:rows, :cols] ^
                    rng.integers(0, 16, (rows, cols), dtype=np.uint8) for _ in range(3)])
    want = np.stack([model_undistort(rows, cols, name, f) for f in raw])
    ex = orb.ORBextractor(nfeatures=300, nlevels=4, max_rows=rows, max_cols=cols, max_batch=3)
    ex.set_camera(cam.K, cam.D)
    got = ex.extract_batch(raw)
    for f in range(3):
        assert np.array_equal(ex.debug_level(f, 0), want[f]), f
    plain = orb.ORBextractor(nfeatures=300, nlevels=4, max_rows=rows, max_cols=cols, max_batch=3)
    ref = plain.extract_batch(want)
    assert sum(len(k) for k, _ in ref) > 100
    for (k, d), (kr, dr) in zip(got, ref):
        assert np.array_equal(k, kr) and np.array_equal(d, dr)
    assert any(not np.array_equal(k, kr) for (k, _), (kr, _) in zip(plain.extract_batch(raw), ref))   # the camera matters


@pytest.mark.gpu
def test_identity_camera_end_to_end(synth):
    """set_camera(K, 0) runs the kernel over the identity map: byte-identical output; set_camera(None) puts the plain path back"""
    from se2lam_amd import orb
    img = synth.frame(0)
    rows, cols = img.shape
    cam = camera(rows, cols, "D0")
    k0, d0 = orb.ORBextractor()(img)
    assert len(k0) > 500
    ex = orb.ORBextractor()
    ex.set_camera(cam.K, cam.D)
    k1, d1 = ex(img)
    assert np.array_equal(k1, k0) and np.array_equal(d1, d0)
    assert np.array_equal(ex.debug_level(0, 0), img)
    cam5 = camera(rows, cols, "D5")
    ex.set_camera(cam5.K, cam5.D)
    k2, _ = ex(img)
    assert not np.array_equal(k2, k0)
    ex.set_camera(None)
    k3, d3 = ex(img)
    assert np.array_equal(k3, k0) and np.array_equal(d3, d0)
    assert np.array_equal(ex.debug_level(0, 0), img)


@pytest.mark.gpu
def test_one_handle_across_image_sizes(small):
    """120 x 160, then 93 x 157, then 120 x 160 again with one camera: the maps follow the image size"""
    cam = camera(120, 160, "D4")       # ONE camera for both sizes (the principal point is off-centre at 93 x 157)
    small.set_camera(cam.K, cam.D)
    for i, (rows, cols) in enumerate([(120, 160), (93, 157), (120, 160)]):
        img = noise(rows, cols, 40 + i)
        small(img)
        assert np.array_equal(small.debug_level(0, 0), um.undistort(cam, img)), (i, rows, cols)


@pytest.mark.gpu
def test_cpp_extractor_with_a_camera(tmp_path):
    """ORBextractor::setCamera / clearCamera of the C++ mirror on the device (tests/cpp_undistort_compile.cpp)"""
    assert "OK (device:" in _run_cpp(tmp_path)
