"""The undistortion stage against REAL OpenCV - wherever OpenCV exists.

Two sources, either is enough: a live `import cv2`, or the fixture tests/golden/undistort_pin.npz written by
tools/gen_golden_undistort_cv2.py on a machine that has OpenCV.  Without both these tests are collected and skipped; they
are the hook that pins the arithmetic DESIGN.md restates ("Camera undistortion") the first time the repository is
checked out next to an OpenCV install:

    python tools/gen_golden_undistort_cv2.py && python -m pytest tests/test_undistort_pin.py

OpenCV 3.x must be met exactly; later versions (which may build the map with SIMD float paths) within one grey level.
"""
import importlib.util
import os

import numpy as np
import pytest

import undistort_model as um

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "undistort_pin.npz")


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_undistort_cv2",
                                                  os.path.join(HERE, "..", "tools", "gen_golden_undistort_cv2.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    if not os.path.exists(FIXTURE):
        pytest.importorskip("cv2", reason="no OpenCV here and no tests/golden/undistort_pin.npz (tools/gen_golden_undistort_cv2.py)")
        _tool().main()
    return dict(np.load(FIXTURE, allow_pickle=False))


def _exact(gold):
    return str(gold["cv_version"]).startswith("3.")


def _camera(tool, rows, cols, name):
    K = tool.intrinsics(rows, cols)
    return um.Camera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], tool.DISTS[name])


def test_model_against_cv_undistort():
    gold, tool = _golden(), _tool()
    for rows, cols, name in tool.cases():
        got = um.undistort(_camera(tool, rows, cols, name), tool.raw_image(rows, cols)).astype(int)
        want = gold[f"{rows}x{cols}_{name}_undistorted"].astype(int)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= (0 if _exact(gold) else 1), (rows, cols, name)


def test_library_points_against_cv_undistort_points():
    from se2lam_amd import orb
    gold, tool = _golden(), _tool()
    for rows, cols, name in tool.cases():
        cam = _camera(tool, rows, cols, name)
        got = orb.undistort_points(cam.K, cam.D, tool.points(rows, cols))
        want = gold[f"{rows}x{cols}_{name}_points"]
        if _exact(gold):
            assert np.array_equal(got, want), (rows, cols, name)
        else:   # the same five iterations by default, but not necessarily the same expression order: float results up to
            #     ~700 px have an ulp of 6e-5, a handful of them is the allowance
            assert np.abs(got - want).max() <= 1e-3, (rows, cols, name)


@pytest.mark.gpu
def test_hip_undistort_against_cv_fixture():
    """level 0 of an extractor that carries the camera against real OpenCV's cv::undistort"""
    from se2lam_amd import orb
    gold, tool = _golden(), _tool()
    for rows, cols, name in tool.cases():
        cam = _camera(tool, rows, cols, name)
        ex = orb.ORBextractor(nfeatures=300, nlevels=4, max_rows=rows, max_cols=cols)
        ex.set_camera(cam.K, cam.D)
        ex(tool.raw_image(rows, cols))
        got = ex.debug_level(0, 0).astype(int)
        want = gold[f"{rows}x{cols}_{name}_undistorted"].astype(int)
        assert np.abs(got - want).max() <= (0 if _exact(gold) else 1), (rows, cols, name)
