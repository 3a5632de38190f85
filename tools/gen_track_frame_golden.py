#!/usr/bin/env python3
"""Writes tests/golden/track_frame_ref.npz: what Track::doTriangulate of THE REFERENCE ITSELF - its own sources compiled
unmodified in oracle/_ref (oracle/Makefile, target `ref`) - gives on the scenes of tests/test_track_frame_model.py
(GOLDEN_SCENES over tests/test_triangulate.scene).  Data only: per scene the positions (mLocalMPs, (-1, -1, -1) where the
reference did not touch them), mvbGoodPrl, the updated mMatchIdx and {mnGoodPrl, nTrackedOld}.  The model of
se2gpu_track_frames_batch_device is held to them on machines where the compiled reference is absent.

    python tools/gen_track_frame_golden.py          (needs the reference's sources: builds oracle/_ref first)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref  # noqa: E402
import test_track_frame_model as T  # noqa: E402

OUT = T.GOLDEN


def build():
    arr = {}
    K = np.array([[400.0, 0, 320.0], [0, 400.0, 240.0], [0, 0, 1]], np.float32)
    for n, seed in T.GOLDEN_SCENES:
        _, (k1, k2, match, has_obs, X, Tcr) = T.golden_case(n, seed)
        pos, good, m, ng, nold = ref.track_triangulate(K, k1, k2, match, has_obs, X, Tcr, 500.0, 8000.0)
        tag = "n%d_s%d_" % (n, seed)
        arr[tag + "pos"], arr[tag + "good"], arr[tag + "match"] = pos, good, m
        arr[tag + "counts"] = np.array([ng, nold], np.int32)
    np.savez_compressed(OUT, **arr)
    return arr


if __name__ == "__main__":
    arr = build()
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(arr), "arrays")
