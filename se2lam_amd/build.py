"""Build recipe of libse2gpu.so (HIP kernels + C ABI) for gfx950, in-tree.

    python -m se2lam_amd.build [--force]

Each csrc/*.hip is compiled to an object with hipcc (--offload-arch=gfx950) and linked into
se2lam_amd/lib/libse2gpu.so.  The ORB / matcher translation units are compiled with
-ffp-contract=off: their float index arithmetic (x*b + y*a, fastAtan2) must round exactly like
the reference's non-FMA x86 build so descriptors and matches are bit-exact (SURVEY.md §7 hard
part 3).  hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libse2gpu.so")
OBJDIR = os.path.join(LIBDIR, "obj")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")

ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
          "-Wno-unused-result", "-I", INCLUDE]
PER_FILE = {
    "orb.hip": ["-ffp-contract=off"],
    "match.hip": ["-ffp-contract=off"],
    "triangulate.hip": ["-ffp-contract=off"],
    "ransac.hip": ["-ffp-contract=off"],
    "track_frames.hip": ["-ffp-contract=off"],   # triangulate_dlt and the parallax test round as triangulate.hip's, to the bit
    "bow.hip": ["-ffp-contract=off"],        # BowVector values and scores equal the host vocabulary's to the bit
    "voc_train.hip": ["-ffp-contract=off"],  # cut_d = u * sum is one IEEE multiply on host and device
    "mappoint.hip": ["-ffp-contract=off"],   # mMinDist / mMaxDist are IEEE operations, equal to the host's to the bit
    "new_kf.hip": ["-ffp-contract=off"],     # view_info.h: float arithmetic in the reference's order, equal to the host mirror's
    "map_apply.hip": ["-ffp-contract=off"],  # map_normal.h: mNormalVector rounds operation by operation, as the host mirror's
    "covis.hip": ["-ffp-contract=off"],      # the ratios and threshold tests are single IEEE operations, as in the reference
    "sparsify.hip": ["-ffp-contract=off"],   # forward differences with delta 1e-6 decide the result: reproduce them to the bit
    "feat_edge_device.hip": ["-ffp-contract=off"],   # the plane-motion prior's information equals the host function's to the bit
    "local_ba_device.hip": ["-ffp-contract=off"],    # the gathered informations are sums and products rounded one by one, as a numpy model's
    # the gathered values and the plane-motion prior are sums and products rounded one by one, as a numpy model's.  pose_ba.hip keeps
    # the default, so the solver both call (pose_ba_device.h) agrees between them to rounding, not to the bit
    "localizer_ba_device.hip": ["-ffp-contract=off"],
}


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJDIR, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE) if f.endswith(".h")]
    sub = os.path.join(INCLUDE, "se2lam_amd", "VocabularyTree.h")   # the one adapter header a translation unit (bow.hip) includes
    sub2 = os.path.join(INCLUDE, "se2lam_amd", "VocabularyTrain.h")   # voc_train.hip shares its inline functions with the host mirror
    sub3 = os.path.join(INCLUDE, "se2lam_amd", "view_info.h")         # triangulate.hip / new_kf.hip share it with FindCorrespd.h
    sub4 = os.path.join(INCLUDE, "se2lam_amd", "obs_table.h")         # mappoint.hip / new_kf.hip / covis.hip share it with their mirrors
    sub5 = os.path.join(INCLUDE, "se2lam_amd", "map_normal.h")        # map_apply.hip shares it with MapUpdate.h
    headers += [sub, sub2, sub3, sub4, sub5, os.path.abspath(__file__)]
    objs = []
    for src in sources():
        obj = os.path.join(OBJDIR, src[:-4] + ".o")
        objs.append(obj)
        if force or _stale(obj, [os.path.join(CSRC, src)] + headers):
            cmd = [_hipcc()] + COMMON + PER_FILE.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    if force or _stale(LIB, objs):
        cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
