#!/usr/bin/env python
"""Record se2gpu_plane_motion_prior_iso3 on 100 seeded poses -> tests/golden/plane_prior_iso3.npz.

The file pins the host function's results to the bit across changes of where its arithmetic lives (it is shared with the
device kernel k_plane_prior_iso3).  It holds this library's own outputs: run it with the library of the commit whose
results are to be kept, and only then.  No device is used.

    python tools/gen_plane_prior_golden.py [out.npz]
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from se2lam_amd import capi, feat_edge, synth   # noqa: E402

SEED, N = 20250607, 100


def poses(seed=SEED, n=N):
    """n x 12 (R row-major, t): a ground robot's camera poses with roll, pitch and height off the plane, every fourth one
    a large rotation (the non-positive-trace branches of the quaternion conversion)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12))
    for i in range(n):
        ang = rng.uniform(-np.pi, np.pi) if i % 4 == 0 else rng.uniform(-0.2, 0.2)
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        Rtilt = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        yaw = rng.uniform(-np.pi, np.pi)
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        Twb = np.eye(4)
        Twb[:3, :3] = Rz @ Rtilt
        Twb[:3, 3] = rng.uniform(-8000, 8000, 3) * [1, 1, 0.01]   # millimetres, as synth.TBC
        Tbc = np.eye(4)
        Tbc[:3, :3] = np.asarray(synth.RBC, np.float64).reshape(3, 3)
        Tbc[:3, 3] = synth.TBC
        out[i] = feat_edge.pose12(Twb @ Tbc)
    return out


def run(Twc12, tbc, xrot, yrot, zinfo):
    meas, info = np.zeros((len(Twc12), 12)), np.zeros((len(Twc12), 36))
    for i in range(len(Twc12)):
        capi.check(capi.lib().se2gpu_plane_motion_prior_iso3(Twc12[i].ctypes.data, tbc.ctypes.data, xrot, yrot, zinfo,
                                                             meas[i].ctypes.data, info[i].ctypes.data))
    return meas, info


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "tests", "golden", "plane_prior_iso3.npz")
    Twc12, tbc = poses(), feat_edge.Tbc12()
    xrot, yrot, zinfo = float(synth.PLANEMOTION_XROT_INFO), float(synth.PLANEMOTION_XROT_INFO), float(synth.PLANEMOTION_Z_INFO)
    meas, info = run(Twc12, tbc, xrot, yrot, zinfo)
    np.savez(out, Twc12=Twc12, Tbc12=tbc, infos=np.array([xrot, yrot, zinfo]), meas12=meas, info36=info)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
