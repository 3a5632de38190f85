#!/usr/bin/env python3
"""Vocabulary training on the device (se2gpu_voc_train) against the host mirror ORBVocabulary::create (g++ -O2, one thread) on
the same input: the descriptors of 256 of the bench's synthetic frames, about 1,000 each, extracted on the device and handed
over in device memory; k = 10, L = 5.

    python tools/voc_train_bench.py [--quick] [--out profiles/voc_train] [--commit ID]

The device time is the wall time of the synchronous call (it ends in a stream synchronise), after one warm-up call: `--runs`
windows of `--calls` back-to-back calls each, so that a timed window lasts a good fraction of a second; reported per call as the
median over the windows with the fastest and slowest window.  The host time is the mirror's create alone, timed inside the driver.  The
device result is compared with the mirror's bit for bit before anything is reported.  The per-kernel table comes from a
separate call with the library's profile hooks on (HIP events around every launch: that call is slower and is not the one
timed).  Writes <out>.md and <out>.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from se2lam_amd import capi, synth  # noqa: E402
from se2lam_amd.orb import ORBextractor  # noqa: E402
from se2lam_amd.vocabulary import Vocabulary  # noqa: E402
import voc_train_cases as vc  # noqa: E402


def commit(arg):
    if arg:
        return arg
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def profile_table():
    rows, i = [], 0
    name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
    while capi.lib().se2gpu_voc_train_profile_get(i, C.byref(name), C.byref(ms), C.byref(n)) == 0:
        rows.append((name.value.decode(), ms.value, n.value))
        i += 1
    return sorted(rows, key=lambda r: -r[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="32 frames, L = 3: a functional check of the tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voc_train"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--runs", type=int, default=7, help="timed windows")
    ap.add_argument("--calls", type=int, default=25, help="back-to-back training calls per window")
    ap.add_argument("--host-runs", type=int, default=2)
    a = ap.parse_args()
    assert capi.device_count() > 0, "needs a GPU"
    nframes, k, L, cap, B = (32, 10, 3, 1024, 32) if a.quick else (256, 10, 5, 1024, 64)
    seed, wt, sc = 2024, 0, 0

    ex = ORBextractor(max_batch=B)
    d_desc, d_cnt, d_kps = capi.DeviceArray(nframes * cap * 32), capi.DeviceArray(nframes * 4), capi.DeviceArray(B * cap * 28)
    for f0 in range(0, nframes, B):
        d_img = capi.DeviceArray.from_numpy(synth.frames(B, start=f0))
        ex.extract_batch_device(d_img.ptr, B, 480, 640, d_kps.ptr, C.c_void_p(d_desc.ptr.value + f0 * cap * 32),
                                C.c_void_p(d_cnt.ptr.value + f0 * 4), cap)
        ex.sync()
    counts = d_cnt.to_numpy(np.int32, (nframes,))
    desc = d_desc.to_numpy(np.uint8, (nframes, cap, 32))
    total = int(counts.sum())
    print("input: %d frames, %d descriptors" % (nframes, total), flush=True)

    def train():
        return Vocabulary.train(d_desc.ptr, d_cnt.ptr, k, L, wt, sc, seed, cap=cap, nframes=nframes)

    voc = train()   # warm-up: code objects, allocator
    dev_s = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            voc = train()
        dev_s.append((time.perf_counter() - t0) / a.calls)
    print("device seconds per call, one figure per window of %d calls" % a.calls, dev_s, flush=True)

    tmp = tempfile.mkdtemp(prefix="voc_train_bench_")
    exe, r = vc.compile_mirror(tmp)
    assert r.returncode == 0, r.stderr
    docs = [desc[f, :counts[f]] for f in range(nframes)]
    vc.write_case(os.path.join(tmp, "case.bin"), docs, k, L, wt, sc, seed, 0)
    r = subprocess.run([exe, os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin"), "-", str(a.host_runs)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    host_s = [float(x) for x in [l for l in r.stdout.splitlines() if l.startswith("SECONDS")][0].split()[1:]]
    print("host seconds", host_s, flush=True)
    want = vc.parse_out(os.path.join(tmp, "out.bin"))
    parent, ndesc, weight, leaf = voc.export()
    equal = (voc.train_stats == want["stats"] and np.array_equal(parent, want["parent"]) and np.array_equal(ndesc[1:], want["desc"][1:]) and
             np.array_equal(weight, want["weight"]) and np.array_equal(leaf, want["leaf"]))
    assert equal, "the device vocabulary differs from the mirror's"

    capi.check(capi.lib().se2gpu_voc_train_profile(1))
    train()
    table = profile_table()
    capi.check(capi.lib().se2gpu_voc_train_profile(0))

    dev_med, host_med = statistics.median(dev_s), statistics.median(host_s)
    res = dict(commit=commit(a.commit), frames=nframes, descriptors=total, k=k, L=L, stats=voc.train_stats, device_seconds=dev_s, calls_per_window=a.calls, host_seconds=host_s,
               device_median_s=dev_med, host_median_s=host_med, speedup=host_med / dev_med, equal_to_mirror=bool(equal),
               kernels=[dict(name=n, total_ms=ms, launches=c) for n, ms, c in table])
    with open(a.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    with open(a.out + ".md", "w") as f:
        f.write("# Vocabulary training: device against the one-thread host mirror\n\n")
        f.write("Tree: %s.  `tools/voc_train_bench.py%s`: %d synthetic frames, %d descriptors, extracted on the device and handed over in device "
                "memory; k = %d, L = %d, TF-IDF.  The device vocabulary equals the mirror's bit for bit (checked in this run).\n\n"
                % (res["commit"], " --quick" if a.quick else "", nframes, total, k, L))
        f.write("| | median | min | max | runs |\n|---|---|---|---|---|\n")
        f.write("| `se2gpu_voc_train` (wall per synchronous call; windows of %d back-to-back calls) | %.4f s | %.4f s | %.4f s | %d windows |\n"
                % (a.calls, dev_med, min(dev_s), max(dev_s), len(dev_s)))
        f.write("| `ORBVocabulary::create` (g++ -O2, one thread) | %.3f s | %.3f s | %.3f s | %d |\n" % (host_med, min(host_s), max(host_s), len(host_s)))
        f.write("\nHost over device: %.1fx.\n\n" % (host_med / dev_med))
        f.write("Vocabulary: %s\n\n" % json.dumps(voc.train_stats))
        f.write("Kernels of one call with the profile hooks on (HIP events around every launch; this call is serialised and slower than the timed "
                "ones; the transform's own two kernels of the weights step are not in the table):\n\n| kernel | launches | total ms | mean us |\n|---|---|---|---|\n")
        for n, ms, c in table:
            f.write("| `%s` | %d | %.3f | %.1f |\n" % (n, c, ms, 1e3 * ms / max(c, 1)))
        f.write("| sum | %d | %.3f | |\n" % (sum(c for _, _, c in table), sum(ms for _, ms, _ in table)))
    print(json.dumps({key: res[key] for key in ("device_median_s", "host_median_s", "speedup", "equal_to_mirror")}))


if __name__ == "__main__":
    main()
