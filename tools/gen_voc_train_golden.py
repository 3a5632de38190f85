"""Regenerates tests/golden/voc_train_dbow2.npz: three small training sets, the vocabulary file that the reference's own DBoW2
makes of each, and the rand() values it consumed on the way (tools/gen_voc_train_golden.cpp).

    python tools/gen_voc_train_golden.py [--reference DIR]

Needs the reference's source tree (SE2LAM_REFERENCE, as oracle/ref.py); the program is compiled into a temporary directory with
the flags of REFMAP_FLAGS in oracle/Makefile.  The reference's create dereferences a null pointer when a cluster loses all its
members ("Vocabulary training", deviation 2): a case whose process dies stops this script - pick another seed for it.
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "voc_train_dbow2.npz")
# (data seed, documents, descriptors per document, prototypes, bit-flip rate, k, L, weighting, srand seed)
CASES = [(1, 12, 60, 40, 0.05, 4, 3, 0, 1001), (2, 20, 100, 200, 0.08, 10, 3, 0, 1002), (5, 6, 40, 400, 0.2, 6, 2, 1, 1005)]
SCORING = 0


def make_docs(seed, ndocs, per, nproto, flips):
    """random prototypes with random bit flips and a few exact duplicates"""
    r = np.random.default_rng(seed)
    protos = r.integers(0, 256, (nproto, 32), dtype=np.uint8)
    docs = []
    for _ in range(ndocs):
        bits = np.unpackbits(protos[r.integers(0, nproto, per)], axis=1)
        docs.append(np.packbits(bits ^ (r.random(bits.shape) < flips), axis=1))
    docs[0][1] = docs[0][0]
    docs[1][0] = docs[0][0]
    return docs


def main():
    ap = argparse.ArgumentParser()
    sys.path.insert(0, ROOT)
    from oracle import ref as oracle_ref
    ap.add_argument("--reference", default=oracle_ref.REFERENCE, help="the reference's source tree (default: where oracle/ref.py looks)")
    a = ap.parse_args()
    ref, shim = a.reference, os.path.join(ROOT, "oracle", "_shim")
    if not os.path.isdir(os.path.join(ref, "Thirdparty", "DBoW2")):
        sys.exit("the reference's tree is not at %s" % ref)
    db = os.path.join(ref, "Thirdparty", "DBoW2")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gen_voc_train_golden")
        cmd = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++14", "-w", "-I", shim, "-I", os.path.join(ref, "include", "se2lam"),
               "-I", ref, "-include", os.path.join(shim, "se2lam_stubs_map.h"), os.path.join(ROOT, "tools", "gen_voc_train_golden.cpp"),
               os.path.join(shim, "cv_shim.cpp")] + [os.path.join(db, p) for p in ("DBoW2/FeatureVector.cpp", "DBoW2/BowVector.cpp", "DBoW2/FORB.cpp",
                                                                                  "DBoW2/ScoringObject.cpp", "DUtils/Random.cpp", "DUtils/Timestamp.cpp")]
        subprocess.check_call(cmd + ["-o", exe, "-lm", "-lpthread"])
        out = {"ncases": np.int32(len(CASES))}
        for i, (dseed, ndocs, per, nproto, flips, k, L, wt, seed) in enumerate(CASES):
            docs = make_docs(dseed, ndocs, per, nproto, flips)
            counts = np.array([len(d) for d in docs], "<i4")
            case, voc, rnd = (os.path.join(tmp, n) for n in ("case.bin", "voc.bin", "rand.bin"))
            with open(case, "wb") as f:
                f.write(struct.pack("<6i", ndocs, k, L, wt, SCORING, seed) + counts.tobytes() + np.concatenate(docs).tobytes())
            r = subprocess.run([exe, case, voc, rnd], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("case %d: the reference's create ended with %d (a negative value is a signal: an emptied cluster, most likely) - "
                         "choose another seed for it\n%s" % (i + 1, r.returncode, r.stderr))
            print("case", i + 1, r.stdout.strip())
            out["desc%d" % i] = np.concatenate(docs)
            out["counts%d" % i] = counts
            out["params%d" % i] = np.array([k, L, wt, SCORING, seed], np.int64)
            out["rand%d" % i] = np.fromfile(rnd, "<i4")
            out["voc%d" % i] = np.fromfile(voc, np.uint8)
        np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
