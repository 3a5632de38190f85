"""The training cases that tests/test_voc_train.py (mirror against model) and tests/test_voc_train_gpu.py (device against mirror)
share, and the plumbing around tests/cpp_voc_train.cpp.  Every case names what it is for; `expect` is asserted on the model's
result before anything is compared."""
import os
import struct
import subprocess

import numpy as np

import voc_train_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "voc_train_dbow2.npz")
TF_IDF, TF, IDF, BINARY = range(4)


def golden_case(i):
    """-> (docs, k, L, weighting, scoring, srand seed, rand values, vocabulary file bytes) of case i (0-based) of the fixture"""
    g = np.load(GOLDEN)
    counts, desc = g["counts%d" % i], g["desc%d" % i]
    docs = np.split(desc, np.cumsum(counts)[:-1])
    k, L, wt, sc, seed = (int(x) for x in g["params%d" % i])
    return docs, k, L, wt, sc, seed, g["rand%d" % i], g["voc%d" % i].tobytes()


def parse_voc(blob):
    """the file saveToBinaryFile writes -> (k, L, scoring, weighting, parent, desc, weight float32, leaf), root included"""
    nb, sz, k, L, sc, wt = struct.unpack_from("<IIiiii", blob, 0)
    assert sz == 41 and len(blob) == 24 + 41 * (nb - 1)
    rec = np.frombuffer(blob, np.dtype([("parent", "<i4"), ("desc", "u1", 32), ("weight", "<f4"), ("leaf", "u1")]), nb - 1, 24)
    z = lambda a, dt: np.concatenate([np.zeros((1,) + a.shape[1:], dt), a.astype(dt)])
    return k, L, sc, wt, z(rec["parent"], np.int32), z(rec["desc"], np.uint8), z(rec["weight"], np.float32), z(rec["leaf"], bool)


def noisy_docs(seed, counts, nproto, flips):
    r = np.random.default_rng(seed)
    protos = r.integers(0, 256, (nproto, 32), dtype=np.uint8)
    docs = []
    for c in counts:
        bits = np.unpackbits(protos[r.integers(0, nproto, c)], axis=1)
        docs.append(np.packbits(bits ^ (r.random(bits.shape) < flips), axis=1).reshape(-1, 32))
    return docs


def _dups(seed):
    """more than k copies of fewer than k distinct descriptors (k = 4: 3 distinct, 6 copies each) among 200 others, spread over
    the documents; the three are far from everything else, so a node ends up holding only them and its seeding stops short"""
    docs = noisy_docs(seed, [40] * 5, 12, 0.03)
    r = np.random.default_rng(seed + 1)
    trio = r.integers(0, 256, (3, 32), dtype=np.uint8)
    for d in range(5):
        docs[d] = np.concatenate([docs[d], trio, trio[:1]] if d < 3 else [docs[d], trio])
    return docs


def _has_node(m, members, inner=None, below_L=None, L=None):
    ok = m["node_members"] == members
    ok[0] = members == m["node_members"][0]
    if inner is not None:
        ok &= (~m["leaf"]) == inner
    if below_L:
        ok &= m["node_level"] < L
    return bool(ok.any())


# name -> (docs, k, L, weighting, scoring, seed, max_iters, cap beyond the largest count, expect(model result))
def build_cases():
    g1, g2 = golden_case(0), golden_case(1)
    c = {}
    # the first two cases of the fixture with value semantics lose clusters (empty_clusters > 0); g2 is a root of 2,000 = 7 tiles + 208
    c["golden1-empty"] = (g1[0], 4, 3, TF_IDF, 0, 1001, 0, 0, lambda m: m["stats"]["empty_clusters"] > 0)
    c["golden2-root2000"] = (g2[0], 10, 3, TF_IDF, 0, 1002, 0, 0,
                             lambda m: m["stats"]["empty_clusters"] > 0 and m["ties"] > 0 and m["node_members"][0] == 2000 and
                             ((m["node_members"] > 10) & (m["node_members"] < 64)).any())   # k-means nodes smaller than a wave
    # 2,049 = 8 tiles + 1, documents without descriptors, a capacity beyond every count, k = 2 down to depth 6
    cnt = [0, 683, 0, 683, 683, 0]
    c["root2049-k2-L6-idf"] = (noisy_docs(11, cnt, 60, 0.06), 2, 6, IDF, 1, 7, 0, 17,
                               lambda m: m["node_members"][0] == 2049 and m["node_level"].max() == 6 and m["stats"]["kmeans_nodes"] > 20)
    c["k32-L1-tf"] = (noisy_docs(12, [300] * 5, 100, 0.1), 32, 1, TF, 4, 8, 0, 0, lambda m: m["stats"]["kmeans_nodes"] == 1 and m["stats"]["nodes"] > 30)
    c["dups-short-seeding-binary"] = (_dups(13), 4, 4, BINARY, 5, 9, 0, 3, lambda m: m["stats"]["short_seeded_nodes"] > 0)
    c["capped-max-iters-2"] = (g2[0], 10, 3, TF_IDF, 0, 1002, 2, 0, lambda m: m["stats"]["capped_nodes"] > 0 and m["stats"]["lloyd_iters_max"] == 2)
    # the sizes around k: a root with exactly k members (trivial: no draws), one with k + 1 (the smallest k-means node)
    c["root-n-equals-k"] = (noisy_docs(14, [2, 3], 5, 0.2), 5, 3, TF_IDF, 0, 10, 0, 5,
                            lambda m: m["stats"]["trivial_nodes"] == 1 and m["stats"]["kmeans_nodes"] == 0 and m["stats"]["words"] == 5)
    c["root-n-equals-k-plus-1"] = (noisy_docs(15, [3, 3], 3, 0.05), 5, 3, IDF, 0, 11, 0, 0,
                                   lambda m: m["stats"]["kmeans_nodes"] >= 1 and m["node_members"][0] == 6)
    # an inner node with exactly k members (trivial below the root), leaves with one member above depth L
    c["k3-L6-small-nodes"] = (noisy_docs(16, [50] * 8, 30, 0.03), 3, 6, TF_IDF, 2, 12, 0, 1,
                              lambda m: _has_node(m, 3, inner=True) and _has_node(m, 1, below_L=True, L=6) and m["stats"]["trivial_nodes"] > 0)
    # a root of 100,000 members = 391 tiles: the node sum and the search for the cut's tile go over more than one chunk of 256
    # tile sums, and a seed is taken beyond the first chunk
    c["root100000-k5-L1"] = (noisy_docs(17, [4000] * 25, 8, 0.1), 5, 1, TF, 0, 13, 0, 0,
                             lambda m: m["node_members"][0] == 100000 and m["far_picks"] > 0)
    return c


def model_of(case):
    docs, k, L, wt, sc, seed, max_iters, extra, _ = case
    return vm.train(docs, k, L, wt, vm.Counter(seed), alias=False, max_iters=max_iters or 1000)


def compile_mirror(dirpath, flags=("-O2",), name="cpp_voc_train"):
    exe = os.path.join(str(dirpath), name)
    r = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_voc_train.cpp"), "-o", exe],
                       capture_output=True, text=True)
    return exe, r


def compile_device_class(dirpath):
    exe = os.path.join(str(dirpath), "cpp_voc_train_device")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_voc_train_device.cpp"),
                           "-o", exe, "-L", libdir, "-lse2gpu", "-Wl,-rpath," + libdir])
    return exe


def write_case(path, docs, k, L, wt, sc, seed, max_iters):
    counts = np.array([len(d) for d in docs], "<i4")
    feats = np.concatenate([np.asarray(d, np.uint8).reshape(-1, 32) for d in docs]) if len(docs) else np.zeros((0, 32), np.uint8)
    with open(path, "wb") as f:
        f.write(struct.pack("<6iQ", len(docs), k, L, wt, sc, max_iters, seed) + counts.tobytes() + feats.tobytes())


def run_mirror(exe, tmp, docs, k, L, wt, sc, seed, max_iters=0, voc_out=None, env=None):
    """-> None when refused, else dict(parent, desc, weight float64, leaf, stats)"""
    tmp = str(tmp)
    write_case(os.path.join(tmp, "case.bin"), docs, k, L, wt, sc, seed, max_iters)
    r = subprocess.run([exe, os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin"), str(voc_out) if voc_out else "-"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return parse_out(os.path.join(tmp, "out.bin"))


def parse_out(path):
    """the driver's output file -> None when refused, else dict(parent, desc, weight float64, leaf, stats)"""
    buf = open(path, "rb").read()
    if struct.unpack_from("<i", buf, 0)[0] == 0:
        return None
    st = dict(zip(vm.STAT_NAMES, struct.unpack_from("<10i", buf, 4)))
    n = struct.unpack_from("<i", buf, 44)[0]
    at = 48
    parent = np.frombuffer(buf, "<i4", n, at); at += 4 * n
    desc = np.frombuffer(buf, np.uint8, 32 * n, at).reshape(n, 32); at += 32 * n
    weight = np.frombuffer(buf, "<f8", n, at); at += 8 * n
    leaf = np.frombuffer(buf, np.uint8, n, at).astype(bool); at += n
    assert at == len(buf)
    return dict(parent=parent, desc=desc, weight=weight, leaf=leaf, stats=st)


def pad_docs(docs, extra):
    """the documents in the layout of se2gpu_voc_train: desc (nframes, cap, 32) with cap = the largest count + extra, and counts;
    the slots beyond a count hold 0xff so that reading one shows"""
    counts = np.array([len(d) for d in docs], np.int32)
    cap = max(int(counts.max()) + extra, 1)
    desc = np.full((len(docs), cap, 32), 0xff, np.uint8)
    for i, d in enumerate(docs):
        desc[i, :len(d)] = d
    return desc, counts, cap
