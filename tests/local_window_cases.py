"""Inputs of the local-window tests: hand-worked maps whose answers are written down here, seeded random directed adjacencies
on the maps of tests/covis_cases.py, the fixture of the compiled reference (tests/golden/local_window_ref.npz, written by
tools/gen_local_window_golden.py) and the driver of tests/cpp_local_window.cpp."""
import os

import numpy as np

import covis_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "local_window_ref.npz")


def random_adjacency(seed, nframes, tail_bits=True):
    """mCovisibleKFs per slot: 0-2 slots within two places on a ring, now and then a far one or the slot itself; directed.
    tail_bits: a few entries in nframes .. 64 * WF - 1, which the contract calls zero and the calls must ignore."""
    rng = np.random.default_rng(seed)
    adj = []
    for a in range(nframes):
        near = [(a + int(d)) % nframes for d in rng.integers(-2, 3, int(rng.integers(0, 3)))]
        if rng.random() < 0.1:
            near.append(int(rng.integers(0, nframes)))
        adj.append(sorted(set(near)))
    room = 64 * ((nframes + 63) // 64) - nframes
    if tail_bits and room:
        for a in rng.integers(0, nframes, 3):
            adj[int(a)] = sorted(set(adj[int(a)]) | {nframes + int(rng.integers(0, room))})
    return adj


def permuted_order(seed, n, plant=True):
    """a permutation of 0..n-1; plant: two entries replaced by values out of range, which the lists skip"""
    rng = np.random.default_rng(seed)
    o = rng.permutation(n).astype(np.int32)
    if plant and n > 4:
        o[rng.integers(0, n)] = -1
        o[rng.integers(0, n)] = n
    return o


def job_list(nframes):
    """every slot as the current key frame (at most 40), one slot out of range, one slot twice"""
    jobs = list(range(nframes)) if nframes <= 40 else [int(x) for x in np.linspace(0, nframes - 1, 40).astype(int)]
    return np.array(jobs[:len(jobs) // 2] + [nframes] + jobs[len(jobs) // 2:] + [jobs[0], -1], np.int32)


# Hand cases: name -> dict(kf (tables of the key frame's side), mp (tables of the point's side or None), adj, frame_null, cur,
# level, local, ref, mps, n_obs).  The answers are worked out by hand from Map.cpp:298-326.
def hand_cases():
    c = {}

    def case(name, kf_points, m, adj, cur, local, ref, mps, n_obs, level=3, null=(), frame_null=None, mp_points=None):
        c[name] = dict(kf=cc.from_kf_lists(kf_points, m, null=null), mp=None if mp_points is None else cc.from_kf_lists(mp_points, m, null=null),
                       adj=adj, frame_null=frame_null, cur=cur, level=level, local=local, ref=ref, mps=mps, n_obs=n_obs)

    six = [[0], [1], [2], [3], [4], [5, 0]]
    # three hops down a chain reach four key frames, whichever way the slots run: a sweep that expands in place, in ascending
    # slot order, would reach all six in the first round of the ascending chain
    case("chain_ascending", six, 6, [[1], [2], [3], [4], [5], []], 0, [0, 1, 2, 3], [5], [0, 1, 2, 3], 5)
    case("chain_descending", six, 6, [[], [0], [1], [2], [3], [4]], 5, [2, 3, 4, 5], [0], [0, 2, 3, 4, 5], 6)
    # 0 lists 1, 1 does not list 0
    case("one_way_followed", [[0], [0, 1]], 2, [[1], []], 0, [0, 1], [], [0, 1], 3)
    case("one_way_not_followed", [[0], [0, 1]], 2, [[1], []], 1, [1], [0], [0, 1], 3)
    case("self_loop", [[0], [1]], 2, [[0], []], 0, [0], [], [0], 1)
    case("isolated", [[0, 1], [1], [2]], 3, [[], [0], []], 0, [0], [1], [0, 1], 3)
    # word edges of the key-frame rows: neighbours in the word below and two words up
    pts = [[] for _ in range(130)]
    pts[63], pts[64], pts[128], pts[129] = [0], [1], [2], [2]
    adj = [[] for _ in range(130)]
    adj[64] = [63, 128]
    case("slot_64", pts, 3, adj, 64, [63, 64, 128], [129], [0, 1, 2], 4)
    # point 1 is null: it leaves the point set, and key frame 1, which sees nothing else, is no reference key frame
    case("null_point", [[0, 1], [1], [0]], 2, [[], [], []], 0, [0], [2], [0], 2, null=[1])
    # key frame 1 is null and reachable: local, and its point counts; key frame 2 is null and only an observer: not a reference
    # key frame; neither adds an edge
    case("null_key_frame", [[0], [1], [0], [1]], 2, [[1], [], [], []], 0, [0, 1], [3], [0, 1], 2, frame_null=[0, 1, 1, 0])
    # point 0 lists key frame 1, key frame 1 does not list point 0: getObservations() decides (:320)
    case("sides_differ", [[0], [], [1]], 2, [[], [], []], 0, [0], [1], [0], 2, mp_points=[[0], [0], [1]])
    return c


def golden_maps(path=GOLDEN):
    """One dict per map: kf_id, mp_id, kf_obs (points per slot), adj (slots per slot), jobs = [(local, ref, mps)] per current
    slot, as the compiled reference listed them (slot / point indices in the reference's order)."""
    z = {k: v.astype(np.int64) for k, v in np.load(path).items()}
    cut = lambda name, i: [int(x) for x in z[name][z[name + "_off"][i]:z[name + "_off"][i + 1]]]  # noqa: E731
    maps = []
    for i in range(len(z["kf_off"]) - 1):
        k0, k1 = int(z["kf_off"][i]), int(z["kf_off"][i + 1])
        maps.append(dict(kf_id=[int(x) for x in z["kf_id"][k0:k1]],
                         mp_id=[int(x) for x in z["mp_id"][z["mp_off"][i]:z["mp_off"][i + 1]]],
                         kf_obs=[cut("obs", k) for k in range(k0, k1)], adj=[cut("adj", k) for k in range(k0, k1)],
                         jobs=[(cut("loc", k), cut("ref", k), cut("mps", k)) for k in range(k0, k1)]))
    return maps


def golden_coverage(maps):
    """(share of jobs that select fewer key frames than the map holds, share with a reference key frame, maps with a one-way
    edge, maps whose slots are in id order)"""
    jobs = [(len(g["kf_id"]), j) for g in maps for j in g["jobs"]]
    one_way = sum(any(a not in g["adj"][b] for a in range(len(g["adj"])) for b in g["adj"][a]) for g in maps)
    in_order = sum(all(x < y for x, y in zip(g["kf_id"], g["kf_id"][1:])) for g in maps)
    return (sum(len(j[0]) < n for n, j in jobs) / len(jobs), sum(len(j[1]) > 0 for _, j in jobs) / len(jobs), one_way, in_order)


def golden_tables(g):
    return cc.from_kf_lists(g["kf_obs"], len(g["mp_id"]), cap=128)


def id_order(ids):
    """the slots / points by ascending id: d_kf_order / d_mp_order"""
    return np.argsort(np.asarray(ids), kind="stable").astype(np.int32)


# ---- the header's host functions (include/se2lam_amd/LocalWindow.h) through tests/cpp_local_window.cpp

def cpp_build(outdir):
    import subprocess
    out = os.path.join(str(outdir), "cpp_local_window")
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_local_window.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    return out


def cpp_map_lines(kf_id, mp_id, kf_obs, mp_obs, adj, kf_null=None, mp_null=None):
    nkf, m = len(kf_id), len(mp_id)
    j = lambda v: " ".join(str(int(x)) for x in v)  # noqa: E731
    lines = ["M %d %d %s %s %s %s" % (nkf, m, j(kf_id), j(mp_id), j(kf_null if kf_null is not None else [0] * nkf),
                                      j(mp_null if mp_null is not None else [0] * m))]
    for tag, sets in (("A", adj), ("K", kf_obs), ("O", mp_obs)):
        lines += ["%s %d %d %s" % (tag, i, len(s), j(sorted(s))) for i, s in enumerate(sets)]
    return lines


def cpp_run(program, path, lines):
    """-> the output lines as lists: ("G", slot, [slots]) and ("U", n_obs, local, ref, mps)"""
    import subprocess
    with open(str(path), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = []
    for ln in r.stdout.splitlines():
        v = [int(x) for x in ln.split()[1:]]
        if ln[0] == "G":
            assert v[1] == len(v) - 2
            out.append(("G", v[0], v[2:]))
        else:
            lists, at = [], 1
            for _ in range(3):
                lists.append(v[at + 1:at + 1 + v[at]])
                at += 1 + v[at]
            assert at == len(v)
            out.append(("U", v[0], *lists))
    return out
