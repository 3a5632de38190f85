"""Inputs of the covisibility tests: hand-worked maps whose answers are written down here, and seeded random maps with the
irregularities the calls must survive (entries out of range, descending and overlapping d_mp_ptr segments)."""
import numpy as np

CAP = 16


def from_kf_lists(kf_points, m, null=(), bad_prl=(), cap=64, twice=()):
    """A map given as the points each key frame observes (kf_points[f], the key frame's side).  Returns the tables as a dict.
    twice: (frame, point) pairs whose entry is listed a second time with another feature."""
    nframes = len(kf_points)
    lists = [[] for _ in range(m)]
    nxt = [0] * nframes
    for f, pts in enumerate(kf_points):
        for p in pts:
            lists[p].append((f, nxt[f]))
            nxt[f] += 1
    for f, p in twice:
        lists[p].append((f, nxt[f]))
        nxt[f] += 1
    assert max(nxt + [0]) <= cap
    ptr = np.zeros(m + 1, np.int32)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    flat = [e for l in lists for e in l]
    mp_null, good = np.zeros(m, np.uint8), np.ones(m, np.uint8)
    mp_null[list(null)] = 1
    good[list(bad_prl)] = 0
    return dict(counts=np.full(nframes, cap, np.int32), cap=cap, mp_ptr=ptr,
                obs_frame=np.array([e[0] for e in flat], np.int32), obs_ftr=np.array([e[1] for e in flat], np.int32),
                mp_null=mp_null, good_prl=good)


def tables(t):
    return (t["counts"], t["cap"], t["mp_ptr"], t["obs_frame"], t["obs_ftr"], t["mp_null"], t["good_prl"])


# Hand cases: name -> (tables, call, expected).  call = ("pairs", a, b) or ("refset", kf, refs, k)
def hand_cases():
    c = {}
    r = lambda a, b: list(range(a, b))  # noqa: E731
    # Map.cpp:794 with 0.3f: 0.3f = 0.300000011920928955078125, times 10 = 3.00000011920928955078125, exactly halfway between
    # the floats 3 and 3 + 2^-22: ties-to-even gives 3.0f, and 3.0f > 3.0f is false
    c["size10_n3_float"] = (from_kf_lists([r(0, 10), r(0, 3)], 10), ("pairs", 0, 1),
                            dict(out=(3, 10, 3, 0b10), ratio=(np.float32(3) / np.float32(10), np.float32(1))))   # 3 > 0.1 * 10 in double
    c["size10_n4_float"] = (from_kf_lists([r(0, 10), r(0, 4)], 10), ("pairs", 0, 1),
                            dict(out=(4, 10, 4, 0b11), ratio=(np.float32(4) / np.float32(10), np.float32(1))))
    # Localizer.cpp:683 with 0.1 in double: the product 0.1 * 30 = 3 + 1.7e-16 is at least 3 (it rounds to 3.0), so 3 > it is
    # false where 3 > 0.0999 * 30 would be true; in float 3 > 9.0f is false
    c["size30_n3_double"] = (from_kf_lists([r(0, 30), r(0, 3)], 30), ("pairs", 0, 1),
                             dict(out=(3, 30, 3, 0), ratio=(np.float32(3) / np.float32(30), np.float32(1))))
    # a null point that still has entries: in both sizes, not in n_same
    c["null_point"] = (from_kf_lists([[0, 1, 2], [1, 2, 3]], 4, null=[1]), ("pairs", 0, 1),
                       dict(out=(1, 3, 3, 0b11), ratio=(np.float32(1) / np.float32(3), np.float32(1) / np.float32(3)), common=[2]))
    # a point that is not good parallax counts in the pair call ...
    bad = from_kf_lists([[0, 1, 2], [0, 1, 2], [0, 1, 2]], 3, bad_prl=[0])
    c["bad_parallax_pairs"] = (bad, ("pairs", 0, 1), dict(out=(3, 3, 3, 0b11), ratio=(np.float32(1), np.float32(1)), common=[0, 1, 2]))
    # ... and not in the reference-set call: all = 2, both seen twice
    c["bad_parallax_refset"] = (bad, ("refset", 0, [1, 2], 2), dict(out=(2, 2, 1), ratio=1.0, ret=[1, 2]))
    # Map.cpp:196: cnt 4 of all 5, 4.0 / 5.0 is the double 0.8 and 0.8 >= 0.8
    five = from_kf_lists([r(0, 5), r(0, 4), r(0, 4)], 5)
    c["cnt4_all5"] = (five, ("refset", 0, [1, 2], 2), dict(out=(4, 5, 1), ratio=4.0 / 5.0, ret=[0, 1, 2, 3]))
    c["cnt3_all5"] = (from_kf_lists([r(0, 5), r(0, 4), r(0, 3)], 5), ("refset", 0, [1, 2], 2), dict(out=(3, 5, 0), ratio=3.0 / 5.0, ret=[0, 1, 2]))
    # all == 0: a key frame with null points only (:377-379)
    c["all_zero"] = (from_kf_lists([[0, 1], [0, 1]], 2, null=[0, 1]), ("refset", 0, [1], 1), dict(out=(0, 0, 0), ratio=-1.0, ret=[]))
    # a frame listed twice by one point counts once, and e_a is its first entry
    tw = from_kf_lists([[0, 1], [0, 1]], 2, twice=[(0, 0)])
    c["frame_twice"] = (tw, ("pairs", 0, 1), dict(out=(2, 2, 2, 0b11), ratio=(np.float32(1), np.float32(1)), common=[0, 1]))
    # a reference slot listed twice counts twice: frame 1 alone reaches k = 2
    c["ref_twice"] = (five, ("refset", 0, [1, 1], 2), dict(out=(4, 5, 1), ratio=4.0 / 5.0, ret=[0, 1, 2, 3]))
    c["ref_once"] = (five, ("refset", 0, [1], 2), dict(out=(0, 5, 0), ratio=0.0, ret=[]))
    return c


def random_map(seed, nframes, m, cap=CAP, irregular=True):
    """Lists of 0-6 entries.  irregular: planted invalid entries (frame -1, nframes, feature >= counts, feature < 0) and a few
    d_mp_ptr values replaced (descending, overlapping, negative, past nobs)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(cap // 2, cap + 5, nframes).astype(np.int32)      # some beyond cap: min(counts, cap) rules
    n = rng.integers(0, 7, m)
    ptr = np.zeros(m + 1, np.int32)
    ptr[1:] = np.cumsum(n)
    nobs = int(ptr[-1])
    # a window of key frames per point, as a map has; frames may repeat inside a list
    centre = rng.integers(0, nframes, m)
    owner = np.repeat(np.arange(m), n)
    obs_frame = ((centre[owner] + rng.integers(-3, 4, nobs)) % nframes).astype(np.int32)
    obs_ftr = rng.integers(0, cap // 2, nobs).astype(np.int32)
    if irregular and nobs:
        k = max(nobs // 12, 1)
        for val in (-1, nframes, nframes + 7):
            obs_frame[rng.integers(0, nobs, k)] = val
        at = rng.integers(0, nobs, k)
        obs_ftr[at] = np.minimum(counts[np.clip(obs_frame[at], 0, nframes - 1)], cap) + rng.integers(0, 2, k)
        obs_ftr[rng.integers(0, nobs, k)] = -1
        if m > 4:
            at = rng.integers(1, m, max(m // 16, 1))
            ptr[at] = rng.integers(-3, nobs + 4, len(at))
    return dict(counts=counts, cap=cap, mp_ptr=ptr, obs_frame=obs_frame, obs_ftr=obs_ftr,
                mp_null=(rng.random(m) < 0.1).astype(np.uint8), good_prl=(rng.random(m) < 0.7).astype(np.uint8))


def pair_list(seed, nframes, npairs=None):
    """all ordered pairs ((a, a) included) at small nframes, a seeded sample otherwise; out-of-range slots at the end"""
    if npairs is None:
        pa, pb = [list(x.ravel()) for x in np.meshgrid(np.arange(nframes), np.arange(nframes), indexing="ij")]
    else:
        rng = np.random.default_rng(seed)
        pa, pb = list(rng.integers(0, nframes, npairs)), list(rng.integers(0, nframes, npairs))
        pa[0], pb[0] = nframes - 1, nframes - 1
    return (np.array(pa + [-1, 0, nframes, 1 << 30], np.int32), np.array(pb + [0, nframes, 0, 0], np.int32))


def job_list(seed, nframes, njobs, max_refs):
    """reference lists of 0..max_refs slots, some out of range and some repeated; the last two jobs out of range"""
    rng = np.random.default_rng(seed)
    kf = rng.integers(0, nframes, njobs).astype(np.int32)
    n = rng.integers(0, max_refs + 1, njobs)
    n[0], n[-3] = 0, max_refs
    ptr = np.zeros(njobs + 1, np.int32)
    ptr[1:] = np.cumsum(n)
    idx = rng.integers(-1, nframes + 1, int(ptr[-1])).astype(np.int32)
    kf[-2:] = (-1, nframes)
    return kf, ptr, idx


# ---- the header's host functions (include/se2lam_amd/Covisibility.h) through tests/cpp_covis.cpp

def cpp_build(outdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(str(outdir), "cpp_covis")
    libdir = os.path.join(root, "se2lam_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_covis.cpp"), "-o", out, "-L", libdir, "-lse2gpu",
                           "-Wl,-rpath," + libdir])
    return out


def cpp_run(program, path, jobs):
    """jobs: [(tables, [call, ...])] with call = ("pairs", a, b) or ("refset", kf, refs, k).  Returns one dict per call:
    pairs -> n_same, size_a, size_b, ratio (2 float32), connect, common; refset -> cnt, ratio (float64), redundant, common."""
    import subprocess
    lines = []
    for t, calls in jobs:
        nobs = len(t["obs_frame"])
        lines.append("T " + " ".join(map(str, [len(t["counts"]), t["cap"], len(t["mp_ptr"]) - 1, nobs] + list(t["counts"]) +
                                         list(t["mp_ptr"]) + list(t["obs_frame"]) + list(t["obs_ftr"]) + list(t["mp_null"]) +
                                         list(t["good_prl"]))))
        for c in calls:
            lines.append("P %d %d" % (c[1], c[2]) if c[0] == "pairs" else
                         "R %d %d %d %s" % (c[1], c[3], len(c[2]), " ".join(map(str, c[2]))))
    with open(str(path), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = []
    for ln in r.stdout.splitlines():
        v = [int(x) for x in ln.split()[1:]]
        if ln[0] == "P":
            assert v[6] == len(v) - 7
            out.append(dict(n_same=v[0], size_a=v[1], size_b=v[2], ratio=np.array(v[3:5], np.uint32).view(np.float32), connect=v[5],
                            common=v[7:]))
        else:
            assert v[3] == len(v) - 4
            out.append(dict(cnt=v[0], ratio=float(np.array([v[1]], np.uint64).view(np.float64)[0]), redundant=v[2], common=v[4:]))
    assert len(out) == sum(len(c) for _, c in jobs)
    return out


def against_header(program, path, jobs):
    """cpp_run held to the set model (tests/covis_model.py), exactly; returns the number of calls compared"""
    import covis_model as cm
    got = cpp_run(program, path, jobs)
    i = 0
    for t, calls in jobs:
        m = cm.Model(*tables(t))
        for c in calls:
            g = got[i]
            i += 1
            if c[0] == "pairs":
                w = m.pairs([c[1]], [c[2]], 0.3, 0.1)
                assert (g["n_same"], g["size_a"], g["size_b"], g["connect"]) == (*w["out"][0, :3], w["out"][0, 3] & 1), c
                assert cm.same_floats(g["ratio"], w["ratio"][0]) and g["common"] == m.common(c[1], c[2]), c
            else:
                w = m.refset([c[1]], [0, len(c[2])], c[2], c[3], 0.8)
                assert g["cnt"] == w["out"][0, 0] and cm.same_floats(g["ratio"], w["ratio"][0]), c
                assert g["common"] == m.refset_points(c[1], c[2], c[3])[0], c
                assert g["redundant"] == m.refset([c[1]], [0, len(c[2])], c[2], 2, 0.8)["out"][0, 2], c
    return i


# ---- tests/golden/covis_ref.npz: maps built with the reference's own objects and what the compiled reference answered
# (tools/gen_covis_golden.cpp)

def golden_maps(path):
    """One dict per map: tables (as from_kf_lists returns them), nkf, pairs = [(a, b, ratio (2 float32), common)],
    jobs = [(kf, refs, ratio, common)] at k = 2, new_kf, local_kfs, connect."""
    z = {k: v for k, v in np.load(path).items()}
    i4 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    cut = lambda name, off, i: z[name][z[off][i]:z[off][i + 1]]  # noqa: E731
    maps = []
    for i in range(len(z["kf_off"]) - 1):
        counts = i4(cut("counts", "kf_off", i))
        nkf = len(counts)
        t = dict(counts=counts, cap=int(z["cap"][0]), mp_ptr=i4(cut("mp_ptr", "ptr_off", i)),
                 obs_frame=i4(cut("obs_frame", "obs_off", i)), obs_ftr=i4(cut("obs_ftr", "obs_off", i)),
                 mp_null=cut("mp_null", "mp_off", i).copy(), good_prl=cut("good_prl", "mp_off", i).copy())
        p0, k0 = int(z["pair_off"][i]), int(z["kf_off"][i])
        assert z["pair_off"][i + 1] - p0 == nkf * nkf
        pairs = [(a, b, z["pair_ratio"][p0 + a * nkf + b], [int(x) for x in cut("pair_common", "pair_common_off", p0 + a * nkf + b)])
                 for a in range(nkf) for b in range(nkf)]
        jobs = [(f, [int(x) for x in cut("ref_idx", "ref_off", k0 + f)], float(z["job_ratio"][k0 + f]),
                 [int(x) for x in cut("job_common", "job_common_off", k0 + f)]) for f in range(nkf)]
        maps.append(dict(tables=t, nkf=nkf, pairs=pairs, jobs=jobs, new_kf=int(z["new_kf"][i]),
                         local_kfs=[int(x) for x in cut("local_kfs", "local_off", i)],
                         connect=[int(x) for x in cut("connect", "connect_off", i)]))
    return maps
