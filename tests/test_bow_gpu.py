"""The device DBoW2 vocabulary (csrc/bow.hip through the C ABI: se2gpu_voc_*, se2gpu_bow_*, se2gpu_bowdb_*) against the host
vocabulary include/se2lam_amd/ORBVocabulary.h (compiled -O2 and driven by tests/cpp_bow_mirror.cpp, raw doubles both ways),
the numpy walk of tests/test_vocabulary.py and the reference's vendored DBoW2 (oracle/ref.py, RefVocabulary).

The rule: every output of the device equals the host vocabulary's bit for bit - ids with ==, values with np.array_equal.

Against the numpy walk, ids, counts and feature vectors are compared with ==.  Its values cannot be compared to the bit as
test_vocabulary._numpy_transform returns them, because it normalises with numpy's pairwise .sum(); the values are therefore
recomputed here from its words and counts with a sequential Python sum (the definition's order) and THOSE are compared with
np.array_equal, while _numpy_transform's own values are held to rtol 1e-14 as in tests/test_vocabulary.py.

Every case asserts, before anything is compared, that its inputs exercise what is easy to miss: a word with count >= 3, a
descriptor on a stopped word, a walk that meets a tie at the minimal distance between siblings (two siblings share one
descriptor; the earlier one must win), a walk that ends on a leaf above depth L (the "early" variants; these are compared with the
host vocabulary and numpy only, the reference leaves the node id uninitialised there), a node with fewer than k children (all
but the full tree)."""
import os
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vocabulary as tv  # noqa: E402

from oracle import ref  # noqa: E402

pytestmark = pytest.mark.gpu

NFRAMES, CAP = 64, 256
# (k, L, scoring, weighting, levelsup, seed): the seven tuples of test_vocabulary_mirror_equals_the_compiled_dbow2 ...
TUPLES = [(10, 4, 0, 0, 2, 0), (6, 6, 0, 0, 4, 1), (4, 3, 1, 1, 4, 2), (5, 4, 5, 0, 1, 3), (3, 5, 2, 2, 0, 4), (8, 3, 3, 3, 1, 5), (7, 4, 4, 0, 3, 6)]
# ... each without and with leaves above depth L, plus a full k = 10, L = 5 tree
CASES = [t + (False, False) for t in TUPLES] + [t + (True, False) for t in TUPLES] + [(10, 5, 0, 0, 4, 7, False, True)]
IDS = ["k%d-L%d-s%d-w%d-up%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "-early" if c[6] else "", "-full" if c[7] else "") for c in CASES]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("bow")
    exe = str(d / "cpp_bow_mirror")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp_bow_mirror.cpp"),
                        "-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, exe


def mirror_transform(exe, voc_path, desc, counts, levelsup, tmp):
    nframes, cap = desc.shape[:2]
    (tmp / "in.bin").write_bytes(struct.pack("<ii", nframes, cap) + np.asarray(counts, "<i4").tobytes() + np.ascontiguousarray(desc, np.uint8).tobytes())
    r = subprocess.run([exe, "transform", str(voc_path), str(tmp / "in.bin"), str(levelsup), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = (tmp / "out.bin").read_bytes()
    at, out = 0, []
    for _ in range(nframes):
        nb = struct.unpack_from("<i", buf, at)[0]; at += 4
        w = np.frombuffer(buf, "<u4", nb, at); at += 4 * nb
        v = np.frombuffer(buf, "<f8", nb, at); at += 8 * nb
        nn = struct.unpack_from("<i", buf, at)[0]; at += 4
        nodes = np.frombuffer(buf, "<i4", nn, at); at += 4 * nn
        ptr = np.frombuffer(buf, "<i4", nn + 1, at); at += 4 * (nn + 1)
        idx = np.frombuffer(buf, "<i4", int(ptr[nn]), at); at += 4 * int(ptr[nn])
        out.append((w, v, (nodes, ptr, idx)))
    assert at == len(buf)
    return out


def mirror_scores(exe, voc_path, queries, entries, tmp):
    blob = struct.pack("<ii", len(queries), len(entries))
    for w, v in list(queries) + list(entries):
        blob += struct.pack("<i", len(w)) + np.asarray(w, "<u4").tobytes() + np.asarray(v, "<f8").tobytes()
    (tmp / "vecs.bin").write_bytes(blob)
    r = subprocess.run([exe, "score", str(voc_path), str(tmp / "vecs.bin"), str(tmp / "scores.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.frombuffer((tmp / "scores.bin").read_bytes(), "<f8").reshape(len(queries), len(entries)).copy()


def walk_stats(parent, desc, weight, leaf, L, feats):
    """an independent walk that only counts: (walks that met a tie at the minimal distance, features on stopped words, walks that
    ended on a leaf above depth L, the word-defining leaf of every feature)"""
    n = len(parent)
    order = np.argsort(parent[1:], kind="stable") + 1
    start = np.searchsorted(parent[order], np.arange(n + 1))
    ties = stopped = early = 0
    leaves = []
    for f in feats:
        node, level = 0, 0
        while True:
            level += 1
            ch = order[start[node]:start[node + 1]]
            d = tv.POP[desc[ch] ^ f].sum(1)
            ties += int((d == d.min()).sum() > 1)
            node = ch[int(np.argmin(d))]
            if leaf[node]:
                break
        stopped += int(not weight[node] > 0)
        early += int(level < L)
        leaves.append(node)
    return ties, stopped, early, np.array(leaves, int)


def make_frames(rng, parent, desc, weight, leaf):
    """64 frames of 0 .. CAP descriptors near the words, with repeats; frame 0 is empty, frame 1 full.  A share of the features
    are the descriptors of leaves below a tied pair of siblings, unchanged, so that the tie is met at the minimal distance, and
    a few are the descriptors of stopped words and of leaves above depth L."""
    n = len(parent)
    first = np.nonzero(np.diff(parent[1:], prepend=-1))[0] + 1
    first = first[first + 1 < n]
    tied = first[(parent[first + 1] == parent[first]) & (desc[first] == desc[first + 1]).all(1)]
    below, depth = np.zeros(n, bool), np.zeros(n, int)
    below[tied] = True
    for i in range(1, n):
        below[i] |= below[parent[i]]
        depth[i] = depth[parent[i]] + 1
    early_leaves = np.nonzero(leaf & (depth < depth.max()))[0]
    tied_leaves, leaves = np.nonzero(leaf & below)[0], np.nonzero(leaf)[0]
    stopped_leaves = np.nonzero(leaf & ~(weight > 0))[0]
    assert len(tied_leaves) > 0 and len(stopped_leaves) > 0
    counts = rng.integers(0, CAP + 1, NFRAMES).astype(np.int32)
    counts[0], counts[1] = 0, CAP
    frames = np.zeros((NFRAMES, CAP, 32), np.uint8)
    for f in range(NFRAMES):
        c = int(counts[f])
        if c == 0:
            continue
        pool = rng.choice(leaves, max(c // 4, 1))                         # few words per frame: counts of 3 and more
        base = desc[rng.choice(pool, c)]
        noise = np.packbits(rng.random((c, 256)) < 0.03, axis=1)
        exact = rng.random(c) < 0.15
        base[exact] = desc[rng.choice(tied_leaves, int(exact.sum()))]
        noise[exact] = 0
        stop = rng.random(c) < 0.03
        base[stop] = desc[rng.choice(stopped_leaves, int(stop.sum()))]
        if len(early_leaves):
            up = rng.random(c) < 0.05
            base[up] = desc[rng.choice(early_leaves, int(up.sum()))]
        frames[f, :c] = base ^ noise
    return frames, counts


_cache = {}


def case_data(case, work):
    """vocabulary, frames, the host vocabulary's answer and the device's (batch form), built once per case"""
    if case in _cache:
        return _cache[case]
    from se2lam_amd import vocabulary as V
    tmp, exe = work
    k, L, scoring, weighting, levelsup, seed, early, full = case
    parent, desc, weight, leaf = V.synthetic_vocabulary(seed, k, L, weighting, full=full, early_leaf=0.25 if early else 0.0, tie_frac=0.3, stop_frac=0.1)
    path = tmp / ("voc_%d.bin" % CASES.index(case))
    V.write_vocabulary_file(path, k, L, scoring, weighting, parent, desc, weight, leaf)
    rng = np.random.default_rng(100 + seed)
    frames, counts = make_frames(rng, parent, desc, weight, leaf)
    voc = V.Vocabulary.load(path)
    ctx = V.BowContext(voc, max_features=CAP, max_batch=NFRAMES)
    d = dict(parent=parent, desc=desc, weight=weight, leaf=leaf, path=path, frames=frames, counts=counts, voc=voc, ctx=ctx,
             host=mirror_transform(exe, path, frames, counts, levelsup, tmp), dev=ctx.transform_batch(frames, counts, levelsup))
    _cache[case] = d
    return d


def same_vectors(a, b):
    return (np.array_equal(a[0], b[0]) and a[0].dtype == b[0].dtype and np.array_equal(a[1], b[1]) and
            all(np.array_equal(x, y) for x, y in zip(a[2], b[2])))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_transform_equals_the_host_vocabulary_and_the_numpy_walk(case, work):
    k, L, scoring, weighting, levelsup, seed, early, full = case
    d = case_data(case, work)
    parent, desc, weight, leaf, frames, counts = d["parent"], d["desc"], d["weight"], d["leaf"], d["frames"], d["counts"]
    assert d["voc"].words == int(leaf.sum()) and d["voc"].nodes == len(parent) and (d["voc"].k, d["voc"].L) == (k, L)
    assert (d["voc"].scoring, d["voc"].weighting) == (scoring, weighting)
    # ---- what the inputs exercise
    ties = stopped = early_walks = 0
    max_count = 0
    word_of = -np.ones(len(parent), int); word_of[np.nonzero(leaf)[0]] = np.arange(int(leaf.sum()))
    want_counts = []
    for f in range(NFRAMES):
        t, s, e, leaves = walk_stats(parent, desc, weight, leaf, L, frames[f, :counts[f]])
        ties += t; stopped += s; early_walks += e
        live = word_of[leaves[weight[leaves] > 0]] if len(leaves) else np.zeros(0, int)
        w, c = np.unique(live, return_counts=True)
        want_counts.append((w, c))
        max_count = max(max_count, int(c.max()) if len(c) else 0)
    nch = np.bincount(parent[1:], minlength=len(parent))
    print("inputs: %d tie walks, %d stopped features, %d early-leaf walks, largest count %d, children %d..%d" %
          (ties, stopped, early_walks, max_count, nch[~leaf].min(), nch[~leaf].max()))
    assert counts[0] == 0 and counts[1] == CAP and max_count >= 3 and stopped >= 1 and ties >= 1
    assert (early_walks >= 1) == early
    assert (nch[~leaf].min() < k) == (not full) and nch[~leaf].max() <= k
    # ---- device (batch) == host vocabulary, bit for bit; single-frame form == batch form
    for f in range(NFRAMES):
        assert same_vectors(d["dev"][f], d["host"][f]), f
    for f in list(range(8)) + [int(np.argmax(counts[2:])) + 2]:
        w, v, fv = d["ctx"].transform(frames[f, :counts[f]], levelsup)
        assert same_vectors((w, v, fv), d["dev"][f]), f
    assert len(d["dev"][0][0]) == 0 and len(d["dev"][0][2][0]) == 0 and list(d["dev"][0][2][1]) == [0]      # the empty frame
    # ---- == the numpy walk
    once = weighting in (2, 3)
    for f in range(NFRAMES):
        words, vals, fv = tv._numpy_transform(parent, desc, weight, leaf, L, scoring, weighting, frames[f, :counts[f]], levelsup)
        gw, gv, (gn, gp, gi) = d["dev"][f]
        assert gw.tolist() == words == want_counts[f][0].tolist()
        assert gn.tolist() == sorted(fv) and {int(gn[j]): gi[gp[j]:gp[j + 1]].tolist() for j in range(len(gn))} == fv
        if levelsup >= L and len(words):
            assert gn.tolist() == [0]
        assert np.allclose(gv, vals, rtol=1e-14, atol=0)
        # the definition's values, summed in the definition's order
        wl = weight[np.nonzero(leaf)[0]].astype(np.float64)
        raw = []
        for w_, c_ in zip(*want_counts[f]):
            acc = 0.0
            for _ in range(1 if once else int(c_)):
                acc += float(wl[w_])
            raw.append(acc)
        if scoring == 5:
            div = float(len(raw)) if (not once and raw) else 0.0
        else:
            div = 0.0
            for x in raw:
                div += x * x if scoring == 1 else abs(x)
            div = float(np.sqrt(np.float64(div))) if scoring == 1 else div
        seq = np.array([x / div for x in raw] if div > 0 else raw, np.float64)
        assert np.array_equal(gv, seq), f


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built and the reference's sources are not here")
@pytest.mark.parametrize("case", [c for c in CASES if not c[6]], ids=[i for i, c in zip(IDS, CASES) if not c[6]])
def test_transform_equals_the_compiled_dbow2(case, work):
    levelsup = case[4]
    d = case_data(case, work)
    v = ref.RefVocabulary(d["path"])
    assert v.loaded
    for f in range(NFRAMES):
        words, vals, fv = v.transform(d["frames"][f, :d["counts"][f]], levelsup)
        gw, gv, (gn, gp, gi) = d["dev"][f]
        assert gw.tolist() == words
        assert np.allclose(gv, vals, rtol=1e-15, atol=0)
        assert {int(gn[j]): gi[gp[j]:gp[j + 1]].tolist() for j in range(len(gn))} == fv


def test_batch_is_deterministic(work):
    case = CASES[1]
    d = case_data(case, work)
    for _ in range(3):
        again = d["ctx"].transform_batch(d["frames"], d["counts"], case[4])
        assert all(same_vectors(a, b) for a, b in zip(again, d["dev"]))


def test_two_threads_share_one_vocabulary(work):
    from se2lam_amd import vocabulary as V
    case = CASES[0]
    d = case_data(case, work)
    out, err = {}, []

    def run(i):
        try:
            ctx = V.BowContext(d["voc"], max_features=CAP, max_batch=NFRAMES)
            for _ in range(3):
                out[i] = ctx.transform_batch(d["frames"], d["counts"], case[4])
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not err, err
    for i in range(2):
        assert all(same_vectors(a, b) for a, b in zip(out[i], d["dev"]))


def test_malformed_vocabularies_are_refused(work, tmp_path):
    from se2lam_amd import capi, vocabulary as V
    parent, desc, weight, leaf = V.synthetic_vocabulary(9, 4, 3, full=False, early_leaf=0.2)
    good = tmp_path / "voc.bin"
    V.write_vocabulary_file(good, 4, 3, 0, 0, parent, desc, weight, leaf)
    assert V.Vocabulary.load(good).words == int(leaf.sum())
    blob = good.read_bytes()
    last_leaf = 24 + 41 * (len(parent) - 2) + 40
    cases = {"truncated": blob[:-17], "node size": blob[:4] + struct.pack("<I", 40) + blob[8:],
             "forward parent": blob[:24] + struct.pack("<i", 5) + blob[28:], "empty": b"",
             "childless inner node": blob[:last_leaf] + b"\x00" + blob[last_leaf + 1:]}
    frames = struct.pack("<iii", 1, 4, 4) + desc[1:5].tobytes()
    (tmp_path / "in.bin").write_bytes(frames)
    for name, data in cases.items():
        p = tmp_path / (name.replace(" ", "_") + ".bin")
        p.write_bytes(data)
        with pytest.raises(capi.Se2GpuError) as e:
            V.Vocabulary.load(p)
        assert e.value.code == capi.ERR_INVALID, name
        r = subprocess.run([work[1], "transform", str(p), str(tmp_path / "in.bin"), "1", str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert r.returncode == 1 and "LOAD failed" in r.stdout, name          # ... as the host vocabulary refuses it
    with pytest.raises(capi.Se2GpuError):
        V.Vocabulary.load(tmp_path / "missing.bin")
    bad = parent.copy(); bad[3] = 7
    noleaf = leaf.copy(); noleaf[-1] = False
    for args in ((4, 3, 0, 0, bad, desc, weight, leaf), (4, 3, 0, 0, parent, desc, weight, noleaf), (0, 3, 0, 0, parent, desc, weight, leaf),
                 (4, 3, 6, 0, parent, desc, weight, leaf), (4, 3, 0, 4, parent, desc, weight, leaf)):
        with pytest.raises(capi.Se2GpuError) as e:
            V.Vocabulary(*args)
        assert e.value.code == capi.ERR_INVALID
    # se2gpu_voc_create == se2gpu_voc_load on good records
    a, b = V.Vocabulary(4, 3, 0, 0, parent, desc, weight, leaf), V.Vocabulary.load(good)
    f = desc[np.nonzero(leaf)[0][:50]]
    assert same_vectors(V.BowContext(a, 64).transform(f, 1), V.BowContext(b, 64).transform(f, 1))
    # capacities
    ctx = V.BowContext(a, 16, 1)
    with pytest.raises(capi.Se2GpuError) as e:
        ctx.transform(desc[:17], 1)
    assert e.value.code == capi.ERR_CAPACITY
    with pytest.raises(capi.Se2GpuError) as e:
        V.BowContext(a, 5000, 1)
    assert e.value.code == capi.ERR_INVALID


# ---- scoring ---------------------------------------------------------------------------------------------------------------
def replay_detect_loop(scores, kf_ids, cur, min_off):
    """GlobalMapper::DetectLoopClose / Localizer::DetectLoopClose over given scores"""
    best, entry = 0.0, -1
    for i, (s, kf) in enumerate(zip(scores, kf_ids)):
        if abs(int(kf) - cur) < min_off:
            continue
        if s > best:
            best, entry = float(s), i
    return entry, (int(kf_ids[entry]) if entry >= 0 else -1), best


def scoring_data(scoring, work, nq=5, ndb=300):
    """BowVectors of nq + ndb frames of ~150 features from the device transform (= the host vocabulary's, see above); the
    queries share features with some entries"""
    from se2lam_amd import vocabulary as V
    tmp, exe = work
    k, L, weighting = 6, 4, 0
    parent, desc, weight, leaf = V.synthetic_vocabulary(40 + scoring, k, L, weighting, full=False)
    path = tmp / ("score_voc_%d.bin" % scoring)
    V.write_vocabulary_file(path, k, L, scoring, weighting, parent, desc, weight, leaf)
    rng = np.random.default_rng(scoring)
    leaves = np.nonzero(leaf)[0]
    n, cap = nq + ndb, 160
    frames = np.zeros((n, cap, 32), np.uint8)
    counts = rng.integers(100, cap + 1, n).astype(np.int32)
    for f in range(n):
        c = int(counts[f])
        frames[f, :c] = desc[rng.choice(leaves, c)] ^ np.packbits(rng.random((c, 256)) < 0.02, axis=1)
    for q in range(nq):                                              # a query sees what some key frames saw
        for j, e in enumerate(rng.choice(ndb, 6, replace=False)):
            frames[q, 15 * j:15 * (j + 1)] = frames[nq + e, 15 * j:15 * (j + 1)]
    voc = V.Vocabulary.load(path)
    ctx = V.BowContext(voc, cap, n)
    vecs = [(w, v) for w, v, _ in ctx.transform_batch(frames, counts, 2)]
    return voc, ctx, path, vecs[:nq], vecs[nq:]


@pytest.mark.parametrize("scoring", [0, 1, 2, 4, 5])
def test_scores_equal_the_host_vocabulary(scoring, work):
    from se2lam_amd import vocabulary as V
    tmp, exe = work
    voc, ctx, path, queries, entries = scoring_data(scoring, work)
    want = mirror_scores(exe, path, queries, entries, tmp)
    db = V.BowDatabase(voc)
    kf_ids = [5 + 2 * i for i in range(len(entries))]
    for kf, (w, v) in zip(kf_ids, entries):
        db.add(kf, w, v)
    assert len(db) == len(entries) == 300
    rv = ref.RefVocabulary(path) if ref.available() else None
    for q, (w, v) in enumerate(queries):
        got, entry, kf, best = db.query(ctx, w, v)
        print("scoring %d query %d: %d scores above 0, best %.6g" % (scoring, q, int((want[q] > 0).sum()), want[q].max()))
        assert (want[q] > 0).sum() >= 6
        assert np.array_equal(got, want[q])
        assert (entry, kf, best) == replay_detect_loop(want[q], kf_ids, 0, 0)
        if rv is not None:
            for e in range(len(entries)):
                assert got[e] == pytest.approx(rv.score((w, v), entries[e]), rel=1e-14, abs=1e-16)
        # the query read from device memory gives the same
        from se2lam_amd import capi
        dw, dv = capi.DeviceArray.from_numpy(w), capi.DeviceArray.from_numpy(v)
        got2, entry2, kf2, best2 = db.query(ctx, dw.ptr, dv.ptr, n=len(w))
        assert np.array_equal(got2, got) and (entry2, kf2, best2) == (entry, kf, best)


def test_kl_scoring_is_refused_at_create(work):
    from se2lam_amd import capi, vocabulary as V
    parent, desc, weight, leaf = V.synthetic_vocabulary(1, 4, 3)
    voc = V.Vocabulary(4, 3, V.KL, V.TF_IDF, parent, desc, weight, leaf)
    with pytest.raises(capi.Se2GpuError) as e:
        V.BowDatabase(voc)
    assert e.value.code == capi.ERR_INVALID and "KL" in str(e.value)
    w, v, fv = V.BowContext(voc, 64).transform(desc[np.nonzero(leaf)[0][:40]], 1)      # transform does not depend on the scoring's score()
    assert len(w) > 0 and abs(v.sum() - 1.0) < 1e-12


def test_loop_candidate_is_the_one_detect_loop_close_keeps(work):
    from se2lam_amd import vocabulary as V
    tmp, exe = work
    voc, ctx, path, queries, entries = scoring_data(0, work)
    entries = list(entries)
    qw, qv = queries[0]
    entries[40] = (qw.copy(), qv.copy())            # two entries identical to the query, at different positions: both score 1
    entries[200] = (qw.copy(), qv.copy())
    kf_ids = [5 + 2 * i for i in range(len(entries))]
    want = mirror_scores(exe, path, queries, entries, tmp)
    db = V.BowDatabase(voc)
    for kf, (w, v) in zip(kf_ids, entries):
        db.add(kf, w, v)
    got, entry, kf, best = db.query(ctx, qw, qv, cur_kf_id=1000, min_kfid_offset=0)
    assert np.array_equal(got, want[0]) and got[40] == got[200] == got.max()
    assert (entry, kf, best) == replay_detect_loop(want[0], kf_ids, 1000, 0) and entry == 40       # the earlier of the two
    for q, (w, v) in enumerate(queries):
        for cur, off in ((1000, 0), (kf_ids[40] + 3, 30), (kf_ids[200] - 29, 30), (kf_ids[120], 30), (kf_ids[120], 10 ** 6)):
            got, entry, kf, best = db.query(ctx, w, v, cur_kf_id=cur, min_kfid_offset=off)
            assert (entry, kf, best) == replay_detect_loop(want[q], kf_ids, cur, off), (q, cur, off)
    assert db.query(ctx, qw, qv, kf_ids[40] + 3, 30)[1] == 200             # entry 40 is too close to the current key frame
    assert db.query(ctx, qw, qv, kf_ids[120], 10 ** 6)[1:] == (-1, -1, 0.0)   # nobody is far enough
    # Map::pruneRedundantKF deletes the best: the next one wins, the order is kept
    db.remove(kf_ids[40])
    kept = [i for i in range(len(entries)) if i != 40]
    got, entry, kf, best = db.query(ctx, qw, qv, 1000, 0)
    assert len(db) == 299 and np.array_equal(got, want[0][kept])
    assert (entry, kf) == (199, kf_ids[200]) == replay_detect_loop(want[0][kept], [kf_ids[i] for i in kept], 1000, 0)[:2]
    db.remove(kf_ids[200])
    kept.remove(200)
    got, entry, kf, best = db.query(ctx, qw, qv, 1000, 0)
    assert np.array_equal(got, want[0][kept]) and (entry, kf, best) == replay_detect_loop(want[0][kept], [kf_ids[i] for i in kept], 1000, 0)
    db.add(7777, qw, qv)                                                   # a new key frame goes to the end
    got, entry, kf, best = db.query(ctx, qw, qv, 1000, 0)
    assert len(db) == 299 and np.array_equal(got[:-1], want[0][kept]) and (entry, kf) == (298, 7777) and got[-1] == want[0][40]
    from se2lam_amd import capi
    with pytest.raises(capi.Se2GpuError):
        db.remove(123456)
    # a data base in which nothing scores above 0: no word in common
    nothing = V.BowDatabase(voc)
    others = np.setdiff1d(np.arange(voc.words, dtype=np.uint32), qw)
    for i in range(20):
        w = np.sort(np.random.default_rng(i).choice(others, 50, replace=False)).astype(np.uint32)
        nothing.add(i, w, np.full(50, 1.0 / 50))
    got, entry, kf, best = nothing.query(ctx, qw, qv, 1000, 0)
    assert (got == 0).all() and (entry, kf, best) == (-1, -1, 0.0)
    assert V.BowDatabase(voc).query(ctx, qw, qv)[1:] == (-1, -1, 0.0)      # and an empty one


# ---- end to end on the device -------------------------------------------------------------------------------------------
def test_extract_transform_search_and_query_on_the_device(work, synth):
    """se2gpu_orb_extract_batch_device -> se2gpu_bow_transform_batch_device on the descriptors where they lie -> the CSR into
    se2gpu_search_by_bow; -> se2gpu_bowdb_add_device -> query: all equal to the route over downloaded descriptors and the host
    vocabulary"""
    from se2lam_amd import capi, orb, vocabulary as V
    from se2lam_amd.matcher import ORBmatcher
    tmp, exe = work
    imgs = np.stack([synth.frame(0), synth.frame(1)])
    B, rows, cols = imgs.shape
    cap = 2000
    ex = orb.ORBextractor(max_batch=2)
    D = capi.DeviceArray
    d_img, d_kps, d_desc, d_cnt = D.from_numpy(imgs), D(B * cap * 28), D(B * cap * 32), D(B * 4)
    ex.extract_batch_device(d_img.ptr, B, rows, cols, d_kps.ptr, d_desc.ptr, d_cnt.ptr, cap)
    ex.sync()
    cnt = d_cnt.to_numpy(np.int32, (B,))
    kps, desc = d_kps.to_numpy(capi.KP_DTYPE, (B, cap)), d_desc.to_numpy(np.uint8, (B, cap, 32))
    assert cnt.min() > 300
    # a small vocabulary "trained" on the scene, as in tests/test_vocabulary.py
    rng = np.random.default_rng(4)
    k, L = 8, 3
    parent, depth, desc_v, leaf, weight = V_tree(rng, k, L, desc[0, :cnt[0]])
    path = tmp / "scene_voc.bin"
    V.write_vocabulary_file(path, k, L, 0, 0, parent, desc_v, weight, leaf)
    voc = V.Vocabulary.load(path)
    ctx = V.BowContext(voc, cap, B)
    bw, bv, bn = D(4 * B * cap), D(8 * B * cap), D(4 * B)
    fn, fp, fi, nn = D(4 * B * cap), D(4 * B * (cap + 1)), D(4 * B * cap), D(4 * B)
    ctx.transform_batch_device(d_desc.ptr, d_cnt.ptr, cap, B, 2, bw.ptr, bv.ptr, bn.ptr, fn.ptr, fp.ptr, fi.ptr, nn.ptr)
    db = V.BowDatabase(voc)
    for f in range(B):                                                   # straight from the transform's output, same stream
        db.add_device(ctx, 10 + f, bw.ptr.value + 4 * f * cap, bv.ptr.value + 8 * f * cap, bn.ptr.value + 4 * f, cap)
    ctx.sync()
    h_bn, h_nn = bn.to_numpy(np.int32, B), nn.to_numpy(np.int32, B)
    h_bw, h_bv = bw.to_numpy(np.uint32, (B, cap)), bv.to_numpy(np.float64, (B, cap))
    h_fn, h_fp, h_fi = fn.to_numpy(np.int32, (B, cap)), fp.to_numpy(np.int32, (B, cap + 1)), fi.to_numpy(np.int32, (B, cap))
    host = mirror_transform(exe, path, desc, cnt, 2, tmp)                 # the route over downloaded descriptors
    fvs = []
    for f in range(B):
        got = (h_bw[f, :h_bn[f]], h_bv[f, :h_bn[f]], (h_fn[f, :h_nn[f]], h_fp[f, :h_nn[f] + 1], h_fi[f, :h_fp[f, h_nn[f]]]))
        assert same_vectors(got, host[f]) and len(got[0]) > 50
        fvs.append(got[2])
    m = ORBmatcher(0.9)
    k1, k2, d1, d2 = kps[0, :cnt[0]], kps[1, :cnt[1]], desc[0, :cnt[0]], desc[1, :cnt[1]]
    h1, h2 = np.ones(cnt[0], np.uint8), np.ones(cnt[1], np.uint8)
    nm, m12 = m.SearchByBoW(k1, d1, fvs[0], h1, k2, d2, fvs[1], h2, False)
    nm_h, m12_h = m.SearchByBoW(k1, d1, host[0][2], h1, k2, d2, host[1][2], h2, False)
    assert nm == nm_h > 100 and np.array_equal(m12, m12_h)
    want = mirror_scores(exe, path, [host[0][:2], host[1][:2]], [host[0][:2], host[1][:2]], tmp)
    for f in range(B):                                                   # the query is the device slice as well
        got, entry, kf, best = db.query(ctx, bw.ptr.value + 4 * f * cap, bv.ptr.value + 8 * f * cap, n=int(h_bn[f]))
        assert np.array_equal(got, want[f]) and (entry, kf) == (f, 10 + f) and 0 < got[1 - f] < got[f]


def V_tree(rng, k, L, d1):
    parent, depth, frontier = [0], [0], [0]
    for lv in range(1, L + 1):
        nxt = []
        for p in frontier:
            for _ in range(k):
                parent.append(p); depth.append(lv); nxt.append(len(parent) - 1)
        frontier = nxt
    n = len(parent)
    parent = np.array(parent, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    for i in range(1, n):
        if parent[i] == 0:
            desc[i] = d1[rng.integers(0, len(d1))]
        else:
            desc[i] = desc[parent[i]] ^ np.packbits(rng.random((32, 8)) < 0.05 * depth[i], axis=1).reshape(32)
    leaf = np.array(depth) == L
    return parent, depth, desc, leaf, np.where(leaf, 1.0, 0.0).astype(np.float32)


def test_cpp_class_gives_the_host_class_results(work, tmp_path):
    """include/se2lam_amd/ORBVocabularyDevice.h: the reference's call lines, BowDatabaseDevice::scoreAll / detectLoop"""
    from se2lam_amd import vocabulary as V
    libdir = os.path.join(ROOT, "se2lam_amd", "lib")
    exe = str(tmp_path / "cpp_bow_device")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp_bow_device_compile.cpp"), "-o", exe, "-L", libdir, "-lse2gpu", "-Wl,-rpath," + libdir])
    parent, desc, weight, leaf = V.synthetic_vocabulary(11, 10, 4, full=False, tie_frac=0.2)
    V.write_vocabulary_file(tmp_path / "voc.bin", 10, 4, 0, 0, parent, desc, weight, leaf)
    rng = np.random.default_rng(5)
    leaves = np.nonzero(leaf)[0]
    a = desc[rng.choice(leaves, 700)] ^ np.packbits(rng.random((700, 256)) < 0.03, axis=1)
    b = desc[rng.choice(leaves, 650)] ^ np.packbits(rng.random((650, 256)) < 0.03, axis=1)
    b[:200] = a[:200]
    (tmp_path / "a.bin").write_bytes(a.tobytes()); (tmp_path / "b.bin").write_bytes(b.tobytes())
    r = subprocess.run([exe, str(tmp_path / "voc.bin"), str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), "4"], capture_output=True, text=True)
    assert r.returncode == 0 and "device vocabulary ran" in r.stdout, r.stdout + r.stderr
