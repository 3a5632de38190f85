"""Hand-stated cases of the map update, one per rule of se2gpu_map_apply_batch_device, shared by the model's own test, the
host mirror's (tests/cpp_map_apply.cpp) and the device call's.  A case is the dict of tests/map_apply_model.py."""
import numpy as np

import map_apply_model as mm

f32 = np.float32
CAP, NFRAMES, M_CAP, NOBS_CAP = 16, 6, 48, 256


def view_of(f, k):
    return np.array([0.1 * f + 0.01 * k + 1.0, -0.5 + 0.02 * k, 2.0 + 0.3 * f], f32)


def base(lists=None, jobs=((1, 3),), **kw):
    """three frames of observations: p0 seen by frames 0, 1; p1 by 1; p2 by 0, 1, 2; p3 by 2 alone"""
    lists = [[(0, 1), (1, 2)], [(1, 3)], [(0, 5), (1, 5), (2, 5)], [(2, 7)]] if lists is None else lists
    c = mm.blank_case(kw.pop("cap", CAP), kw.pop("nframes", NFRAMES), kw.pop("m_cap", M_CAP), kw.pop("nobs_cap", NOBS_CAP))
    mm.set_lists(c, lists, view_of)
    for p in range(len(lists)):
        c["mp_normal"][p] = mm.unit(np.array([0.1 * p, 0.2, 1.0], f32))
        c["pos"][p] = [100.0 * p, -50.0, 3000.0]
        c["good_prl"][p] = p % 2
    mm.set_jobs(c, list(jobs))
    c.update(kw)
    return c


def row(c, b, j, kind, src, good=1):
    """row j of job b, with floats that tell the rows and their fields apart"""
    t = f32(1000 * b + 10 * j)
    c["kind"][b, j], c["src"][b, j] = kind, src
    c["view"][b, j] = [t + 1, t + 2, t + 3000]
    c["info"][b, j] = np.arange(9, dtype=f32) * f32(0.5) + t
    if kind == 3:
        c["new_pos_w"][b, j] = [t + 7, t + 8, t + 9]
        c["info_prev"][b, j] = np.arange(9, dtype=f32) * f32(0.25) - t
        if 0 <= src < c["cap"]:
            c["local_pos"][b, src] = [-t - 1, t + 5, 2500 + t]
            c["good_prl_row"][b, src] = good
    return c


def kind1_alone():
    c = base()
    return row(row(c, 0, 0, 1, 2), 0, 4, 1, 3)            # features 2 and 3 of frame 1 hold p0 and p1


def kind2_alone():
    return row(base(), 0, 2, 2, 3)                        # p3, which frame 1 does not see


def kind3_alone():
    c = base()                                            # src order 4, 6, 9 against j order 5, 7, 1
    return row(row(row(c, 0, 1, 3, 9, good=0), 0, 5, 3, 4), 0, 7, 3, 6)


def mixed(kinds=14):
    c = base(kinds=kinds)
    row(c, 0, 0, 1, 2)
    row(c, 0, 2, 2, 3)
    row(c, 0, 9, 3, 8)
    return row(c, 0, 3, 3, 11)


def two_jobs_one_point():
    c = base(jobs=((1, 3), (0, 4), (2, 5)))
    row(c, 0, 6, 2, 3)
    row(c, 1, 2, 2, 3)
    row(c, 2, 9, 1, 7)                                    # feature 7 of frame 2 holds p3 too
    row(c, 1, 4, 3, 12)
    return row(c, 0, 8, 3, 10)


def duplicate_claim():
    c = base()
    row(c, 0, 2, 2, 3)
    row(c, 0, 6, 2, 3)
    row(c, 0, 1, 3, 9)
    return row(c, 0, 8, 3, 9)                             # and two rows that want to create a point from one feature


def refused_targets():
    c = base()
    c["mp_null"][1] = 1                                   # p1 is null (its list goes in rule 1)
    row(c, 0, 0, 2, 1)                                    # a null point
    row(c, 0, 1, 2, -1)                                   # no point
    row(c, 0, 2, 2, 99)                                   # out of range
    row(c, 0, 3, 1, 9)                                    # a feature of frame 1 that holds nothing
    row(c, 0, 4, 1, 77)                                   # no such feature
    row(c, 0, 5, 3, 16)                                   # kind 3 from no feature
    c["kf_observed"][3 * CAP:3 * CAP + 6] = 1             # as the correspd call leaves them
    return row(c, 0, 7, 2, 3)                             # and one that is taken


def already_observed():
    c = base(jobs=((0, 1),))
    row(c, 0, 9, 2, 0)                                    # frame 1 holds p0 already
    return row(c, 0, 10, 2, 3)


def erase_null_frame():
    c = base(lists=[[(0, 1), (1, 2)], [(1, 3)], [(0, 5), (1, 5), (2, 5)], [(2, 7)], [(1, 9)], [(1, 10), (2, 10), (1, 11)]], jobs=())
    c["frame_null"][1] = 1                                # p1 and p4 are left empty; p5 loses two entries in list order
    return c


def erase_null_frame_and_add():
    c = erase_null_frame()
    mm.set_jobs(c, [(2, 4), (1, 5)])                      # the second job names a null frame and is skipped
    row(c, 0, 3, 2, 1)                                    # p1 becomes null in this call: refused
    row(c, 0, 4, 2, 5)
    row(c, 1, 4, 2, 0)
    return row(c, 0, 6, 3, 2)


def erase_null_point_and_status():
    c = base(jobs=())
    c["mp_null"][0] = 1
    c["parallax_status"][:4] = [0, 1, 2, 3]
    c["has_status"] = True
    return c


def invalid_old_entry():
    c = base(lists=[[(0, 1), (7, 0), (1, 2)], [(1, 15), (-1, 3)], [(0, 5), (1, 5), (2, 5)], [(2, 16)]])
    c["counts"][1] = 10                                   # feature 15 of frame 1 does not exist
    return row(c, 0, 1, 2, 0)


def long_list():
    """p1 holds 70 entries over frames 0..4; frame 0 is null, and a job appends to what is left"""
    big = [(f, k) for k in range(14) for f in range(5)]
    c = base(lists=[[(0, 15), (1, 15)], big, [(2, 14)]], jobs=((2, 5),))
    c["frame_null"][0] = 1
    return row(row(c, 0, 3, 2, 1), 0, 4, 1, 14)


def capacity_points():
    c = base(m_cap=5)
    return row(row(row(c, 0, 1, 3, 9), 0, 5, 3, 4), 0, 2, 2, 3)


def capacity_entries():
    c = base(nobs_cap=8)
    return row(row(c, 0, 2, 2, 3), 0, 5, 3, 4)


def bad_jobs():
    c = base(jobs=((1, 1), (0, 9), (-1, 2), (2, 3)))
    for b in range(4):
        row(c, b, 2, 2, 3)
    return c


def no_entry_rows():
    c = mixed()
    c["has_rows"] = False
    return c


def random_case(seed, cap=64, nframes=8, m_cap=3000, m_old=2800, jobs=((0, 5), (1, 6), (2, 7)), nrows=40):
    """a consistent table (a feature belongs to one point at most) spread over m_old slots, so that the scan over the points
    spans a dozen workgroups; lists of 0 to 3; random rows of every kind, some of them refused"""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(m_old)]
    feats = [(f, k) for f in range(nframes) for k in range(cap - 8)]
    rng.shuffle(feats)
    at = 0
    for p in rng.permutation(m_old)[:len(feats) // 2]:
        n = int(rng.integers(1, 4))
        fr = set()
        while n and at < len(feats):
            f, k = feats[at]
            at += 1
            if f not in fr:
                fr.add(f)
                lists[p].append((int(f), int(k)))
                n -= 1
    c = mm.blank_case(cap, nframes, m_cap, 4 * len(feats))
    mm.set_lists(c, lists, view_of)
    c["mp_normal"][:] = rng.normal(size=(m_cap, 3)).astype(f32)
    c["good_prl"][:m_old] = rng.integers(0, 2, m_old)
    c["frame_null"][3] = 1
    c["parallax_status"][:] = rng.choice([0, 1, 2, 3], m_cap, p=[0.7, 0.1, 0.1, 0.1])
    c["has_status"] = True
    mm.set_jobs(c, list(jobs))
    full = [p for p in range(m_old) if lists[p]]
    for b in range(len(jobs)):
        js = rng.permutation(cap - 4)[:nrows]
        srcs3 = rng.permutation(cap)[:nrows]
        for n, j in enumerate(js):
            kind = int(rng.integers(1, 4))
            src = int(srcs3[n]) if kind != 2 else int(rng.choice(full) if rng.random() < 0.8 else rng.integers(-2, m_cap))
            row(c, b, int(j), kind, src, good=int(rng.integers(0, 2)))
    return c


def many_frames():
    """more frame slots than a launch has rows (65,535): 66,000 slots of one feature, two of them null"""
    c = base(lists=[[(65990, 0), (3, 0)], [(7, 0)], [(65999, 0)]], jobs=((3, 65998),), cap=1, nframes=66000)
    c["frame_null"][[65990, 65999]] = 1
    return row(c, 0, 0, 2, 1)


CASES = dict(many_frames=many_frames, kind1_alone=kind1_alone, kind2_alone=kind2_alone, kind3_alone=kind3_alone, mixed=mixed,
             mixed_kind1_only=lambda: mixed(2), mixed_kinds_2_3=lambda: mixed(12), two_jobs_one_point=two_jobs_one_point,
             duplicate_claim=duplicate_claim, refused_targets=refused_targets, already_observed=already_observed,
             erase_null_frame=erase_null_frame, erase_null_frame_and_add=erase_null_frame_and_add,
             erase_null_point_and_status=erase_null_point_and_status, invalid_old_entry=invalid_old_entry, long_list=long_list,
             capacity_points=capacity_points, capacity_entries=capacity_entries, bad_jobs=bad_jobs, no_entry_rows=no_entry_rows,
             random_small=lambda: random_case(7, cap=32, nframes=8, m_cap=96, m_old=80, nrows=12),
             random_scan=lambda: random_case(11))


def compare(got, want, what="", keys=None, prefix=False):
    """every output of the call, bit for bit; after a capacity status only what that leaves defined.  prefix: the entry arrays
    up to nobs_new only (a table that has been written before holds older entries behind them)"""
    keys = keys or (mm.OUT_FIELDS if want["sizes_out"][0] == 0 else mm.INPLACE + ["sizes_out", "job_counts"])
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if prefix and k.startswith("obs_"):
            g, w = g[:want["sizes_out"][mm.NOBS_NEW]], w[:want["sizes_out"][mm.NOBS_NEW]]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        same = g.view(np.uint32) == w.view(np.uint32) if g.dtype == np.float32 else g == w
        assert same.all(), (what, k, np.argwhere(~same)[:5].tolist(), g[~same][:5], w[~same][:5])


def dump(c, path):
    """the case as tests/cpp_map_apply.cpp reads it"""
    z = {k: int(c[k]) for k in mm.SIZE_KEYS}
    with open(path, "wb") as f:
        f.write(np.array([z[k] for k in mm.SIZE_KEYS] + [c.get("has_frame_null", True), c.get("has_rows", True),
                                                           c.get("has_status", False)], np.int32).tobytes())
        for name, dt, shape in mm.CASE_FIELDS:
            a = np.ascontiguousarray(c[name], dt)
            assert a.shape == shape(z), (name, a.shape, shape(z))
            f.write(a.tobytes())


def load_out(c, path):
    """what tests/cpp_map_apply.cpp wrote for case c"""
    z = {k: int(c[k]) for k in mm.SIZE_KEYS}
    shapes = {name: (dt, shape(z)) for name, dt, shape in mm.CASE_FIELDS}
    shapes.update(mp_ptr_new=(np.int32, (z["m_cap"] + 1,)), obs_frame_new=(np.int32, (z["nobs_cap"],)),
                  obs_ftr_new=(np.int32, (z["nobs_cap"],)), obs_view_new=(np.float32, (z["nobs_cap"], 3)),
                  obs_info_new=(np.float32, (z["nobs_cap"], 9)), new_frame=(np.int32, (z["m_cap"],)), sizes_out=(np.int32, (9,)),
                  job_counts=(np.int32, (z["B"], 6)))
    raw, at, out = open(path, "rb").read(), 0, {}
    for k in mm.OUT_FIELDS:
        dt, sh = shapes[k]
        n = int(np.prod(sh)) * np.dtype(dt).itemsize
        out[k] = np.frombuffer(raw[at:at + n], dt).reshape(sh)
        at += n
    assert at == len(raw)
    return out
