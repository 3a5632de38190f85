"""A numpy statement of what se2gpu_local_ba_batch_device gathers (include/se2gpu.h), written from Map::loadLocalGraph
(src/Map.cpp:891-1053 of the reference) and independent of the library: the loops of the reference over the window's lists, with
the tables of the call standing in for the pointer graph.  No vectorisation, no sharing with the kernels.

load_local_graph(T, job_slot, win_out, local_row, ref_row, mp_row, caps) -> dict(status, counts, fixed, poses, o_i, o_j, o_meas,
o_info, lm_ptr, e_kf, e_uv, e_info, lms); the arrays are None for a status that gathers nothing (1-4)."""
import numpy as np

MAX_DEGREE = 64      # kWindowMaxDegree of the resident kernel
MAX_FREE = 64        # its 192 unknowns


def normalize_theta(theta):
    """g2o::SE2's constructor (normalize_theta of g2o/stuff/misc.h)"""
    if -np.pi <= theta < np.pi:
        return theta
    mult = np.floor(theta / (2 * np.pi))
    theta = theta - mult * 2 * np.pi
    if theta >= np.pi:
        theta -= 2 * np.pi
    if theta < -np.pi:
        theta += 2 * np.pi
    return theta


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def entry_valid(T, f, k):
    """the entry rule of obs_table.h, null observers included (MapPoint::getObservations skips them, :995)"""
    nframes = len(T["counts"])
    if not 0 <= f < nframes:
        return False
    if T["frame_null"] is not None and T["frame_null"][f]:
        return False
    return 0 <= k < min(int(T["counts"][f]), int(T["cap"]))


def point_entries(T, p):
    """the segment rule of obs_table.h"""
    nobs = len(T["obs_frame"])
    s = min(max(int(T["mp_ptr"][p]), 0), nobs)
    e = min(max(int(T["mp_ptr"][p + 1]), 0), nobs)
    return [(int(T["obs_frame"][i]), int(T["obs_ftr"][i])) for i in range(s, e)]


def edge_information(T, f, k, lw, sigma2):
    """Map.cpp:1024-1049, in double on the float tables; Sigma_rotxy and Sigma_z are floats there (:1043-1044)"""
    fx = np.float64(np.float32(T["K"][0, 0]))
    Sigma_u = np.eye(2) * np.float64(sigma2)
    lc = T["view_pos"][f, k].astype(np.float64)
    zc_inv = 1.0 / lc[2]
    zc_inv2 = zc_inv * zc_inv
    J_pi = np.array([[fx * zc_inv, 0, -fx * lc[0] * zc_inv2], [0, fx * zc_inv, -fx * lc[1] * zc_inv2]])
    Rcw = T["Tcw"][f].reshape(3, 4)[:, :3].astype(np.float64)
    pi = np.array([np.float64(T["Twb"][f, 0]), np.float64(T["Twb"][f, 1]), 0.0])
    J_pi_Rcw = J_pi @ Rcw
    J_rotxy = (J_pi_Rcw @ skew(lw - pi))[:2, :2]
    J_z = -J_pi_Rcw[:, 2:3]
    Sigma_rotxy = np.float64(np.float32(1.0 / T["xrot_info"]))
    Sigma_z = np.float64(np.float32(1.0 / T["z_info"]))
    Sigma_all = Sigma_rotxy * J_rotxy @ J_rotxy.T + Sigma_z * J_z @ J_z.T + Sigma_u
    det = Sigma_all[0, 0] * Sigma_all[1, 1] - Sigma_all[0, 1] * Sigma_all[1, 0]       # Eigen's 2 x 2 inverse: the adjugate over det
    return np.array([Sigma_all[1, 1], -Sigma_all[0, 1], Sigma_all[0, 0]]) / det


def cov_inverse(c):
    """Eigen's closed-form 3 x 3 inverse: cofactors over the determinant (:951-952)"""
    c = np.asarray(c, np.float64).reshape(3, 3)
    cof = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            r = [x for x in range(3) if x != i]
            q = [x for x in range(3) if x != j]
            cof[i, j] = (-1) ** (i + j) * (c[r[0], q[0]] * c[r[1], q[1]] - c[r[0], q[1]] * c[r[1], q[0]])
    det = c[0, 0] * cof[0, 0] + c[0, 1] * cof[0, 1] + c[0, 2] * cof[0, 2]
    return cof.T / det


def load_local_graph(T, job_slot, win_out, local_row, ref_row, mp_row, caps):
    nframes, m = len(T["counts"]), len(T["pos"])
    nlevels = len(T["level_sigma2"])
    null = T["frame_null"] if T["frame_null"] is not None else np.zeros(nframes, np.uint8)
    none = dict(fixed=None, poses=None, o_i=None, o_j=None, o_meas=None, o_info=None, lm_ptr=None, e_kf=None, e_uv=None, e_info=None,
                lms=None)

    def result(status, counts, **arrays):
        return dict(none, status=status, counts=np.array(list(counts) + [0] * (8 - len(counts)), np.int32), **arrays)

    n_local, n_ref, n_mp = int(win_out[0]), max(int(win_out[1]), 0), max(int(win_out[2]), 0)
    if not 0 <= job_slot < nframes or n_local < 0:
        return result(1, [])
    if (n_local > min(caps["kf_list_cap"], caps["max_local"]) or n_ref > min(caps["kf_list_cap"], caps["max_ref"])
            or n_mp > min(caps["mp_list_cap"], caps["max_mp"])):
        return result(2, [])
    mLocalGraphKFs = [int(x) for x in local_row[:n_local]]
    mRefKFs = [int(x) for x in ref_row[:n_ref]]
    mLocalGraphMPs = [int(x) for x in mp_row[:n_mp]]
    if any(not 0 <= f < nframes for f in mLocalGraphKFs + mRefKFs) or any(not 0 <= p < m for p in mLocalGraphMPs):
        return result(1, [])
    nLocalKFs, nRefKFs = len(mLocalGraphKFs), len(mRefKFs)

    # :899-912
    minKFid = -1
    if not mRefKFs:
        minKFid = min([int(T["frame_id"][f]) for f in mLocalGraphKFs], default=-1)
    # :918-932, :959-970
    fixed, poses = [], []
    for i, f in enumerate(mLocalGraphKFs + mRefKFs):
        kfid = int(T["frame_id"][f])
        fixed.append(1 if i >= nLocalKFs or (not mRefKFs and kfid == minKFid) or kfid == 1 else 0)
        poses.append([np.float64(T["Twb"][f, 0]), np.float64(T["Twb"][f, 1]), normalize_theta(np.float64(T["Twb"][f, 2]))])
    n_free = fixed.count(0)
    has_null = any(null[f] for f in mLocalGraphKFs)
    # :935-956
    o_i, o_j, o_meas, o_info = [], [], [], []
    self_loop = False
    if T["odo_to"] is not None:
        for i, f in enumerate(mLocalGraphKFs):
            t = int(T["odo_to"][f])
            self_loop |= t == f
            if not 0 <= t < nframes or t not in mLocalGraphKFs or null[t]:
                continue
            o_i.append(i)
            o_j.append(mLocalGraphKFs.index(t))
            o_meas.append(np.asarray(T["odo_meas"][f], np.float64))
            o_info.append(cov_inverse(T["odo_cov"][f]))
    # :980-1051
    lm_ptr, e_kf, e_uv, e_info, lms = [0], [], [], [], []
    entries, flags, maxdeg = 0, 0, 0
    for p in mLocalGraphMPs:
        lw = T["pos"][p].astype(np.float64)
        lms.append(lw)
        pKFs = set()                                            # getObservations() is a std::set: a frame counts once
        deg = 0
        for f, k in point_entries(T, p):
            entries += 1
            if not entry_valid(T, f, k):
                continue
            if f in mLocalGraphKFs:
                vertexIdKF = mLocalGraphKFs.index(f)
            elif f in mRefKFs:
                vertexIdKF = mRefKFs.index(f) + nLocalKFs
            else:
                continue
            if f in pKFs:
                continue
            pKFs.add(f)
            octave = int(T["kps_octave"][f, k])
            if not 0 <= octave < nlevels:
                flags |= 1
                continue
            e_kf.append(vertexIdKF)
            e_uv.append([np.float64(T["kps_xy"][f, k, 0]), np.float64(T["kps_xy"][f, k, 1])])
            e_info.append(edge_information(T, f, k, lw, T["level_sigma2"][octave]))
            deg += 1
        maxdeg = max(maxdeg, deg)
        lm_ptr.append(len(e_kf))
    E, O = len(e_kf), len(o_i)
    counts = [nLocalKFs + nRefKFs, n_free, n_mp, E, O, entries - E, flags]
    if E > caps["max_obs"] or n_free > MAX_FREE or self_loop:
        return result(2, counts)
    if has_null:
        return result(3, counts)
    if maxdeg > MAX_DEGREE:
        return result(4, counts)
    status = 5 if n_free == 0 or E + O == 0 else 0
    arr = lambda a, dtype, shape: np.asarray(a, dtype).reshape(shape)  # noqa: E731
    return result(status, counts, fixed=arr(fixed, np.uint8, (-1,)), poses=arr(poses, np.float64, (-1, 3)), o_i=arr(o_i, np.int32, (-1,)),
                  o_j=arr(o_j, np.int32, (-1,)), o_meas=arr(o_meas, np.float64, (-1, 3)), o_info=arr(o_info, np.float64, (-1, 3, 3)),
                  lm_ptr=arr(lm_ptr, np.int32, (-1,)), e_kf=arr(e_kf, np.int32, (-1,)), e_uv=arr(e_uv, np.float64, (-1, 2)),
                  e_info=arr(e_info, np.float64, (-1, 3)), lms=arr(lms, np.float64, (-1, 3)))


def batch(T, job_kf, win_out, local_list, ref_list, mp_list, caps, job_caps=None):
    """every job of a batch; job_caps: per-job overrides of the caps (the tests call the device once per distinct set)"""
    out = []
    for j in range(len(job_kf)):
        c = dict(caps, **(job_caps[j] if job_caps else {}))
        out.append(load_local_graph(T, int(job_kf[j]), win_out[j], local_list[j], ref_list[j], mp_list[j], c))
    return out
