"""An independent numpy model of se2gpu_mappoint_parallax_batch_device and se2gpu_kf_correspd_batch_device
(MapPoint::updateParallax, src/MapPoint.cpp:124-185, and LocalMapper::findCorrespd, src/LocalMapper.cpp:87-170 of the
reference, with Track::calcSE3toXYZInfo, Track.cpp:259-306, and MapPoint::acceptNewObserve, MapPoint.cpp:202-209).

The selection rules (which entry is pKF0, which pass takes a feature) are written once and take a LAYER for the arithmetic:
  L64  the definitions in FP64: LAPACK's SVD for the DLT, the closed-form Rodrigues matrix, R = I on the optical axis
  L32  the float32 restatement, operation by operation as the reference (with the cv::Mat stand-in of oracle/_shim) computes:
       Point3f / Matx33f arithmetic in float in index order, cv::norm in double and narrowed, asinf, Rodrigues and the sums
       of a cv::Mat product in double, one-sided Jacobi in FP64 on the float32 rows
Both read the same float32 inputs.  `margins`, when a list, collects (name, value, threshold) of every gated quantity.
"""
import math

import numpy as np

f32 = np.float32
SENT = -7.0          # float outputs the calls leave alone
MIN_COS = 0.9994     # cvu::checkParallax, minDegree 2
COS_ANGLE = 0.866    # MapPoint::acceptNewObserve


class L64:
    dtype = np.float64

    @staticmethod
    def se3map(T, p):
        T = np.asarray(T, np.float64).reshape(3, 4)
        return T[:, :3] @ np.asarray(p, np.float64) + T[:, 3]

    @staticmethod
    def triangulate(pt1, pt2, P1, P2):
        P1, P2 = np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4)
        A = np.stack([float(pt1[0]) * P1[2] - P1[0], float(pt1[1]) * P1[2] - P1[1],
                      float(pt2[0]) * P2[2] - P2[0], float(pt2[1]) * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][3]
        return v[:3] / v[3]

    @staticmethod
    def rodrigues(k):
        theta = np.linalg.norm(k)
        if theta == 0.0:
            return np.eye(3)
        x, y, z = k / theta
        K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)

    @classmethod
    def view_info(cls, xyz, length, dxy, dz):
        D = np.diag([1.0 / dxy ** 2, 1.0 / dxy ** 2, 1.0 / dz ** 2])
        k = np.cross(xyz, [0.0, 0.0, length])
        nk = np.linalg.norm(k)
        if nk == 0.0:
            return D                                   # the limit on the optical axis (the reference divides 0 by 0 there)
        R = cls.rodrigues(k * (math.asin(min(nk / (length * np.linalg.norm(xyz)), 1.0)) / nk))
        return R.T @ D @ R

    @classmethod
    def se3_to_xyz_info(cls, xyz1, Twc1, Tcw2, Twc2, fx, margins=None):
        xyz1 = np.asarray(xyz1, np.float64)
        O1, O2 = np.asarray(Twc1, np.float64).reshape(3, 4)[:, 3], np.asarray(Twc2, np.float64).reshape(3, 4)[:, 3]
        xyz = cls.se3map(Twc1, xyz1)
        v1, v2 = xyz - O1, xyz - O2
        sin_prl = np.linalg.norm(np.cross(v1, v2)) / (np.linalg.norm(v1) * np.linalg.norm(v2))
        if margins is not None:
            margins.append(("sinParallax", float(sin_prl), 0.0))
        xyz2 = cls.se3map(Tcw2, xyz)
        l1, l2 = np.linalg.norm(xyz1), np.linalg.norm(xyz2)
        dxy1, dxy2 = 2.0 * l1 / float(fx), 2.0 * l2 / float(fx)
        dz1, dz2 = dxy2 / sin_prl, dxy1 / sin_prl
        return cls.view_info(xyz1, l1, dxy1, dz1), cls.view_info(xyz2, l2, dxy2, dz2), xyz2

    @staticmethod
    def cos_parallax(o1, o2, p):
        p1, p2 = np.asarray(p, np.float64) - np.asarray(o1, np.float64), np.asarray(p, np.float64) - np.asarray(o2, np.float64)
        return abs(p1 @ p2) / (np.linalg.norm(p1) * np.linalg.norm(p2))

    @staticmethod
    def accept_terms(pos, normal):
        pos, normal = np.asarray(pos, np.float64), np.asarray(normal, np.float64)
        dist = np.linalg.norm(pos)
        return dist, abs(pos @ normal) / (dist * np.linalg.norm(normal))

    @staticmethod
    def at_m_a(A, M):
        A = np.asarray(A, np.float64)
        return A.T @ M @ A

    @staticmethod
    def a_m_at(A, M):
        A = np.asarray(A, np.float64)
        return A @ M @ A.T


def _norm3(v):                                         # cv::norm(Point3f): double
    x, y, z = float(v[0]), float(v[1]), float(v[2])
    return math.sqrt(x * x + y * y + z * z)


def _cross32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def _mul32(a, b):                                      # cv::Mat product, CV_32F: double accumulator, float element
    out = np.zeros((3, 3), f32)
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                s += float(a[r, k]) * float(b[k, c])
            out[r, c] = f32(s)
    return out


def jacobi_smallest_right_singular_vector(A):
    """one-sided Jacobi (Hestenes) on A^T in FP64, as cv::SVD's JacobiSVDImpl_ runs it; A: 4x4 doubles"""
    At = [[float(A[k][i]) for k in range(4)] for i in range(4)]
    Vt = [[1.0 if i == k else 0.0 for k in range(4)] for i in range(4)]
    W = []
    for i in range(4):
        sd = 0.0
        for k in range(4):
            sd += At[i][k] * At[i][k]
        W.append(sd)
    eps = 2.220446049250313e-16 * 10
    for _ in range(30):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                a, p, b = W[i], 0.0, W[j]
                for k in range(4):
                    p += At[i][k] * At[j][k]
                if abs(p) <= eps * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = math.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = math.sqrt(delta / gamma)
                    c = p / (gamma * s * 2)
                else:
                    c = math.sqrt((gamma + beta) / (gamma * 2))
                    s = p / (gamma * c * 2)
                a = b = 0.0
                for k in range(4):
                    t0 = c * At[i][k] + s * At[j][k]
                    t1 = -s * At[i][k] + c * At[j][k]
                    At[i][k], At[j][k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                for k in range(4):
                    t0 = c * Vt[i][k] + s * Vt[j][k]
                    t1 = -s * Vt[i][k] + c * Vt[j][k]
                    Vt[i][k], Vt[j][k] = t0, t1
        if not changed:
            break
    m = 0
    for i in range(1, 4):
        if W[i] < W[m]:
            m = i
    return Vt[m]


class L32:
    dtype = np.float32

    @staticmethod
    def se3map(T, p):
        T, p = np.asarray(T, f32).reshape(3, 4), np.asarray(p, f32)
        return np.array([(T[i, 0] * p[0] + T[i, 1] * p[1] + T[i, 2] * p[2]) + T[i, 3] for i in range(3)], f32)

    @staticmethod
    def triangulate(pt1, pt2, P1, P2):
        P1, P2 = np.asarray(P1, f32).reshape(3, 4), np.asarray(P2, f32).reshape(3, 4)
        x1, y1, x2, y2 = f32(pt1[0]), f32(pt1[1]), f32(pt2[0]), f32(pt2[1])
        A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]])
        assert A.dtype == np.float32
        v = jacobi_smallest_right_singular_vector(A.astype(np.float64))
        w = f32(v[3])
        return np.array([f32(v[0]) / w, f32(v[1]) / w, f32(v[2]) / w], f32)

    @staticmethod
    def rodrigues(k):
        r = [float(k[0]), float(k[1]), float(k[2])]
        theta = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        R = np.eye(3)
        if not theta < np.finfo(np.float64).eps:
            if math.isnan(theta):
                return np.full((3, 3), np.nan, f32)
            c, s = math.cos(theta), math.sin(theta)
            c1, it = 1.0 - c, (1.0 / theta if theta else 0.0)
            x, y, z = r[0] * it, r[1] * it, r[2] * it
            rrt = [x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z]
            rx = [0, -z, y, z, 0, -x, -y, x, 0]
            I = [1, 0, 0, 0, 1, 0, 0, 0, 1]
            R = np.array([c * I[i] + c1 * rrt[i] + s * rx[i] for i in range(9)]).reshape(3, 3)
        return R.astype(f32)

    @classmethod
    def view_info(cls, xyz, length, dxy, dz):
        one = f32(1)
        ixy, iz = one / (dxy * dxy), one / (dz * dz)
        D = np.array([[ixy, 0, 0], [0, ixy, 0], [0, 0, iz]], f32)
        z = np.array([0, 0, length], f32)
        k = _cross32(xyz, z)
        normk = f32(_norm3(k))
        sn = f32(float(normk) / (_norm3(z) * _norm3(xyz)))
        f = np.arcsin(sn) / normk                       # std::asin(float) / float
        assert isinstance(f, np.float32)
        R = cls.rodrigues(np.array([k[0] * f, k[1] * f, k[2] * f], f32))
        return _mul32(_mul32(R.T, D), R)

    @classmethod
    def se3_to_xyz_info(cls, xyz1, Twc1, Tcw2, Twc2, fx, margins=None):
        with np.errstate(all="ignore"):
            xyz1, fx = np.asarray(xyz1, f32), f32(fx)
            O1, O2 = np.asarray(Twc1, f32).reshape(3, 4)[:, 3], np.asarray(Twc2, f32).reshape(3, 4)[:, 3]
            xyz = cls.se3map(Twc1, xyz1)
            v1, v2 = xyz - O1, xyz - O2
            sin_prl = f32(_norm3(_cross32(v1, v2)) / (_norm3(v1) * _norm3(v2)))
            xyz2 = cls.se3map(Tcw2, xyz)
            l1, l2 = f32(_norm3(xyz1)), f32(_norm3(xyz2))
            dxy1, dxy2 = f32(2) * l1 / fx, f32(2) * l2 / fx
            dz1, dz2 = dxy2 / sin_prl, dxy1 / sin_prl
            return cls.view_info(xyz1, l1, dxy1, dz1), cls.view_info(xyz2, l2, dxy2, dz2), xyz2

    @staticmethod
    def cos_parallax(o1, o2, p):
        p, o1, o2 = np.asarray(p, f32), np.asarray(o1, f32), np.asarray(o2, f32)
        p1, p2 = p - o1, p - o2
        dot = p1[0] * p2[0] + p1[1] * p2[1] + p1[2] * p2[2]
        return f32(abs(float(dot)) / (_norm3(p1) * _norm3(p2)))

    @staticmethod
    def accept_terms(pos, normal):
        pos, normal = np.asarray(pos, f32), np.asarray(normal, f32)
        dist = f32(_norm3(pos))
        dot = pos[0] * normal[0] + pos[1] * normal[1] + pos[2] * normal[2]
        return dist, f32(abs(float(dot)) / (float(dist) * _norm3(normal)))

    @staticmethod
    def at_m_a(A, M):
        A = np.asarray(A, f32)
        return _mul32(_mul32(A.T, M), A)

    @staticmethod
    def a_m_at(A, M):
        A = np.asarray(A, f32)
        return _mul32(_mul32(A, M), A.T)


def _const(L, v):
    return f32(v) if L is L32 else float(v)


def accept_new_observe(L, pos, normal, main_octave, kp_octave, min_dist, max_dist, margins=None):
    dist, cos_angle = L.accept_terms(pos, normal)
    if margins is not None:
        margins += [("cosAngle", float(cos_angle), COS_ANGLE), ("dist_min", float(dist), float(min_dist)),
                    ("dist_max", float(dist), float(max_dist))]
    c1 = abs(int(main_octave) - int(kp_octave)) <= 2
    c2 = cos_angle >= _const(L, f32(COS_ANGLE))
    c3 = _const(L, min_dist) <= dist <= _const(L, max_dist)
    return bool(c1 and c2 and c3)


def _depth_ok(L, z, lower, upper, margins):
    if margins is not None:
        margins += [("depth_lower", float(z), float(lower)), ("depth_upper", float(z), float(upper))]
    return _const(L, lower) <= z <= _const(L, upper)


class Frames:
    """the frame arrays of both calls: kps (nframes * cap, fields x, y, octave), counts, Tcw / Twc / P (nframes, 12) float32,
    idkf (nframes)"""

    def __init__(self, kps, counts, cap, Tcw, Twc, P, idkf):
        self.kps, self.counts, self.cap, self.nframes = kps, np.asarray(counts, np.int32), int(cap), len(counts)
        self.Tcw, self.Twc, self.P = (np.asarray(a, f32).reshape(self.nframes, 12) for a in (Tcw, Twc, P))
        self.idkf = np.asarray(idkf, np.int32)

    def offset(self, f, k):
        if not 0 <= f < self.nframes:
            return -1
        if not 0 <= k < min(int(self.counts[f]), self.cap):
            return -1
        return int(f) * self.cap + int(k)

    def pt(self, off):
        return self.kps["x"][off], self.kps["y"][off]

    def R(self, f):
        return self.Tcw[f].reshape(3, 4)[:, :3]


def parallax_batch(L, fr, mp_ptr, obs_frame, obs_ftr, good_prl, new_frame, fx, lower, upper, kf_observed=None, margins=None):
    m, nobs = len(mp_ptr) - 1, len(obs_frame)
    out = dict(status=np.zeros(m, np.int32), place=np.full(m, -1, np.int32), pos=np.full((m, 3), SENT, L.dtype),
               obs_view=np.full((max(nobs, 1), 3), SENT, L.dtype), obs_info=np.full((max(nobs, 1), 9), SENT, L.dtype),
               kf_observed=None if kf_observed is None else np.array(kf_observed, np.uint8).ravel().copy())
    for p in range(m):
        s, e = (min(max(int(v), 0), nobs) for v in (mp_ptr[p], mp_ptr[p + 1]))
        ent = [(i, int(obs_frame[s + i]), fr.offset(int(obs_frame[s + i]), int(obs_ftr[s + i]))) for i in range(max(e - s, 0))]
        ent = [t for t in ent if t[2] >= 0]
        fnew = int(new_frame[p])
        mine = [t for t in ent if t[1] == fnew]
        if good_prl[p] or len(ent) <= 2 or not mine:
            continue
        place1, _, off1 = mine[0]
        id1 = int(fr.idkf[fnew])
        best = None
        for t in ent:
            if id1 - int(fr.idkf[t[1]]) > 6:
                continue
            if best is None or int(fr.idkf[t[1]]) < int(fr.idkf[best[1]]):
                best = t
        place0, f0, off0 = best
        id0 = int(fr.idkf[f0])
        out["place"][p] = place0
        out["status"][p] = 3
        if f0 == fnew:
            continue
        posW = L.triangulate(fr.pt(off0), fr.pt(off1), fr.P[f0], fr.P[fnew])
        pos0, pos1 = L.se3map(fr.Tcw[f0], posW), L.se3map(fr.Tcw[fnew], posW)
        good = False
        d0, d1 = _depth_ok(L, pos0[2], lower, upper, margins), _depth_ok(L, pos1[2], lower, upper, margins)
        if d0 and d1:
            cosp = L.cos_parallax(fr.Twc[f0].reshape(3, 4)[:, 3], fr.Twc[fnew].reshape(3, 4)[:, 3], posW)
            if margins is not None:
                margins.append(("cosParallax", float(cosp), MIN_COS))
            good = cosp < _const(L, f32(MIN_COS))
        if not good:
            if id1 - id0 >= 6:
                out["status"][p] = 2
                if out["kf_observed"] is not None:
                    for _, _, off in ent:
                        out["kf_observed"][off] = 0
            continue
        out["status"][p] = 1
        out["pos"][p] = posW
        info0, info1, _ = L.se3_to_xyz_info(pos0, fr.Twc[f0], fr.Tcw[fnew], fr.Twc[fnew], fx, margins)
        infoW = L.at_m_a(fr.R(f0), info0)
        for i, f, off in ent:
            if i == place0:
                v, I = pos0, info0
            elif i == place1:
                v, I = pos1, info1
            elif int(fr.idkf[f]) in (id0, id1):
                continue
            else:
                v, I = L.se3map(fr.Tcw[f], posW), L.a_m_at(fr.R(f), infoW)
            out["obs_view"][s + i] = v
            out["obs_info"][s + i] = np.asarray(I).ravel()
    return out


EYE12 = np.eye(4, dtype=f32)[:3].ravel()


def correspd_batch(L, fr, kf_observed, view_pos, job_prev, job_new, Tcr, Trc, matched12, local_pos, match_idx_mp, mp, fx,
                   lower, upper, passes, margins=None):
    """mp: dict(main_frame, main_ftr, main_octave, normal (m, 3), dist (m, 2)) or None.  Returns the outputs of the call;
    kf_observed is a copy."""
    B, cap = len(job_prev), fr.cap
    obs = np.array(kf_observed, np.uint8).ravel().copy()
    m = 0 if mp is None else len(mp["main_frame"])
    out = dict(inv=np.full((B, cap), -1, np.int32), kind=np.zeros((B, cap), np.uint8), src=np.full((B, cap), -1, np.int32),
               view=np.full((B, cap, 3), SENT, L.dtype), info=np.full((B, cap, 9), SENT, L.dtype),
               new_pos_w=np.full((B, cap, 3), SENT, L.dtype), info_prev=np.full((B, cap, 9), SENT, L.dtype),
               counts=np.zeros((B, 5), np.int32))
    matched12 = np.asarray(matched12, np.int32).reshape(B, cap)
    for b in range(B):
        fp, fn = int(job_prev[b]), int(job_new[b])
        if not (0 <= fp < fr.nframes and 0 <= fn < fr.nframes) or fp == fn:
            continue
        n_prev, n_new = (min(int(fr.counts[f]), cap) for f in (fp, fn))
        for i in range(n_prev):
            j = int(matched12[b, i])
            if 0 <= j < n_new:
                if out["inv"][b, j] >= 0:
                    out["counts"][b, 4] += 1
                out["inv"][b, j] = max(out["inv"][b, j], i)
        tcr = np.asarray(Tcr, f32).reshape(B, 12)[b]
        for j in range(n_new):
            onew = fn * cap + j
            was = bool(obs[onew])
            i = int(out["inv"][b, j])
            oprev = fp * cap + max(i, 0)
            prev_obs = i >= 0 and bool(obs[oprev])
            kind, src, view, info = 0, -1, None, None
            if passes & 1 and i >= 0 and prev_obs:
                x = np.asarray(view_pos, f32).reshape(-1, 3)[oprev]
                _, info, _ = L.se3_to_xyz_info(x, EYE12, tcr, np.asarray(Trc, f32).reshape(B, 12)[b], fx, margins)
                view, kind, src = L.se3map(tcr, x), 1, i
            if kind == 0 and passes & 2 and not was:
                q = int(np.asarray(match_idx_mp, np.int32).reshape(B, cap)[b, j])
                if 0 <= q < m:
                    fm = int(mp["main_frame"][q])
                    om = fr.offset(fm, int(mp["main_ftr"][q]))
                    if om >= 0:
                        x3d = L.triangulate(fr.pt(om), fr.pt(onew), fr.P[fm], fr.P[fn])
                        pos = L.se3map(fr.Tcw[fn], x3d)
                        acc = accept_new_observe(L, pos, mp["normal"][q], mp["main_octave"][q], fr.kps["octave"][onew],
                                                 mp["dist"][q][0], mp["dist"][q][1], margins)
                        dep = _depth_ok(L, pos[2], lower, upper, margins)
                        if acc and dep:
                            info, _, _ = L.se3_to_xyz_info(pos, fr.Twc[fn], fr.Tcw[fm], fr.Twc[fm], fx, margins)
                            view, kind, src = pos, 2, q
            if kind == 0 and passes & 4 and not was and i >= 0 and not prev_obs:
                x = np.asarray(local_pos, f32).reshape(B, cap, 3)[b, i]
                ip, info, _ = L.se3_to_xyz_info(x, fr.Twc[fp], fr.Tcw[fn], fr.Twc[fn], fx, margins)
                out["new_pos_w"][b, j] = L.se3map(fr.Twc[fp], x)
                out["info_prev"][b, j] = np.asarray(ip).ravel()
                view, kind, src = L.se3map(tcr, x), 3, i
                obs[oprev] = 1
            if kind:
                out["view"][b, j] = view
                out["info"][b, j] = np.asarray(info).ravel()
                obs[onew] = 1
            out["kind"][b, j], out["src"][b, j] = kind, src
            out["counts"][b, kind] += 1
    out["kf_observed"] = obs
    return out


def near_threshold(margins, tol):
    """the gated quantities that lie within ten tolerances of their threshold (relative to the threshold; absolute for the
    sine of the parallax, whose threshold is 0)"""
    bad = []
    for name, v, thr in margins:
        if not math.isfinite(v) or abs(v - thr) <= 10 * tol * (abs(thr) if thr else 1.0):
            bad.append((name, v, thr))
    return bad


def rel_err_pos(got, want):
    """per position: |got - want| / |want|, rows of 3"""
    got, want = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(want, np.float64).reshape(-1, 3)
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def rel_err_mat(got, want):
    """per 3x3 matrix: the largest |got - want| against the largest |want|, rows of 9"""
    got, want = np.asarray(got, np.float64).reshape(-1, 9), np.asarray(want, np.float64).reshape(-1, 9)
    return np.abs(got - want).max(1) / np.abs(want).max(1)
