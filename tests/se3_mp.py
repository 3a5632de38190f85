"""csrc/se3_math.h again, in mpmath at 50 digits: the same formulas function by function (g2o's SE3Quat exp / log with their
small-angle branches, Eigen's matrix-to-quaternion conversion, toVectorMQT / fromVectorMQT, adj, the two MQT Jacobians), and next
to them the EXACT exponential and logarithm.  Which branch a formula takes is decided on the double inputs by `branch_*`, in IEEE
double arithmetic written in the order the header has it (Python floats): a branch is a decision the device makes on rounded
numbers, and a test that lands one ulp from a threshold must ask for that decision, not for the one exact arithmetic would make.
Everything after the decision is 50-digit arithmetic.  A pose is (R, t): R a list of 9 (row-major), t a list of 3."""
import math

import mpmath as mp

mp.mp.dps = 50
F = mp.mpf
THETA_SMALL = 0.00001      # se3_exp
D_SMALL = 0.99999          # se3_log


def vec(x):
    return [F(float(v)) for v in x]


def pose(p12):
    p = vec(p12)
    return p[:9], p[9:12]


def flat(*parts):
    return [float(v) for part in parts for v in part]


def skew(v):
    return [0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0]


def mat3(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def matvec(A, v):
    return [A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2] for i in range(3)]


def eye_plus(*terms):
    return [(1 if i % 4 == 0 else 0) + sum(c * M[i] for c, M in terms) for i in range(9)]


# ---- branch decisions, in double ---------------------------------------------------------------------------------------------
def branch_quat(R):
    """0: trace > 0; 1 + i: the largest diagonal entry i, the first of equal ones (Eigen)"""
    R = [float(v) for v in R]
    if R[0] + R[4] + R[8] > 0:
        return 0
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    return 1 + i


def theta_double(u):
    u = [float(v) for v in u]
    return math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])


def branch_exp(u):
    return theta_double(u) < THETA_SMALL


def d_double(R):
    R = [float(v) for v in R]
    return 0.5 * (R[0] + R[4] + R[8] - 1)


def branch_log(R):
    return d_double(R) > D_SMALL


def branch_from_mqt(v):
    v = [float(x) for x in v]
    return 1 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5]) < 0


# ---- the header's formulas -----------------------------------------------------------------------------------------------------
def quat_raw(R, b):
    """(w, x, y, z) of branch b before the sign and the normalisation"""
    if b == 0:
        t = mp.sqrt(R[0] + R[4] + R[8] + 1)
        s = F(0.5) / t
        return [F(0.5) * t, (R[7] - R[5]) * s, (R[2] - R[6]) * s, (R[3] - R[1]) * s]
    if b == 1:
        t = mp.sqrt(R[0] - R[4] - R[8] + 1)
        s = F(0.5) / t
        return [(R[7] - R[5]) * s, F(0.5) * t, (R[3] + R[1]) * s, (R[6] + R[2]) * s]
    if b == 2:
        t = mp.sqrt(R[4] - R[8] - R[0] + 1)
        s = F(0.5) / t
        return [(R[2] - R[6]) * s, (R[1] + R[3]) * s, F(0.5) * t, (R[7] + R[5]) * s]
    t = mp.sqrt(R[8] - R[0] - R[4] + 1)
    s = F(0.5) / t
    return [(R[3] - R[1]) * s, (R[2] + R[6]) * s, (R[5] + R[7]) * s, F(0.5) * t]


def quat_of(R, b=None):
    q = quat_raw(R, branch_quat(R) if b is None else b)
    n = mp.sqrt(sum(x * x for x in q))
    s = (-1 if q[0] < 0 else 1) / n
    return [x * s for x in q]


def mat_of_quat(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def normalize_rotation(R, b=None):
    return mat_of_quat(quat_of(R, b))


def se3_mul(A, B, b=None):
    """b: the branch of the renormalisation, decided on the device's own product; default: on the 50-digit product"""
    R = mat3(A[0], B[0])
    t = [x + y for x, y in zip(matvec(A[0], B[1]), A[1])]
    return normalize_rotation(R, b), t


def iso_mul(A, B):
    return mat3(A[0], B[0]), [x + y for x, y in zip(matvec(A[0], B[1]), A[1])]


def inv(A):
    Rt = [A[0][3 * j + i] for i in range(3) for j in range(3)]
    return Rt, [-x for x in matvec(Rt, A[1])]


def se3_exp(u, small=None):
    u = list(u)
    small = branch_exp(u) if small is None else small
    th = mp.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    Om = skew(u)
    Om2 = mat3(Om, Om)
    if small:
        R = V = eye_plus((1, Om), (1, Om2))
    else:
        a, b, c = mp.sin(th) / th, (1 - mp.cos(th)) / (th * th), (th - mp.sin(th)) / (th * th * th)
        R, V = eye_plus((a, Om), (b, Om2)), eye_plus((b, Om), (c, Om2))
    return normalize_rotation(R), matvec(V, u[3:6])


def se3_log(T, small=None):
    R, t = T
    small = branch_log(R) if small is None else small
    d = F(0.5) * (R[0] + R[4] + R[8] - 1)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    if small:
        om = [F(0.5) * x for x in dR]
        c = F(1) / 12
    else:
        th = mp.acos(d)
        k = th / (2 * mp.sqrt(1 - d * d))
        om = [k * x for x in dR]
        c = (1 - th / (2 * mp.tan(th / 2))) / (th * th)
    Om = skew(om)
    Vi = eye_plus((F(-0.5), Om), (c, mat3(Om, Om)))
    return om + matvec(Vi, t)


def se3_adj(T):
    R, t = T
    sR = mat3(skew(t), R)
    A = [F(0)] * 36
    for i in range(3):
        for j in range(3):
            A[6 * i + j] = R[3 * i + j]
            A[6 * (i + 3) + j + 3] = R[3 * i + j]
            A[6 * (i + 3) + j] = sR[3 * i + j]
    return A


def to_mqt(T):
    q = quat_of(T[0])
    return list(T[1]) + q[1:]


def from_mqt(v, outside=None):
    outside = branch_from_mqt(v) if outside is None else outside
    if outside:
        return eye_plus(), list(v[:3])
    w = 1 - (v[3] * v[3] + v[4] * v[4] + v[5] * v[5])
    return mat_of_quat([mp.sqrt(w), v[3], v[4], v[5]]), list(v[:3])


def mqt_jac_right(E):
    q = quat_of(E[0])
    J = [F(0)] * 36
    for r in range(3):
        for c in range(3):
            J[6 * r + c] = E[0][3 * r + c]
    J[21], J[22], J[23] = q[0], -q[3], q[2]
    J[27], J[28], J[29] = q[3], q[0], -q[1]
    J[33], J[34], J[35] = -q[2], q[1], q[0]
    return J


def wprod(A, B):
    qa, qb = quat_of(A[0]), quat_of(B[0])
    return qa[0] * qb[0] - qa[1] * qb[1] - qa[2] * qb[2] - qa[3] * qb[3]


def mqt_jac_left_inv(A, B, negative=None):
    qa, qb = quat_of(A[0]), quat_of(B[0])
    negative = (wprod(A, B) < 0) if negative is None else negative
    sgn = -1 if negative else 1
    J = [F(0)] * 36
    sk = skew(B[1])
    RS = mat3(A[0], sk)
    for r in range(3):
        for c in range(3):
            J[6 * r + c] = -A[0][3 * r + c]
            J[6 * r + 3 + c] = 2 * RS[3 * r + c]
    for c in range(3):
        u = [1 if c == k else 0 for k in range(3)]
        m0 = -qa[1] * u[0] - qa[2] * u[1] - qa[3] * u[2]
        m1 = qa[0] * u[0] + qa[2] * u[2] - qa[3] * u[1]
        m2 = qa[0] * u[1] - qa[1] * u[2] + qa[3] * u[0]
        m3 = qa[0] * u[2] + qa[1] * u[1] - qa[2] * u[0]
        J[6 * 3 + 3 + c] = -sgn * (m0 * qb[1] + m1 * qb[0] + m2 * qb[3] - m3 * qb[2])
        J[6 * 4 + 3 + c] = -sgn * (m0 * qb[2] - m1 * qb[3] + m2 * qb[0] + m3 * qb[1])
        J[6 * 5 + 3 + c] = -sgn * (m0 * qb[3] + m1 * qb[2] - m2 * qb[1] + m3 * qb[0])
    return J


# ---- the exact maps ------------------------------------------------------------------------------------------------------------
def exp_exact(u):
    """the exponential of se(3) in the order (omega, upsilon): Rodrigues' formula and V, by their series below 1e-10 rad"""
    u = list(u)
    th = mp.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    Om = skew(u)
    Om2 = mat3(Om, Om)
    if th < F(10) ** -10:
        a, b, c = 1 - th * th / 6, F(0.5) - th * th / 24, F(1) / 6 - th * th / 120
    else:
        a, b, c = mp.sin(th) / th, (1 - mp.cos(th)) / (th * th), (th - mp.sin(th)) / (th * th * th)
    return eye_plus((a, Om), (b, Om2)), matvec(eye_plus((b, Om), (c, Om2)), u[3:6])


def log_exact(T):
    """the logarithm of a rigid motion whose rotation is orthonormal to working precision and turns by less than pi: the angle
    from atan2(|(R - R')^v| / 2, (tr R - 1) / 2), which is well conditioned everywhere"""
    R, t = T
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    s = mp.sqrt(sum(x * x for x in dR)) / 2
    th = mp.atan2(s, (R[0] + R[4] + R[8] - 1) / 2)
    if th < F(10) ** -10:
        k, c = F(0.5) + th * th / 12, F(1) / 12 + th * th / 720
    else:
        k, c = th / (2 * s), (1 - th / (2 * mp.tan(th / 2))) / (th * th)
    om = [k * x for x in dR]
    Om = skew(om)
    return om + matvec(eye_plus((F(-0.5), Om), (c, mat3(Om, Om))), t)


def jac_fd(f, h=F(10) ** -20):
    """6x6 row-major: d f(d) / d d at 0 by central differences in 50 digits (truncation h^2 = 1e-40, round-off 1e-50 / h = 1e-30)"""
    J = [F(0)] * 36
    for c in range(6):
        d = [F(0)] * 6
        d[c] = h
        fp = f(d)
        d[c] = -h
        fm = f(d)
        for r in range(6):
            J[6 * r + c] = (fp[r] - fm[r]) / (2 * h)
    return J


def jac_right_fd(E):
    return jac_fd(lambda d: to_mqt(iso_mul(E, from_mqt(d, outside=False))))


def jac_left_inv_fd(A, B):
    return jac_fd(lambda d: to_mqt(iso_mul(iso_mul(A, inv(from_mqt(d, outside=False))), B)))
