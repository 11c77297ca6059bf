"""numpy restatement of Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (reference src/Optimizer.cc:416-968, :983-1623,
Marginalize :1644-1725, over g2o's Gauss-Newton and LinearSolverDense), the contract of DESIGN.md 6p: the visual edges as array
operations in the order the contract writes them and summed in the fixed order of 6i's departure (a); the serial section (EdgeInertial,
the two random-walk edges, the prior edge, assembly in vertex-id order, pivoted LDLT at lambda 0, the updates, the final Hessian, the
marginalisation and the eigenvalue clipping) on small float64 arrays whose products add left to right.  Every departure from the
reference's own build (DESIGN.md 6p lists them) is switched in here, operation by operation.  Shared by test_pose_inertial_ref.py
(CPU) and test_gpu_pose_inertial.py; holds the case generators."""
import numpy as np

from pose_opt_ref import (F32, F64, LANES, DELTA_MONO, DELTA_STEREO, DSQR_MONO, DSQR_STEREO, sincos, tree_sum, finite, quat_from_rotvec,
                          quat_to_mat)

MODE_LAST_KEYFRAME, MODE_LAST_FRAME = 0, 1
CAM_FLOATS, STATE_FLOATS, PREINT_FLOATS, COV_RW_FLOATS, PRIOR_DOUBLES = 36, 21, 148, 18, 246
FLAG_SOLVE_FAILED, FLAG_NONFINITE, FLAG_FEW_EDGES, FLAG_RECOVERY, FLAG_INFO_CLIPPED, FLAG_MARG_CUT, FLAG_PRIOR_CLIPPED, FLAG_PRIOR_HUBER = \
    1, 2, 4, 8, 16, 32, 64, 128
FLAG_MODE = 256                                 # the _dev form ran a LastFrame problem without a prior, or an unknown mode, as LastKeyFrame
CHI2_MONO_KF = [F32(12), F32(7.5), F32(5.991), F32(5.991)]
CHI2_MONO_F = [F32(5.991)] * 4
CHI2_STEREO = [F32(15.6), F32(9.8), F32(7.815), F32(7.815)]
CHI2_MONO_OUT, CHI2_STEREO_OUT = F32(18.0), F32(24.0)
GRAVITY = F64(F32(9.81))
SWEEPS = {3: 6, 9: 10, 15: 12}                   # the fixed schedule of the cyclic Jacobi eigen-solver, by order
ROUNDS, ITS = 4, 10

# fdlibm's acos without fma, as lm_device.h states it
PIO2_HI, PIO2_LO, PI = F64(1.57079632679489655800e+00), F64(6.12323399573676603587e-17), F64(3.14159265358979311600e+00)
_PS = [F64(v) for v in (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
                        7.91534994289814532176e-04, 3.47933107596021167570e-05)]
_QS = [F64(v) for v in (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)]


def _acos_r(z):
    p = z * (_PS[0] + z * (_PS[1] + z * (_PS[2] + z * (_PS[3] + z * (_PS[4] + z * _PS[5])))))
    q = 1.0 + z * (_QS[0] + z * (_QS[1] + z * (_QS[2] + z * _QS[3])))
    return p / q


def acos(x):
    x = F64(x)
    if not (np.abs(x) <= 1.0):
        return F64(np.nan)
    if x == 1.0:
        return F64(0.0)
    if x == -1.0:
        return PI + 2.0 * PIO2_LO
    if np.abs(x) < 0.5:
        if np.abs(x) < 6.938893903907228e-18:
            return PIO2_HI + PIO2_LO
        r = _acos_r(x * x)
        return PIO2_HI - (x - (PIO2_LO - x * r))
    if x < 0:
        z = (1.0 + x) * 0.5
        s = np.sqrt(z)
        w = _acos_r(z) * s - PIO2_LO
        return PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = np.sqrt(z)
    df = np.array([s]).view(np.uint64)
    df = (df & np.uint64(0xFFFFFFFF00000000)).view(F64)[0]
    c = (z - df * df) / (s + df)
    w = _acos_r(z) * s + c
    return 2.0 * (df + w)


# ---------------------------------------------------------------- small dense algebra: every sum left to right from its first product
def mm(A, B):
    A, B = np.asarray(A), np.asarray(B)
    C = A[:, 0:1] * B[0:1, :]
    for k in range(1, A.shape[1]):
        C = C + A[:, k:k + 1] * B[k:k + 1, :]
    return C


def mv(A, x):
    return mm(A, np.asarray(x).reshape(-1, 1))[:, 0]


def hat(w):
    z = w.dtype.type(0.0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], w.dtype)


def jacobi_eig(M, n):
    """cyclic Jacobi on the symmetric matrix whose LOWER triangle is M's: SWEEPS[n] sweeps over (p, q), p < q, row by row; a pair whose
    entry is exactly 0 is skipped.  Returns (eigenvalues = the final diagonal, in place order; V with the eigenvectors as columns)."""
    with np.errstate(all="ignore"):               # theta * theta overflows to inf once an entry has all but vanished: t = 0, no rotation
        return _jacobi_eig(M, n)


def _jacobi_eig(M, n):
    A = np.array(M, F64)
    for i in range(n):
        for j in range(i + 1, n):
            A[i, j] = A[j, i]
    V = np.eye(n, dtype=F64)
    for _ in range(SWEEPS[n]):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                if theta < 0:
                    t = -t
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * cp - s * cq
                A[:, q] = s * cp + c * cq
                rp, rq = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c * rp - s * rq
                A[q, :] = s * rp + c * rq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - s * vq
                V[:, q] = s * vp + c * vq
    return np.diag(A).copy(), V


def recompose(V, d):
    """(V diag(d)) V^T"""
    return mm(V * d[None, :], V.T)


def nearest_rotation(R):
    """the stated step in place of NormalizeRotation's SVD: R (R^T R)^(-1/2), the inverse root through jacobi_eig"""
    R = np.asarray(R, F64)
    lam, Q = jacobi_eig(mm(R.T, R), 3)
    return mm(R, recompose(Q, 1.0 / np.sqrt(lam)))


def inv3(A):
    """cofactor inverse"""
    a = np.asarray(A, F64)
    c = np.empty((3, 3), F64)
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            c[i, j] = a[i1, j1] * a[i2, j2] - a[i1, j2] * a[i2, j1]
    det = (a[0, 0] * c[0, 0] + a[0, 1] * c[0, 1]) + a[0, 2] * c[0, 2]
    return c.T / det


def ldlt_inverse(M, n):
    """inverse through an unpivoted LDLT of the symmetric matrix whose lower triangle is M's, column by column"""
    A = np.asarray(M, F64)
    L = np.zeros((n, n), F64)
    d = np.zeros(n, F64)
    v = np.zeros(n, F64)
    for j in range(n):
        acc = A[j, j]
        for k in range(j):
            v[k] = L[j, k] * d[k]
            acc = acc - L[j, k] * v[k]
        d[j] = acc
        for i in range(j + 1, n):
            acc = A[i, j]
            for k in range(j):
                acc = acc - L[i, k] * v[k]
            L[i, j] = acc / d[j]
    X = np.zeros((n, n), F64)
    y = np.zeros(n, F64)
    for c in range(n):
        for i in range(n):
            acc = F64(1.0 if i == c else 0.0)
            for k in range(i):
                acc = acc - L[i, k] * y[k]
            y[i] = acc
        for i in range(n):
            y[i] = y[i] / d[i]
        for i in range(n - 1, -1, -1):
            acc = y[i]
            for k in range(i + 1, n):
                acc = acc - L[k, i] * y[k]
            y[i] = acc
        X[:, c] = y
    return X


def ldlt_solve(H, b, D):
    """6i's departure (c) at order D and lambda 0: LDLT with diagonal pivoting (the largest |diagonal| of the trailing block, the first
    maximum); a negative pivot: (False, None); a zero pivot leaves its column of L and its y zero"""
    A = np.array(H, F64)
    perm = list(range(D))
    d = np.zeros(D, F64)
    for k in range(D):
        p, best = k, np.abs(A[k, k])
        for j in range(k + 1, D):
            if np.abs(A[j, j]) > best:
                p, best = j, np.abs(A[j, j])
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
            perm[k], perm[p] = perm[p], perm[k]
        d[k] = A[k, k]
        if d[k] < 0.0:
            return False, None
        A[k + 1:, k] = A[k + 1:, k] / d[k] if d[k] != 0.0 else 0.0
        new = A[k + 1:, k + 1:] - A[k + 1:, k:k + 1] * A[k:k + 1, k + 1:]
        low = np.tril(new)
        A[k + 1:, k + 1:] = low + np.tril(new, -1).T
    y = np.array([b[perm[i]] for i in range(D)], F64)
    for i in range(D):
        for j in range(i):
            y[i] = y[i] - A[i, j] * y[j]
    for i in range(D):
        y[i] = y[i] / d[i] if d[i] != 0.0 else F64(0.0)
    for i in range(D - 1, -1, -1):
        for j in range(i + 1, D):
            y[i] = y[i] - A[j, i] * y[j]
    x = np.zeros(D, F64)
    for i in range(D):
        x[perm[i]] = y[i]
    return True, x


# ---------------------------------------------------------------- SO3 (G2oTypes.cc:908-985)
def _norm3(w):
    d2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    return d2, np.sqrt(d2)


EYE3 = np.eye(3, dtype=F64)
PATHS = None                                          # a set here receives the names of the branches taken


def _path(name):
    if PATHS is not None:
        PATHS.add(name)


def exp_so3(w):
    d2, d = _norm3(w)
    W = hat(w)
    if d < 1e-5:
        _path("exp_small")
        res = (EYE3 + W) + mm(0.5 * W, W)
    else:
        _path("exp_large")
        s, c = sincos(d)
        res = (EYE3 + (W * s) / d) + (mm(W, W) * (1.0 - c)) / d2
    return nearest_rotation(res)


def log_so3(R):
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    w = np.array([(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2], F64)
    costheta = (tr - 1.0) * 0.5
    if costheta > 1 or costheta < -1:
        _path("log_outside")
        return w
    theta = acos(costheta)
    s, _ = sincos(theta)
    if np.abs(s) < 1e-5:
        _path("log_small")
        return w
    _path("log_large")
    return (theta * w) / s


def inv_right_jacobian(v):
    d2, d = _norm3(v)
    if d < 1e-5:
        _path("invjr_small")
        return EYE3.copy()
    _path("invjr_large")
    W = hat(v)
    s, c = sincos(d)
    return (EYE3 + W / 2) + mm(W, W) * (1.0 / d2 - (1.0 + c) / ((2.0 * d) * s))


def right_jacobian(v):
    d2, d = _norm3(v)
    if d < 1e-5:
        return EYE3.copy()
    W = hat(v)
    s, c = sincos(d)
    return (EYE3 - (W * (1.0 - c)) / d2) + (mm(W, W) * (d - s)) / (d2 * d)


# ---------------------------------------------------------------- the preintegration (ImuTypes.cc:377-427), float
def unpack_preint(p):
    p = np.asarray(p, F32)
    o = {"dT": p[0], "dR": p[1:10].reshape(3, 3), "dV": p[10:13], "dP": p[13:16], "JRg": p[16:25].reshape(3, 3), "JVg": p[25:34].reshape(3, 3),
         "JVa": p[34:43].reshape(3, 3), "JPg": p[43:52].reshape(3, 3), "JPa": p[52:61].reshape(3, 3), "ba": p[61:64], "bg": p[64:67],
         "C": p[67:148].reshape(9, 9)}
    return o


def so3f_exp_matrix(om):
    """Sophus::SO3f::exp(om).matrix(): the quaternion of so3.hpp's expAndTheta with its small-angle branch, Eigen's toRotationMatrix; float.
    sin and cos of the half angle are the float casts of 6i's sincos of its double cast"""
    om = np.asarray(om, F32)
    theta_sq = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    if theta_sq < F32(1e-5) * F32(1e-5):
        _path("so3f_small")
        po4 = theta_sq * theta_sq
        imag = (F32(0.5) - F32(1.0 / 48.0) * theta_sq) + F32(1.0 / 3840.0) * po4
        real = (F32(1) - F32(1.0 / 8.0) * theta_sq) + F32(1.0 / 384.0) * po4
    else:
        _path("so3f_large")
        theta = np.sqrt(theta_sq)
        half = F32(0.5) * theta
        s, c = sincos(F64(half))
        imag = F32(s) / theta
        real = F32(c)
    qw, qx, qy, qz = real, imag * om[0], imag * om[1], imag * om[2]
    two = F32(2)
    tx, ty, tz = two * qx, two * qy, two * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    one = F32(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], F32)


def delta_bias(pre, bg, ba):
    """GetDeltaBias against IMU::Bias(float casts of the double estimates): (dbg, dba) float"""
    return np.asarray(bg, F64).astype(F32) - pre["bg"], np.asarray(ba, F64).astype(F32) - pre["ba"]


def delta_rotation(pre, dbg):
    R = mm(pre["dR"], so3f_exp_matrix(mv(pre["JRg"], dbg)))          # float
    return nearest_rotation(R.astype(F64)).astype(F32).astype(F64)    # the stated step, in double on the float product, cast to float


def delta_velocity(pre, dbg, dba):
    return ((pre["dV"] + mv(pre["JVg"], dbg)) + mv(pre["JVa"], dba)).astype(F64)


def delta_position(pre, dbg, dba):
    return ((pre["dP"] + mv(pre["JPg"], dbg)) + mv(pre["JPa"], dba)).astype(F64)


# ---------------------------------------------------------------- edges of the serial section
def inertial_edge(pre, prev, cur, linearise=True):
    """EdgeInertial::computeError and linearizeOplus: e [9] and J [9, 24] over VPk 6, VVk 3, VGk 3, VAk 3, VP 6, VV 3"""
    dt = F64(pre["dT"])
    g = np.array([0.0, 0.0, -GRAVITY], F64)
    dbg, dba = delta_bias(pre, prev["bg"], prev["ba"])
    dR = delta_rotation(pre, dbg)
    dV, dP = delta_velocity(pre, dbg, dba), delta_position(pre, dbg, dba)
    Rwb1, Rwb2 = prev["Rwb"], cur["Rwb"]
    Rbw1 = Rwb1.T
    eR = mm(mm(dR.T, Rbw1), Rwb2)
    er = log_so3(eR)
    dv = (cur["v"] - prev["v"]) - g * dt
    ev = mv(Rbw1, dv) - dV
    dp = ((cur["twb"] - prev["twb"]) - prev["v"] * dt) - ((g * dt) * dt) / 2
    ep = mv(Rbw1, dp) - dP
    e = np.concatenate([er, ev, ep])
    if not linearise:
        return e, None
    invJr = inv_right_jacobian(er)
    J = np.zeros((9, 24), F64)
    J[0:3, 0:3] = mm(mm(-invJr, Rwb2.T), Rwb1)
    J[3:6, 0:3] = hat(mv(Rbw1, dv))
    dp2 = ((cur["twb"] - prev["twb"]) - prev["v"] * dt) - ((0.5 * g) * dt) * dt
    J[6:9, 0:3] = hat(mv(Rbw1, dp2))
    J[6:9, 3:6] = -EYE3
    J[3:6, 6:9] = -Rbw1
    J[6:9, 6:9] = -Rbw1 * dt
    JRg = pre["JRg"].astype(F64)
    J[0:3, 9:12] = mm(mm(mm(-invJr, eR.T), right_jacobian(mv(JRg, dbg.astype(F64)))), JRg)
    J[3:6, 9:12] = -pre["JVg"].astype(F64)
    J[6:9, 9:12] = -pre["JPg"].astype(F64)
    J[3:6, 12:15] = -pre["JVa"].astype(F64)
    J[6:9, 12:15] = -pre["JPa"].astype(F64)
    J[0:3, 15:18] = invJr
    J[6:9, 18:21] = mm(Rbw1, Rwb2)
    J[3:6, 21:24] = Rbw1
    return e, J


def prior_edge(pri, prev, linearise=True):
    """EdgePriorPoseImu: e [15], J [15, 15] over VPk 6, VVk 3, VGk 3, VAk 3"""
    RtR = mm(pri["Rwb"].T, prev["Rwb"])
    er = log_so3(RtR)
    et = mv(pri["Rwb"].T, prev["twb"] - pri["twb"])
    e = np.concatenate([er, et, prev["v"] - pri["v"], prev["bg"] - pri["bg"], prev["ba"] - pri["ba"]])
    if not linearise:
        return e, None
    J = np.zeros((15, 15), F64)
    J[0:3, 0:3] = inv_right_jacobian(er)
    J[3:6, 3:6] = RtR
    J[6:15, 6:15] = np.eye(9, dtype=F64)
    return e, J


def quad_form(J, Om, e, w):
    """one edge's H = J^T (w Om) J, g = J^T (w (Om e)) (b = -g)"""
    Oe = mv(Om, e)
    JtO = mm(J.T, w * Om)
    return mm(JtO, J), mv(J.T, w * Oe)


def chi2_of(Om, e):
    Oe = mv(Om, e)
    acc = e[0] * Oe[0]
    for r in range(1, len(e)):
        acc = acc + e[r] * Oe[r]
    return acc


def huber(chi2, delta):
    """RobustKernelHuber::robustify -> (rho0, rho1)"""
    dsqr = delta * delta
    if chi2 <= dsqr:
        return chi2, F64(1.0)
    sq = np.sqrt(chi2)
    return 2 * sq * delta - dsqr, delta / sq


# ---------------------------------------------------------------- the visual edges, all features at once
def features(P, kpts, octave, uright, xw, has_mp, track_depth, n):
    n = int(n)
    octv = np.zeros(n, np.int64) if octave is None else np.asarray(octave[:n], np.int64).copy()
    octv[(octv < 0) | (octv >= P["nlevels"])] = 0
    ur = np.full(n, -1.0, F32) if uright is None else np.asarray(uright[:n], F32)
    return {"u": np.asarray(kpts, F32).reshape(-1, 2)[:n, 0].astype(F64), "v": np.asarray(kpts, F32).reshape(-1, 2)[:n, 1].astype(F64), "ur": ur.astype(F64),
            "stereo": ~(ur < 0), "X": np.asarray(xw, F32).reshape(-1, 3)[:n].astype(F64),
            "invsigma2": np.asarray(P["inv_level_sigma2"], F32)[octv].astype(F64), "edge": np.asarray(has_mp[:n]) != 0,
            "close": np.asarray(track_depth[:n], F32) < F32(10.0)}


def visual_terms(P, cam, cur, f, robust, linearise=True):
    """every feature's chi2, rho0 and its 21 + 6 contributions at the estimate (EdgeMonoOnlyPose / EdgeStereoOnlyPose over ImuCamPose):
    terms [n, 28] = H's upper triangle row by row, the 6 sums whose negative is b, rho0"""
    fx, fy, cx, cy, bf = (F64(P[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    n = len(f["u"])
    Rcw, tcw = cur["Rcw"], cur["tcw"]
    X = f["X"]
    Xc = [((Rcw[r, 0] * X[:, 0] + Rcw[r, 1] * X[:, 1]) + Rcw[r, 2] * X[:, 2]) + tcw[r] for r in range(3)]
    x, y, z = Xc
    st, isg = f["stereo"], f["invsigma2"]
    pu = fx * x / z + cx
    pv = fy * y / z + cy
    pr = pu - bf * (1.0 / z)
    e = [f["u"] - pu, f["v"] - pv, np.where(st, f["ur"] - pr, 0.0)]
    chi2 = e[0] * (isg * e[0]) + e[1] * (isg * e[1])
    chi2 = np.where(st, chi2 + e[2] * (isg * e[2]), chi2)
    delta, dsqr = np.where(st, DELTA_STEREO, DELTA_MONO), np.where(st, DSQR_STEREO, DSQR_MONO)
    sq = np.sqrt(chi2)
    inl = chi2 <= dsqr
    rho0 = np.where(inl, chi2, 2 * sq * delta - dsqr)
    rho1 = np.where(inl, 1.0, delta / sq)
    if not robust:
        rho0, rho1 = chi2, np.ones(n, F64)
    if not linearise:
        return chi2, None
    Rbc, tbc, Rcb = cam["Rbc"], cam["tbc"], cam["Rcb"]
    Xb = [((Rbc[r, 0] * x + Rbc[r, 1] * y) + Rbc[r, 2] * z) + tbc[r] for r in range(3)]
    zero, one = np.zeros(n, F64), np.ones(n, F64)
    zz = z * z
    pj = [[fx / z, zero, -fx * x / zz], [zero, fy / z, -fy * y / zz]]
    pj.append([pj[0][0], pj[0][1], pj[0][2] + bf * (1.0 / zz)])
    PR = [[(pj[r][0] * Rcb[0, c] + pj[r][1] * Rcb[1, c]) + pj[r][2] * Rcb[2, c] for c in range(3)] for r in range(3)]
    xb, yb, zb = Xb
    S = [[zero, zb, -yb, one, zero, zero], [-zb, zero, xb, zero, one, zero], [yb, -xb, zero, zero, zero, one]]
    A = [[(PR[r][0] * S[0][c] + PR[r][1] * S[1][c]) + PR[r][2] * S[2][c] for c in range(6)] for r in range(3)]
    w = rho1 * isg
    terms = np.zeros((n, 28), F64)
    col = 0
    for j in range(6):
        for k in range(j, 6):
            h = (A[0][j] * w) * A[0][k] + (A[1][j] * w) * A[1][k]
            terms[:, col] = np.where(st, h + (A[2][j] * w) * A[2][k], h)
            col += 1
    for j in range(6):
        g = ((rho1 * A[0][j]) * isg) * e[0] + ((rho1 * A[1][j]) * isg) * e[1]
        terms[:, col] = np.where(st, g + ((rho1 * A[2][j]) * isg) * e[2], g)
        col += 1
    terms[:, 27] = rho0
    return chi2, terms


def depth_positive(cur, f):
    Rcw, X = cur["Rcw"], f["X"]
    return (((Rcw[2, 0] * X[:, 0] + Rcw[2, 1] * X[:, 1]) + Rcw[2, 2] * X[:, 2]) + cur["tcw"][2]) > 0.0


def classify(P, cam, cur, f, lf, rnd, outl, chi2_in):
    """the float classification behind round rnd (Optimizer.cc:729-810, :1313-1392) at the estimate cur: an edge flagged in outl recomputes
    its error, any other is compared at chi2_in (float32 [n]).  Returns (the new flags, the float chi2 compared), for every row"""
    c2, _ = visual_terms(P, cam, cur, f, False, linearise=False)
    c2f = np.where(outl, c2.astype(F32), np.asarray(chi2_in, F32))
    tm = (CHI2_MONO_F if lf else CHI2_MONO_KF)[rnd]
    close_thr = F32(F64(1.5) * F64(tm))
    dpos = depth_positive(cur, f)
    out_m = ((c2f > tm) & ~f["close"]) | (f["close"] & (c2f > close_thr)) | ~dpos
    out_s = c2f > CHI2_STEREO[rnd]
    return np.where(f["stereo"], out_s, out_m), c2f


def recovered(P, cam, cur, f):
    """the recovery pass's test (:836-857, :1417-1437): every error recomputed, below 18 / 24.  Returns (good, the float chi2)"""
    c2, _ = visual_terms(P, cam, cur, f, False, linearise=False)
    c2f = c2.astype(F32)
    return c2f < np.where(f["stereo"], CHI2_STEREO_OUT, CHI2_MONO_OUT), c2f


# ---------------------------------------------------------------- states
def unpack_state(s, dtype=F32):
    s = np.asarray(s, dtype).astype(F64)
    return {"Rwb": s[0:9].reshape(3, 3).copy(), "twb": s[9:12].copy(), "v": s[12:15].copy(), "bg": s[15:18].copy(), "ba": s[18:21].copy()}


def pack_state(st):
    return np.concatenate([st["Rwb"].reshape(-1), st["twb"], st["v"], st["bg"], st["ba"]]).astype(F64)


def unpack_cam(c):
    c = np.asarray(c, F32).astype(F64)
    Rcb = c[12:21].reshape(3, 3).copy()
    return {"Rcw": c[0:9].reshape(3, 3).copy(), "tcw": c[9:12].copy(), "Rcb": Rcb, "tcb": c[21:24].copy(), "Rbc": Rcb.T.copy(), "tbc": c[33:36].copy()}


def pose_update(st, cam, u):
    """ImuCamPose::Update: the NormalizeRotation(Rwb) of G2oTypes.cc:236 discards its result, so nothing is re-normalised"""
    st["twb"] = st["twb"] + mv(st["Rwb"], u[3:6])
    st["Rwb"] = mm(st["Rwb"], exp_so3(u[0:3]))
    if cam is not None:
        Rbw = st["Rwb"].T
        tbw = mv(-Rbw, st["twb"])
        st["Rcw"] = mm(cam["Rcb"], Rbw)
        st["tcw"] = mv(cam["Rcb"], tbw) + cam["tcb"]


def clip_information(H, n, floor=1e-12):
    """(H + H^T) / 2 then eigenvalues below `floor` set to 0 and recomposed; returns (H, clipped count)"""
    Hs = (H + H.T) / 2
    lam, V = jacobi_eig(Hs, n)
    cl = lam < floor
    return recompose(V, np.where(cl, 0.0, lam)), int(cl.sum())


# ---------------------------------------------------------------- the optimisation
def params(fx, fy, cx, cy, bf, inv_level_sigma2=(1.0,)):
    return {"fx": F32(fx), "fy": F32(fy), "cx": F32(cx), "cy": F32(cy), "bf": F32(bf), "nlevels": len(inv_level_sigma2),
            "inv_level_sigma2": np.asarray(inv_level_sigma2, F32)}


def pose_inertial_optimization(P, mode, rec_init, cam, state, prev_state, preint, cov_rw, prior_in, kpts, octave, uright, xw, has_mp, track_depth,
                               n=None, outlier=None, chi2=None):
    with np.errstate(all="ignore"):
        return _pio(P, int(mode), bool(rec_init), cam, state, prev_state, preint, cov_rw, prior_in, kpts, octave, uright, xw, has_mp, track_depth, n,
                    outlier, chi2)


def _pio(P, mode, rec_init, cam_in, state, prev_state, preint, cov_rw, prior_in, kpts, octave, uright, xw, has_mp, track_depth, n, outlier, chi2):
    N = len(np.asarray(has_mp).reshape(-1))
    n = N if n is None else min(max(int(n), 0), N)
    out_outlier = np.zeros(N, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    out_chi2 = np.zeros(N, F32) if chi2 is None else np.array(chi2, F32)
    trace, stats = np.zeros((4, 8), F64), np.zeros(16, np.int32)
    chi2_rounds = np.full((5, N), np.nan, F32)     # what each round's classification and the recovery pass compared (not an output of the call)
    f = features(P, kpts, octave, uright, xw, has_mp, track_depth, n)
    edge, st = f["edge"], f["stereo"]
    out_outlier[:n][edge] = 0
    n_init = int(edge.sum())
    n_stereo = int((edge & st).sum())
    lf = mode == MODE_LAST_FRAME and prior_in is not None
    D = 30 if lf else 15
    flags = 0 if (mode == MODE_LAST_KEYFRAME or lf) else FLAG_MODE
    cam = unpack_cam(cam_in)
    cur, prev = unpack_state(state), unpack_state(prev_state)
    cur["Rcw"], cur["tcw"] = cam["Rcw"], cam["tcw"]          # until the first update the camera pose is GetPose()'s, not Rwb's
    pre = unpack_preint(preint)
    # EdgeInertial's information: the inverse of C's 9 x 9 block, symmetrised, clipped
    info9, ncl = clip_information(ldlt_inverse(pre["C"].astype(F64), 9), 9)
    if ncl:
        flags |= FLAG_INFO_CLIPPED
    cov = np.asarray(cov_rw, F32).astype(F64)
    infoG, infoA = inv3(cov[0:9].reshape(3, 3)), inv3(cov[9:18].reshape(3, 3))
    pri = None
    if lf:
        pd = np.asarray(prior_in, F64)
        pri = unpack_state(pd[:21], F64)
        pri["H"] = pd[21:246].reshape(15, 15).copy()
    n_edges = n_init + (4 if lf else 3)
    outl = np.zeros(n, bool)
    last_chi2 = np.zeros(n, F64)
    x = np.zeros(30, F64)
    n_bad = n_inl = 0
    tot_its = fails = rounds = 0
    thr_mono = CHI2_MONO_F if lf else CHI2_MONO_KF
    # inertial column -> solver index (vertex-id order VP VV VG VA VPk VVk VGk VAk)
    imap = [c + 15 if c < 15 else c - 15 for c in range(24)]
    for rnd in range(ROUNDS):
        active = edge & ~outl
        robust = rnd < 3                                   # setRobustKernel(0) runs behind round 2's classification
        ok = True
        for it in range(ITS):
            tot_its += 1
            c2, terms = visual_terms(P, cam, cur, f, robust)
            last_chi2[active] = c2[active]
            S = tree_sum(terms, active)
            H = np.zeros((30, 30), F64)
            b = np.zeros(30, F64)
            col = 0
            for j in range(6):
                for k in range(j, 6):
                    H[j, k] = H[k, j] = S[col]
                    col += 1
            for j in range(6):
                b[j] = -S[21 + j]
            total = S[27]
            e, J = inertial_edge(pre, prev, cur)
            Hi, gi = quad_form(J, info9, e, F64(1.0))
            total = total + chi2_of(info9, e)
            for a in range(24):
                b[imap[a]] = b[imap[a]] - gi[a]
                for c in range(24):
                    H[imap[a], imap[c]] = H[imap[a], imap[c]] + Hi[a, c]
            for (Om, kc, kp, off, offk) in ((infoG, "bg", "bg", 9, 24), (infoA, "ba", "ba", 12, 27)):
                erw = cur[kc] - prev[kp]
                Oe = mv(Om, erw)
                total = total + chi2_of(Om, erw)
                for a in range(3):
                    b[off + a] = b[off + a] - Oe[a]
                    b[offk + a] = b[offk + a] + Oe[a]
                    for c in range(3):
                        H[off + a, off + c] = H[off + a, off + c] + Om[a, c]
                        H[offk + a, offk + c] = H[offk + a, offk + c] + Om[a, c]
                        H[off + a, offk + c] = H[off + a, offk + c] - Om[a, c]
                        H[offk + a, off + c] = H[offk + a, off + c] - Om[a, c]
            if lf:
                ep, Jp = prior_edge(pri, prev)
                rho0, rho1 = huber(chi2_of(pri["H"], ep), F64(5.0))
                if rho1 != 1.0:
                    flags |= FLAG_PRIOR_HUBER
                Hp, gp = quad_form(Jp, pri["H"], ep, rho1)
                total = total + rho0
                for a in range(15):
                    b[15 + a] = b[15 + a] - gp[a]
                    for c in range(15):
                        H[15 + a, 15 + c] = H[15 + a, 15 + c] + Hp[a, c]
            if it == 0:
                trace[rnd, 1] = total
            trace[rnd, 0], trace[rnd, 2] = it + 1, total
            ok, sol = ldlt_solve(H[:D, :D], b[:D], D)
            if ok:
                x[:D] = sol
            else:
                flags |= FLAG_SOLVE_FAILED
                fails += 1
            pose_update(cur, cam, x[0:6])
            cur["v"], cur["bg"], cur["ba"] = cur["v"] + x[6:9], cur["bg"] + x[9:12], cur["ba"] + x[12:15]
            if lf:
                pose_update(prev, None, x[15:21])
                prev["v"], prev["bg"], prev["ba"] = prev["v"] + x[21:24], prev["bg"] + x[24:27], prev["ba"] + x[27:30]
            if not ok:
                break
        trace[rnd, 3] = 1.0 if ok else 0.0
        # classification: an edge flagged outlier recomputes its error at the new estimate, the others keep the one the last iteration saw
        out, c2f = classify(P, cam, cur, f, lf, rnd, outl, last_chi2.astype(F32))
        last_chi2[edge & outl] = visual_terms(P, cam, cur, f, False, linearise=False)[0][edge & outl]
        outl = edge & out
        n_bad = int(outl.sum())
        n_inl = n_init - n_bad
        out_outlier[:n][edge] = outl[edge]
        out_chi2[:n][edge] = c2f[edge]
        chi2_rounds[rnd, :n][edge] = c2f[edge]
        trace[rnd, 4] = n_inl
        rounds += 1
        if n_edges < 10:
            flags |= FLAG_FEW_EDGES
            break
    flag_out = outl.copy()
    if n_inl < 30 and not rec_init:
        flags |= FLAG_RECOVERY
        good, c2f = recovered(P, cam, cur, f)
        flag_out = edge & outl & ~good
        n_bad = int((edge & ~good).sum())
        out_outlier[:n][edge] = flag_out[edge]
        out_chi2[:n][edge] = c2f[edge]
        chi2_rounds[4, :n][edge] = c2f[edge]
    # the final Hessian at the final estimate: inliers only, no robust weight
    _, terms = visual_terms(P, cam, cur, f, False)
    S = tree_sum(terms, edge & ~flag_out)
    Hv = np.zeros((6, 6), F64)
    col = 0
    for j in range(6):
        for k in range(j, 6):
            Hv[j, k] = Hv[k, j] = S[col]
            col += 1
    _, J = inertial_edge(pre, prev, cur)
    Hi = mm(mm(J.T, info9), J)
    if lf:
        H = np.zeros((30, 30), F64)
        H[0:24, 0:24] = H[0:24, 0:24] + Hi
        for (Om, o1, o2) in ((infoG, 9, 24), (infoA, 12, 27)):
            H[o1:o1 + 3, o1:o1 + 3] = H[o1:o1 + 3, o1:o1 + 3] + Om
            H[o1:o1 + 3, o2:o2 + 3] = H[o1:o1 + 3, o2:o2 + 3] - Om
            H[o2:o2 + 3, o1:o1 + 3] = H[o2:o2 + 3, o1:o1 + 3] - Om
            H[o2:o2 + 3, o2:o2 + 3] = H[o2:o2 + 3, o2:o2 + 3] + Om
        _, Jp = prior_edge(pri, prev)
        H[0:15, 0:15] = H[0:15, 0:15] + mm(mm(Jp.T, pri["H"]), Jp)
        H[15:21, 15:21] = H[15:21, 15:21] + Hv
        # Marginalize(H, 0, 14): the pseudo-inverse of the previous frame's block through jacobi_eig of its lower triangle
        lam, Q = jacobi_eig(H[0:15, 0:15], 15)
        keep = np.abs(lam) > 1e-6
        inv_b = recompose(Q, np.where(keep, 1.0 / lam, 0.0))
        if not keep.all():
            flags |= FLAG_MARG_CUT
        Hf = H[15:30, 15:30] - mm(mm(H[15:30, 0:15], inv_b), H[0:15, 15:30])
    else:
        Hf = np.zeros((15, 15), F64)
        Hf[0:9, 0:9] = Hf[0:9, 0:9] + Hi[15:24, 15:24]
        Hf[9:12, 9:12] = Hf[9:12, 9:12] + infoG
        Hf[12:15, 12:15] = Hf[12:15, 12:15] + infoA
        Hf[0:6, 0:6] = Hf[0:6, 0:6] + Hv
    # ConstraintPoseImu's constructor: (H + H) / 2 changes nothing; the eigen-solver reads the lower triangle
    lam, V = jacobi_eig(Hf, 15)
    cl = lam < 1e-12
    if cl.any():
        flags |= FLAG_PRIOR_CLIPPED
    Hc = recompose(V, np.where(cl, 0.0, lam))
    so = pack_state(cur)
    prior_out = np.concatenate([so, Hc.reshape(-1)])
    if not (finite(so) and finite(Hc)):
        flags |= FLAG_NONFINITE
    stats[:8] = [n_init - n_bad, n_init, n_bad, n_init - n_stereo, n_stereo, rounds, tot_its, fails]
    stats[8], stats[9] = flags, n_inl
    return {"state": so, "state_f32": so.astype(F32), "outlier": out_outlier, "chi2": out_chi2, "prior_out": prior_out, "trace": trace,
            "stats": stats, "ret": int(stats[0]), "chi2_rounds": chi2_rounds}


def batch(P, cases):
    """B problems (dicts of pose_inertial_optimization's arguments, all of one N): the outputs stacked"""
    rs = [pose_inertial_optimization(P, **c) for c in cases]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("state", "state_f32", "outlier", "chi2", "prior_out", "trace", "stats")}


# ---------------------------------------------------------------- case generators
def _rot(w):
    return quat_to_mat(quat_from_rotvec(w))


def make_preint(rng, R1, p1, v1, R2, p2, v2, dT, bg, ba, noise=1e-4):
    """a preintegration consistent with the motion (R1, p1, v1) -> (R2, p2, v2) over dT at bias (bg, ba), with bias Jacobians and a
    covariance of the size a 200 Hz IMU of EuRoC's noise densities leaves"""
    g = np.array([0, 0, -float(GRAVITY)])
    dR = R1.T @ R2 @ _rot(rng.standard_normal(3) * noise)
    dV = R1.T @ (v2 - v1 - g * dT) + rng.standard_normal(3) * noise
    dP = R1.T @ (p2 - p1 - v1 * dT - 0.5 * g * dT * dT) + rng.standard_normal(3) * noise
    A = rng.standard_normal((3, 3)) * 0.1
    JRg = -dT * (np.eye(3) + A * dT)
    JVa = -dT * (np.eye(3) + rng.standard_normal((3, 3)) * 0.05)
    JPa = -0.5 * dT * dT * (np.eye(3) + rng.standard_normal((3, 3)) * 0.05)
    JVg = rng.standard_normal((3, 3)) * 0.5 * dT * dT
    JPg = rng.standard_normal((3, 3)) * 0.2 * dT ** 3
    ng, na = 1.7e-4 * np.sqrt(200.0), 2.0e-3 * np.sqrt(200.0)
    k = dT * 200.0
    sd = np.concatenate([np.full(3, ng / 200 * np.sqrt(k)), np.full(3, na / 200 * np.sqrt(k)), np.full(3, 0.5 * na / 200 * dT * np.sqrt(k))])
    M = np.eye(9) + rng.standard_normal((9, 9)) * 0.05
    C = (M * sd[None, :]).T @ (M * sd[None, :])
    C = (C + C.T) / 2
    p = np.concatenate([[dT], dR.reshape(-1), dV, dP, JRg.reshape(-1), JVg.reshape(-1), JVa.reshape(-1), JPg.reshape(-1), JPa.reshape(-1), ba, bg,
                        C.reshape(-1)]).astype(F32)
    assert p.size == PREINT_FLOATS
    wg, wa = (1.9e-5 ** 2) * dT, (3.0e-3 ** 2) * dT
    cov_rw = np.concatenate([(np.eye(3) * wg).reshape(-1), (np.eye(3) * wa).reshape(-1)]).astype(F32)
    return p, cov_rw


def scene(seed, N, mode, kind="mixed", dT=0.05, gross=0.2, rot=np.deg2rad(2.0), trans=0.05, bias_off=0.1, noise=1.0, nlevels=4, has=0.9,
          prior_weight=2e5, prev=None):
    """a planted frame: the body moves from the previous state to the true current one; N features (about `has` with a map point) are
    exact projections plus pixel noise, a fraction `gross` displaced by 50 .. 150 px; the start is `rot` rad / `trans` m off and the biases
    `bias_off` (relative) off.  The first frame's prior is isotropic with the information 100 inlier observations at 10 m leave on a position
    (100 (fx / z)^2, about 2e5).  prev: (state_f32 [21], prior [246]) of an earlier frame to continue from"""
    rng = np.random.default_rng(seed)
    sig2 = 1.44 ** np.arange(nlevels)
    P = params(458.654, 457.296, 367.215, 248.375, 47.91, (1.0 / sig2).astype(F32))
    Rcb = _rot(np.array([0.01, -0.02, 1.57]))
    tcb = np.array([0.06, -0.02, 0.01])
    Rbc, tbc = Rcb.T, -Rcb.T @ tcb
    bg_t, ba_t = np.array([0.002, -0.001, 0.0015]), np.array([0.02, 0.05, -0.03])
    if prev is None:
        R1, p1, v1 = _rot(rng.standard_normal(3) * 0.3), rng.standard_normal(3) * 0.5, rng.standard_normal(3) * 0.5
        prev_state = np.concatenate([R1.reshape(-1), p1, v1, bg_t, ba_t]).astype(F32)
        prior = np.concatenate([prev_state.astype(F64), (np.eye(15) * prior_weight).reshape(-1)])
    else:
        prev_state, prior = np.asarray(prev[0], F32), np.asarray(prev[1], F64)
        s = prev_state.astype(F64)
        R1, p1, v1 = s[0:9].reshape(3, 3), s[9:12], s[12:15]
    acc = rng.standard_normal(3) * 1.0
    R2 = R1 @ _rot(rng.standard_normal(3) * 0.5 * dT)
    v2 = v1 + acc * dT
    p2 = p1 + v1 * dT + 0.5 * acc * dT * dT
    preint, cov_rw = make_preint(rng, R1, p1, v1, R2, p2, v2, dT, bg_t, ba_t)
    Rcw_t = Rcb @ R2.T
    tcw_t = Rcb @ (-R2.T @ p2) + tcb
    z = rng.uniform(2.0, 20.0, N)
    u, v = rng.uniform(20, 730, N), rng.uniform(20, 460, N)
    Xc = np.stack([(u - float(P["cx"])) / float(P["fx"]) * z, (v - float(P["cy"])) / float(P["fy"]) * z, z], 1)
    xw = ((Xc - tcw_t) @ Rcw_t).astype(F32)
    octave = rng.integers(0, nlevels, N).astype(np.int32) if kind == "mixed" else np.zeros(N, np.int32)
    stereo = {"mono": np.zeros(N, bool), "stereo": np.ones(N, bool), "mixed": rng.random(N) < 0.5}[kind]
    sg = np.sqrt(sig2)[octave] * noise
    ur = u - float(P["bf"]) / z
    planted = rng.random(N) < gross
    ang, mag = rng.uniform(0, 2 * np.pi, N), rng.uniform(50, 150, N)
    u = u + sg * rng.standard_normal(N) + planted * mag * np.cos(ang)
    v = v + sg * rng.standard_normal(N) + planted * mag * np.sin(ang)
    ur = ur + sg * rng.standard_normal(N)
    uright = np.where(stereo, np.maximum(ur, 0.0), -1.0).astype(F32)
    has_mp = (rng.random(N) < has).astype(np.uint8)
    ax = rng.standard_normal(3)
    R0 = R2 @ _rot(ax / np.linalg.norm(ax) * rot)
    ax = rng.standard_normal(3)
    p0 = p2 + ax / np.linalg.norm(ax) * trans
    state = np.concatenate([R0.reshape(-1), p0, v2 + rng.standard_normal(3) * 0.02, bg_t * (1 + bias_off), ba_t * (1 + bias_off)]).astype(F32)
    s = state.astype(F64)
    R0f, p0f = s[0:9].reshape(3, 3), s[9:12]
    Rcw0 = Rcb @ R0f.T
    tcw0 = Rcb @ (-R0f.T @ p0f) + tcb
    cam = np.concatenate([Rcw0.reshape(-1), tcw0, Rcb.reshape(-1), tcb, Rbc.reshape(-1), tbc]).astype(F32)
    args = {"mode": mode, "rec_init": 0, "cam": cam, "state": state, "prev_state": prev_state, "preint": preint, "cov_rw": cov_rw,
            "prior_in": prior if mode == MODE_LAST_FRAME else None, "kpts": np.stack([u, v], 1).astype(F32), "octave": octave, "uright": uright,
            "xw": xw, "has_mp": has_mp, "track_depth": z.astype(F32)}
    truth = {"Rwb": R2, "twb": p2, "v": v2, "bg": bg_t, "ba": ba_t}
    return {"P": P, "args": args, "truth": truth, "planted": planted}


def solve(c, **kw):
    return pose_inertial_optimization(c["P"], **dict(c["args"], **kw))


def state_distance(s, truth):
    """(rotation rad, position m, velocity, gyro bias, acc bias) between a packed state [21] and a truth dict"""
    s = np.asarray(s, F64)
    R = s[0:9].reshape(3, 3)
    dR = truth["Rwb"].T @ R
    ang = float(np.arctan2(np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2, (np.trace(dR) - 1) / 2))
    return (ang, float(np.linalg.norm(s[9:12] - truth["twb"])), float(np.linalg.norm(s[12:15] - truth["v"])),
            float(np.linalg.norm(s[15:18] - truth["bg"])), float(np.linalg.norm(s[18:21] - truth["ba"])))


def chain(seed, N, modes, kind="mixed", **kw):
    """consecutive frames, each call's prior_out / state_f32 the next one's prior_in / prev_state: a list of (case, result)"""
    out, prev = [], None
    for k, mode in enumerate(modes):
        c = scene(seed + k, N, mode, kind, prev=prev, **kw)
        if prev is None and mode == MODE_LAST_FRAME:
            pass                                            # the first frame's prior is the generator's isotropic one
        r = solve(c)
        out.append((c, r))
        prev = (r["state_f32"], r["prior_out"])
    return out


FORCED = ("failed_solve", "log_outside", "log_small", "info_clipped", "marg_cut", "huber_above", "huber_below", "few_edges_kf", "enough_edges_kf",
          "few_edges_f", "enough_edges_f", "recovery", "recovery_rec_init", "nan")


def forced(name):
    """the cases of the paths that planted scenes do not take by themselves (test_pose_inertial_ref.py, test_gpu_pose_inertial.py)"""
    KF, LF = MODE_LAST_KEYFRAME, MODE_LAST_FRAME
    if name == "failed_solve":                # a negative gyro random-walk block: InfoG is negative, the first pivot is, every round ends
        c = scene(41, 60, LF)                 # after one iteration with the stale x (zeros) applied
        c["args"]["cov_rw"][0:9] = -c["args"]["cov_rw"][0:9]
    elif name == "log_outside":               # the prior's rotation equals the previous state's float matrix: R^T R has a trace a few ulps
        for seed in range(200, 264):          # above or below 3; the first seed that leaves costheta > 1
            c = scene(seed, 40, LF)
            M = mm(c["args"]["prev_state"][0:9].astype(F64).reshape(3, 3).T, c["args"]["prev_state"][0:9].astype(F64).reshape(3, 3))
            if (((M[0, 0] + M[1, 1]) + M[2, 2]) - 1.0) * 0.5 > 1:
                break
        else:
            raise AssertionError("no seed leaves costheta > 1")
    elif name == "log_small":                 # both are the identity: costheta == 1, theta == 0, |sin theta| < 1e-5
        st = np.concatenate([np.eye(3).reshape(-1), [0.1, 0.2, 0.3], [0.3, -0.2, 0.1], [0.002, -0.001, 0.0015], [0.02, 0.05, -0.03]]).astype(F32)
        c = scene(201, 40, LF, prev=(st, np.concatenate([st.astype(F64), (np.eye(15) * 1e4).reshape(-1)])))
    elif name == "info_clipped":              # one direction of C with a variance of 1e13: its information 1e-13 is set to 0
        c = scene(42, 60, KF)
        c["args"]["preint"][67 + 8 * 9 + 8] = F32(1e13)
    elif name == "marg_cut":                  # the same with an empty prior: the previous frame's block is singular
        c = scene(43, 60, LF)
        c["args"]["preint"][67 + 8 * 9 + 8] = F32(1e13)
        c["args"]["prior_in"][21:] = 0.0
    elif name == "huber_above":               # the prior 10 cm off under a weight of 2e5: chi2 = 2000 > 25
        c = scene(44, 60, LF)
        c["args"]["prior_in"][9] += 0.1
    elif name == "huber_below":
        c = scene(45, 60, LF)
    elif name in ("few_edges_kf", "enough_edges_kf", "few_edges_f", "enough_edges_f"):
        n = {"few_edges_kf": 6, "enough_edges_kf": 7, "few_edges_f": 5, "enough_edges_f": 6}[name]
        c = scene(46, n, LF if name.endswith("_f") else KF, has=1.0, gross=0.0)
    elif name in ("recovery", "recovery_rec_init"):   # 25 edges, half of them displaced by 3 .. 4 px: outliers at 5.991, below 18
        c = scene(47, 25, KF, "mono", has=1.0, gross=0.0, noise=0.2)
        c["args"]["kpts"][::2, 0] += F32(3.5)
        c["args"]["rec_init"] = 1 if name == "recovery_rec_init" else 0
    elif name == "nan":
        c = scene(48, 60, LF)
        c["args"]["has_mp"][7] = 1
        c["args"]["xw"][7, 1] = np.nan
    else:
        raise KeyError(name)
    return c
# measured by test_pose_inertial_ref.py: the relative gap between EdgeInertial's d er / d bg block (first order in the bias change) and
# central differences of the error, at a gyro bias 2e-3 rad/s off the preintegration's
INERTIAL_DER_DBG_GAP = {0.05: 6.8e-8, 0.5: 7.0e-8}

# measured by test_pose_inertial_ref.py::test_cost_of_the_departures (worst over its scenes and its chain): the largest difference between
# this restatement and the sequential transcription tests/pose_inertial_seq.py run with the reference's own choices -- entries of Rwb, position (m), velocity (m/s), gyro bias, accelerometer bias, and
# prior_out's H relative to its Frobenius norm.  The float NormalizeRotation of GetDeltaRotation (a float SVD there, the stated step in
# double here) accounts for most of it: dR moves by a float ulp
DEPARTURE_COST = {"rotation": 1.1e-8, "position": 1.1e-8, "velocity": 6.8e-8, "bg": 2.2e-8, "ba": 8.7e-10, "H": 9.4e-9}

# measured by test_pose_inertial_ref.py::test_planted_scene_is_recovered: the worst (rotation rad, position m) left after the optimisation
# from 2 degrees / 5 cm off, by mode, over its scenes (pixel noise of one sigma per level is what remains)
PLANTED_RESIDUAL = {MODE_LAST_KEYFRAME: (2.4e-4, 1.5e-4), MODE_LAST_FRAME: (8.4e-4, 2.2e-3)}
