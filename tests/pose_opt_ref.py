"""numpy float64 restatement of Optimizer::PoseOptimization (reference src/Optimizer.cc:55-401 over g2o's Levenberg-Marquardt, one SE3
vertex and unary mono / stereo edges), the contract of DESIGN.md 6i: the per-edge arithmetic as array operations in the order the contract
writes them, the sums over edges in the fixed order of departure (a), the explicit sincos of departure (b), the pivoted LDLT of departure
(c), and the serial section (lambda policy, exp, rounds) in scalar float64.  Shared by test_pose_opt_ref.py (CPU), test_gpu_pose_opt.py,
test_gpu_pose_opt_dropin.py and tools/bench_pose_opt.py; holds the case generators."""
import numpy as np

F32 = np.float32
F64 = np.float64
MAX_LEVELS = 16
LANES = 256
DBL_MAX = np.finfo(F64).max
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)
DELTA_MONO, DELTA_STEREO = F64(F32(np.sqrt(F64(5.991)))), F64(F32(np.sqrt(F64(7.815))))
# RobustKernelHuber keeps dsqr in a float member (robust_kernel_impl.h:84)
DSQR_MONO, DSQR_STEREO = F64(F32(DELTA_MONO * DELTA_MONO)), F64(F32(DELTA_STEREO * DELTA_STEREO))
FLAG_ENDED_REJECTED, FLAG_SOLVE_FAILED, FLAG_NONFINITE = 1, 2, 4
ROUNDS = 4                                  # a test that wants the flags after an earlier round lowers it

# ---------------------------------------------------------------- departure (b): sin and cos
TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
PIO2_1 = float.fromhex("0x1.921fb544p+0")            # the first 33 bits of pi / 2: k PIO2_1 is exact for k < 2^20
PIO2_2 = float.fromhex("0x1.0b4611a6p-34")
PIO2_3 = float.fromhex("0x1.3198a2ep-69")
PIO2_4 = float.fromhex("0x1.b839a252049c1p-104")
SIN_C = [float.fromhex(h) for h in ("-0x1.5555555555549p-3", "0x1.111111110f8a6p-7", "-0x1.a01a019c161d5p-13", "0x1.71de357b1fe7dp-19",
                                    "-0x1.ae5e68a2b9cebp-26", "0x1.5d93a5acfd57cp-33")]
COS_C = [float.fromhex(h) for h in ("0x1.555555555554cp-5", "-0x1.6c16c16c15177p-10", "0x1.a01a019cb159p-16", "-0x1.27e4f809c52adp-22",
                                    "0x1.1ee9ebdb4b1c4p-29", "-0x1.8fae9be8838d4p-37")]
SINCOS_LOG = None                                     # a list here receives the quadrant (k mod 4) of every call, -1 for the r = 0 fallback
R_MAX = 0.79                                          # pi / 4 and slack: a reduction that lands outside (theta past 2^53 or so) reads r = 0


def sincos(theta):
    """(sin, cos) of a float64 theta >= 0: k = floor(theta 2/pi + 0.5), r = theta - k pi/2 in four Cody-Waite steps, the two polynomials
    in Horner form, the quadrant from k mod 4, clamped to [-1, 1].  One rounding per operation."""
    theta = F64(theta)
    k = np.floor(theta * TWO_OVER_PI + 0.5)
    r = (((theta - k * PIO2_1) - k * PIO2_2) - k * PIO2_3) - k * PIO2_4
    fallback = not (np.abs(r) <= R_MAX)
    if fallback:
        r = F64(0.0)
    q = int(np.fmod(k, 4.0)) if np.isfinite(k) else 0
    if SINCOS_LOG is not None:
        SINCOS_LOG.append(-1 if fallback else q)
    z = r * r
    ps = SIN_C[5]
    for c in (SIN_C[4], SIN_C[3], SIN_C[2], SIN_C[1], SIN_C[0]):
        ps = c + z * ps
    s = r + (r * z) * ps
    pc = COS_C[5]
    for c in (COS_C[4], COS_C[3], COS_C[2], COS_C[1], COS_C[0]):
        pc = c + z * pc
    c = (1.0 - 0.5 * z) + (z * z) * pc
    if q == 1:
        s, c = c, -s
    elif q == 2:
        s, c = -s, -c
    elif q == 3:
        s, c = -c, s
    s = min(max(s, -1.0), 1.0)
    c = min(max(c, -1.0), 1.0)
    return F64(s), F64(c)


# ---------------------------------------------------------------- departure (c): the 6 x 6 solve
def ldlt_solve(M, b):
    """M: symmetric 6 x 6 (nested lists of float64), b: 6.  LDLT with diagonal pivoting -- the largest |diagonal| of the trailing block, the
    first maximum; a negative pivot: not positive, (False, None).  A zero pivot leaves its column of L zero and its y zero."""
    A = [[F64(M[i][j]) for j in range(6)] for i in range(6)]
    perm = list(range(6))
    d = [F64(0.0)] * 6
    for k in range(6):
        p, best = k, np.abs(A[k][k])
        for j in range(k + 1, 6):
            if np.abs(A[j][j]) > best:
                p, best = j, np.abs(A[j][j])
        if p != k:
            A[k], A[p] = A[p], A[k]
            for row in A:
                row[k], row[p] = row[p], row[k]
            perm[k], perm[p] = perm[p], perm[k]
        d[k] = A[k][k]
        if d[k] < 0.0:
            return False, None
        for i in range(k + 1, 6):
            A[i][k] = A[i][k] / d[k] if d[k] != 0.0 else F64(0.0)          # L[i][k]; row k right of the diagonal keeps the unscaled column
        for i in range(k + 1, 6):
            for j in range(k + 1, i + 1):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
                A[j][i] = A[i][j]
    y = [F64(b[perm[i]]) for i in range(6)]
    for i in range(6):
        for j in range(i):
            y[i] = y[i] - A[i][j] * y[j]
    for i in range(6):
        y[i] = y[i] / d[i] if d[i] != 0.0 else F64(0.0)
    for i in range(5, -1, -1):
        for j in range(i + 1, 6):
            y[i] = y[i] - A[j][i] * y[j]
    x = [F64(0.0)] * 6
    for i in range(6):
        x[perm[i]] = y[i]
    return True, x


# ---------------------------------------------------------------- departure (a): sums over edges
def tree_sum(values, active):
    """values [n, C] float64 by feature index, active [n] bool.  Partial p adds the active features i = p (mod 256) in ascending i, from
    +0.0; the 256 partials are combined by stride halving.  Adding +0.0 for an inactive feature equals skipping it bit for bit."""
    n, C = values.shape
    part = np.zeros((LANES, C), F64)
    for c0 in range(0, n, LANES):
        m = min(LANES, n - c0)
        part[:m] = part[:m] + np.where(active[c0:c0 + m, None], values[c0:c0 + m], 0.0)
    s = LANES // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0].copy()


# ---------------------------------------------------------------- SE3
def normalize_rotation(q):
    x, y, z, w = q
    if w < 0:
        x, y, z, w = -x, -y, -z, -w
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)
    return [x / n, y / n, z / n, w / n]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def rotate(q, X):
    """Eigen's quaternion * vector on scalars or arrays: uv = 2 (v x X); X + w uv + v x uv"""
    v = q[:3]
    uv = cross(v, X)
    uv = [u + u for u in uv]
    c2 = cross(v, uv)
    return [(X[i] + q[3] * uv[i]) + c2[i] for i in range(3)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [((aw * bx + ax * bw) + ay * bz) - az * by,
            ((aw * by + ay * bw) + az * bx) - ax * bz,
            ((aw * bz + az * bw) + ax * by) - ay * bx,
            ((aw * bw - ax * bx) - ay * by) - az * bz]


def mat_to_quat(m):
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t, w]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
    q = [None] * 4
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q


def se3_exp(x):
    """SE3Quat::exp (se3quat.h:223-257): omega = x[0:3], upsilon = x[3:6]; returns (q, t), q normalised"""
    o, u = x[:3], x[3:]
    theta = np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    zero = F64(0.0)
    Om = [[zero, -o[2], o[1]], [o[2], zero, -o[0]], [-o[1], o[0], zero]]
    Om2 = [[(Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c] for c in range(3)] for r in range(3)]
    eye = [[F64(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    if theta < 0.00001:
        R = [[(eye[r][c] + Om[r][c]) + Om2[r][c] for c in range(3)] for r in range(3)]
        V = R
    else:
        s, c = sincos(theta)
        a = s / theta
        b = (1.0 - c) / (theta * theta)
        g = (theta - s) / ((theta * theta) * theta)
        R = [[(eye[r][k] + a * Om[r][k]) + b * Om2[r][k] for k in range(3)] for r in range(3)]
        V = [[(eye[r][k] + b * Om[r][k]) + g * Om2[r][k] for k in range(3)] for r in range(3)]
    t = [(V[r][0] * u[0] + V[r][1] * u[1]) + V[r][2] * u[2] for r in range(3)]
    return normalize_rotation(mat_to_quat(R)), t


def se3_mul(q1, t1, q2, t2):
    r = rotate(q1, t2)
    t = [t1[i] + r[i] for i in range(3)]
    return normalize_rotation(quat_mul(q1, q2)), t


# ---------------------------------------------------------------- edges
def edge_terms(P, q, t, f, linearise, robust=True):
    """every feature's error, chi2, rho and -- with `linearise` -- its 21 + 6 contributions at the estimate (q, t).  f: the per-feature
    float64 arrays of features().  Returns chi2 [n], rho0 [n] (robust chi2), rho1 [n] and terms [n, 28] (H upper triangle row by row, the 6
    sums whose negative is b; column 27 is left to the caller)."""
    fx, fy, cx, cy, bf = (F64(P[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    n = len(f["u"])
    X = rotate(q, [f["X"][:, 0], f["X"][:, 1], f["X"][:, 2]])
    x, y, z = X[0] + t[0], X[1] + t[1], X[2] + t[2]
    st, isg = f["stereo"], f["invsigma2"]
    # mono: Pinhole::project, left to right; stereo: cam_project with the float invz
    em0 = f["u"] - (fx * x / z + cx)
    em1 = f["v"] - (fy * y / z + cy)
    invzf = (1.0 / z).astype(F32).astype(F64)
    pu = x * invzf * fx + cx
    pv = y * invzf * fy + cy
    pr = pu - bf * invzf
    e = [np.where(st, f["u"] - pu, em0), np.where(st, f["v"] - pv, em1), np.where(st, f["ur"] - pr, 0.0)]
    chi2 = e[0] * (isg * e[0]) + e[1] * (isg * e[1])
    chi2 = np.where(st, chi2 + e[2] * (isg * e[2]), chi2)
    delta, dsqr = np.where(st, DELTA_STEREO, DELTA_MONO), np.where(st, DSQR_STEREO, DSQR_MONO)
    sq = np.sqrt(chi2)
    inl = chi2 <= dsqr
    rho0 = np.where(inl, chi2, 2 * sq * delta - dsqr)
    rho1 = np.where(inl, 1.0, delta / sq)
    if not robust:                                # base_unary_edge.hpp:65-66 are the robust lines with rho1 = 1: a product by 1.0 is exact
        rho0, rho1 = chi2, np.ones(n, F64)
    if not linearise:
        return chi2, rho0, rho1, None
    zero, one = np.zeros(n, F64), np.ones(n, F64)
    # mono: -projectJac * SE3deriv, every product and sum of the 2x3 by 3x6 product written out
    nJ = [[-(fx / z), -zero, -(-fx * x / (z * z))], [-zero, -(fy / z), -(-fy * y / (z * z))]]
    S = [[zero, z, -y, one, zero, zero], [-z, zero, x, zero, one, zero], [y, -x, zero, zero, zero, one]]
    Am = [[(nJ[r][0] * S[0][c] + nJ[r][1] * S[1][c]) + nJ[r][2] * S[2][c] for c in range(6)] for r in range(2)]
    # stereo: types_six_dof_expmap.cpp:375-404 with the double invz
    invz = 1.0 / z
    invz2 = invz * invz
    As = [[x * y * invz2 * fx, -(1 + (x * x * invz2)) * fx, y * invz * fx, -invz * fx, zero, x * invz2 * fx],
          [(1 + y * y * invz2) * fy, -x * y * invz2 * fy, -x * invz * fy, zero, -invz * fy, y * invz2 * fy]]
    As.append([As[0][0] - bf * y * invz2, As[0][1] + bf * x * invz2, As[0][2], As[0][3], zero, As[0][5] - bf * invz2])
    A = [[np.where(st, As[r][c], Am[r][c]) for c in range(6)] for r in range(2)] + [As[2]]
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
    return chi2, rho0, rho1, terms


def features(P, kpts, octave, uright, xw, has_mp, n):
    n = int(n)
    octv = np.zeros(n, np.int64) if octave is None else np.asarray(octave[:n], np.int64).copy()
    octv[(octv < 0) | (octv >= P["nlevels"])] = 0
    ur = np.full(n, -1.0, F32) if uright is None else np.asarray(uright[:n], F32)
    return {"u": kpts[:n, 0].astype(F64), "v": kpts[:n, 1].astype(F64), "ur": ur.astype(F64), "stereo": ~(ur < 0),
            "X": np.asarray(xw[:n], F32).astype(F64).reshape(n, 3), "invsigma2": np.asarray(P["inv_level_sigma2"], F32)[octv].astype(F64),
            "edge": np.asarray(has_mp[:n]) != 0}


def params(fx, fy, cx, cy, bf, inv_level_sigma2=(1.0,), iterations=(0, 0, 0, 0), max_trials=0):
    return {"fx": F32(fx), "fy": F32(fy), "cx": F32(cx), "cy": F32(cy), "bf": F32(bf), "nlevels": len(inv_level_sigma2),
            "inv_level_sigma2": np.asarray(inv_level_sigma2, F32), "iterations": tuple(int(i) for i in iterations), "max_trials": int(max_trials)}


def finite(v):
    return bool(np.all(np.isfinite(np.asarray(v, F64))))


# ---------------------------------------------------------------- the optimisation
def pose_optimization(P, pose0, kpts, octave, uright, xw, has_mp, n=None, outlier=None, chi2=None):
    """one problem.  pose0 [7] float32 (qx qy qz qw tx ty tz); kpts [N, 2], xw [N, 3] float32; has_mp [N] uint8; octave / uright [N] or None;
    n <= N features count.  outlier / chi2: what the output arrays hold before the call (default zeros).  Returns a dict of pose (float64
    [7]), pose_f32, outlier (uint8 [N]), chi2 (float32 [N]), trace (float64 [4, 8]), stats (int32 [8]) and ret."""
    with np.errstate(all="ignore"):
        return _pose_optimization(P, pose0, kpts, octave, uright, xw, has_mp, n, outlier, chi2)


def _pose_optimization(P, pose0, kpts, octave, uright, xw, has_mp, n, outlier, chi2):
    N = len(kpts)
    n = N if n is None else min(max(int(n), 0), N)
    pose0 = np.asarray(pose0, F32)
    out_outlier = np.zeros(N, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    out_chi2 = np.zeros(N, F32) if chi2 is None else np.array(chi2, F32)
    trace, stats = np.zeros((4, 8), F64), np.zeros(8, np.int32)
    f = features(P, kpts, octave, uright, xw, has_mp, n)
    edge = f["edge"]
    out_outlier[:n][edge] = 0
    n_init = int(edge.sum())
    stats[1] = n_init
    res = {"outlier": out_outlier, "chi2": out_chi2, "trace": trace, "stats": stats}
    if n_init < 3:
        res.update(pose=pose0.astype(F64), pose_f32=pose0.copy(), ret=0)
        return res
    its = [i if i > 0 else 10 for i in P["iterations"]]
    max_trials = P["max_trials"] if P["max_trials"] > 0 else 10
    q0, t0 = normalize_rotation([F64(v) for v in pose0[:4]]), [F64(v) for v in pose0[4:]]
    outl = np.zeros(n, bool)                      # level 1
    last_chi2 = np.zeros(n, F64)                  # chi2 of the _error the last computeActiveErrors left
    thr = np.where(f["stereo"], CHI2_STEREO, CHI2_MONO)
    x = [F64(0.0)] * 6
    flags = n_bad = 0
    q, t = q0, t0
    for rnd in range(ROUNDS):
        q, t = q0, t0
        active = edge & ~outl
        robust = rnd < 3

        def errors(q, t, linearise):
            c2, r0, _, terms = edge_terms(P, q, t, f, linearise, robust)
            last_chi2[active] = c2[active]
            if terms is None:
                terms = np.zeros((n, 28), F64)
            terms[:, 27] = r0
            return tree_sum(terms, active)

        lam, ni, nbad_lm = F64(0.0), F64(2.0), 0
        iters = trials = 0
        ended_rejected = False
        current = F64(0.0)
        for it in range(its[rnd]):
            iters += 1
            S = errors(q, t, True)
            current = S[27]
            ini = current
            H = [[None] * 6 for _ in range(6)]
            col = 0
            for j in range(6):
                for k in range(j, 6):
                    H[j][k] = H[k][j] = S[col]
                    col += 1
            b = [-S[21 + j] for j in range(6)]
            if it == 0:
                maxd = F64(0.0)
                for j in range(6):
                    a = np.abs(H[j][j])
                    maxd = maxd if a < maxd else a
                lam, ni, nbad_lm = 1e-5 * maxd, F64(2.0), 0
            rho, qmax = F64(0.0), 0
            while True:
                trials += 1
                M = [[H[j][k] + lam if j == k else H[j][k] for k in range(6)] for j in range(6)]
                ok, sol = ldlt_solve(M, b)
                if ok:
                    x = sol
                else:
                    flags |= FLAG_SOLVE_FAILED
                dq, dt = se3_exp(x)
                qn, tn = se3_mul(dq, dt, q, t)
                if not finite(qn + tn):
                    flags |= FLAG_NONFINITE
                temp = errors(qn, tn, False)[27]
                if not ok:
                    temp = DBL_MAX
                scale = F64(0.0)
                for j in range(6):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + 1e-3
                rho = (current - temp) / scale
                if rho > 0 and np.isfinite(temp):
                    v = 2 * rho - 1
                    alpha = 1.0 - (v * v) * v
                    alpha = F64(2.0 / 3.0) if F64(2.0 / 3.0) < alpha else alpha
                    lam = lam * (alpha if F64(1.0 / 3.0) < alpha else F64(1.0 / 3.0))
                    ni = F64(2.0)
                    current = temp
                    q, t = qn, tn
                    ended_rejected = False
                else:
                    lam = lam * ni
                    ni = ni * 2
                    stats[6] += 1
                    ended_rejected = True
                qmax += 1
                if not (rho < 0 and qmax < max_trials):
                    break
            if qmax == max_trials or rho == 0:
                break
            if (ini - current) * 1e3 < ini:
                nbad_lm += 1
            else:
                nbad_lm = 0
            if nbad_lm >= 3:
                break
        if ended_rejected:
            flags |= FLAG_ENDED_REJECTED
        # classification: an outlier edge recomputes its error at the round's estimate, an inlier keeps its last one
        c2, _, _, _ = edge_terms(P, q, t, f, False)
        last_chi2[edge & outl] = c2[edge & outl]
        c2f = last_chi2.astype(F32)
        outl = edge & (c2f > thr)
        n_bad = int(outl.sum())
        out_outlier[:n][edge] = outl[edge]
        out_chi2[:n][edge] = c2f[edge]
        stats[3] += 1
        stats[4] += iters
        stats[5] += trials
        trace[rnd, :5] = [iters, trials, lam, current, n_init - n_bad]
        if n_init < 10:
            break
    pose = np.array(list(q) + list(t), F64)
    if not finite(pose):
        flags |= FLAG_NONFINITE
    stats[0], stats[2], stats[7] = n_init - n_bad, n_bad, flags
    res.update(pose=pose, pose_f32=pose.astype(F32), ret=int(stats[0]))
    return res


def pose_optimization_batch(P, pose0, kpts, octave, uright, xw, has_mp, n=None, outlier=None, chi2=None):
    """B problems: the arrays of pose_optimization with a leading B; returns the outputs stacked"""
    B = len(pose0)
    rs = [pose_optimization(P, pose0[b], kpts[b], None if octave is None else octave[b], None if uright is None else uright[b], xw[b], has_mp[b],
                            None if n is None else n[b], None if outlier is None else outlier[b], None if chi2 is None else chi2[b]) for b in range(B)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("pose", "pose_f32", "outlier", "chi2", "trace", "stats")}


# ---------------------------------------------------------------- case generators
def quat_from_rotvec(w):
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.array([0, 0, 0, 1], F64)
    return np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def quat_to_mat(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F64)


def pose_distance(p, truth):
    """(rotation angle in rad, translation distance) between two poses [7]: the angle from the vector part of the relative quaternion,
    which resolves differences far below acos's 1e-8"""
    qa, qb = np.asarray(p[:4], F64), np.asarray(truth[:4], F64)
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    rel = np.array(quat_mul([-qa[0], -qa[1], -qa[2], qa[3]], list(qb)), F64)
    return float(2 * np.arctan2(np.linalg.norm(rel[:3]), abs(rel[3]))), float(np.linalg.norm(np.asarray(p[4:], F64) - np.asarray(truth[4:], F64)))


def scene(seed, N, kind="mixed", noise=1.0, gross=0.2, rot=0.05, trans=0.1, nlevels=4, has=0.9):
    """a synthetic frame: N features of which about `has` carry a map point; exact projections of points 2 .. 20 m in front of the true
    pose plus Gaussian pixel noise (scaled by the level's sigma), a fraction `gross` displaced by 50 .. 150 px, and a start `rot` rad and
    `trans` m off.  kind: mono, stereo or mixed (mixed draws octaves too)."""
    rng = np.random.default_rng(seed)
    sig2 = 1.44 ** np.arange(nlevels)
    P = params(458.654, 457.296, 367.215, 248.375, 47.91, (1.0 / sig2).astype(F32))
    q_true = quat_from_rotvec(rng.standard_normal(3) * 0.3)
    t_true = rng.standard_normal(3) * 0.5
    R = quat_to_mat(q_true)
    z = rng.uniform(2.0, 20.0, N)
    u, v = rng.uniform(20, 730, N), rng.uniform(20, 460, N)
    Xc = np.stack([(u - float(P["cx"])) / float(P["fx"]) * z, (v - float(P["cy"])) / float(P["fy"]) * z, z], 1)
    xw = ((Xc - t_true) @ R).astype(F32)                     # R^T (Xc - t)
    octave = rng.integers(0, nlevels, N).astype(np.int32) if kind == "mixed" else np.zeros(N, np.int32)
    stereo = {"mono": np.zeros(N, bool), "stereo": np.ones(N, bool), "mixed": rng.random(N) < 0.5}[kind]
    s = np.sqrt(sig2)[octave] * noise
    ur = u - float(P["bf"]) / z
    planted = rng.random(N) < gross
    ang, mag = rng.uniform(0, 2 * np.pi, N), rng.uniform(50, 150, N)
    u = u + s * rng.standard_normal(N) + planted * mag * np.cos(ang)
    v = v + s * rng.standard_normal(N) + planted * mag * np.sin(ang)
    ur = ur + s * rng.standard_normal(N)
    uright = np.where(stereo, np.maximum(ur, 0.0), -1.0).astype(F32)
    has_mp = (rng.random(N) < has).astype(np.uint8)
    dq = quat_from_rotvec(_unit(rng.standard_normal(3)) * rot)
    q0 = np.array(quat_mul(list(dq), list(q_true)), F64)
    t0 = t_true + _unit(rng.standard_normal(3)) * trans
    return {"P": P, "pose0": np.concatenate([q0, t0]).astype(F32), "kpts": np.stack([u, v], 1).astype(F32), "octave": octave, "uright": uright,
            "xw": xw, "has_mp": has_mp, "truth": np.concatenate([q_true, t_true]), "planted": planted}


def _unit(v):
    return v / np.linalg.norm(v)


def solve(c, **kw):
    return pose_optimization(c["P"], c["pose0"], c["kpts"], c["octave"], c["uright"], c["xw"], c["has_mp"], **kw)


def forced(name):
    """the cases of the paths that random scenes do not take (test_pose_opt_ref.py, test_gpu_pose_opt.py)"""
    if name == "rejected":                    # one trial per iteration from 0.5 rad off: a round ends on its rejected first step
        c = scene(21, 300, "mixed", rot=0.5, trans=0.3)
        c["P"] = dict(c["P"], max_trials=1)
    elif name == "stale":                     # two trials per iteration: round 0 ends near its minimum on two rejected steps, all inliers active
        c = scene(29, 300, "mixed", rot=0.2, trans=0.5)
        c["P"] = dict(c["P"], max_trials=2)
    elif name in ("quadrants", "huge_step"):  # observations a million / 1e20 px off: steps of many radians reach every quadrant of sincos;
        c = scene(35, 40, "mixed", has=1.0)   # steps past 2^53 rad its r = 0 fallback
        rng = np.random.default_rng(35)
        c["kpts"] = (c["kpts"] + (1e6 if name == "quadrants" else 1e20) * rng.standard_normal(c["kpts"].shape)).astype(F32)
    elif name == "one_iteration":
        c = scene(22, 300, "mixed")
        c["P"] = dict(c["P"], iterations=(1, 1, 1, 1))
    elif name == "exact":
        c = _exact_case()
    elif name == "two":
        c = scene(24, 2, "mixed", has=1.0)
    elif name == "nine":
        c = scene(25, 9, "mixed", has=1.0, gross=0.0)
    elif name == "comes_back":
        c = scene(26, 300, "mixed")           # one iteration in round 0 leaves a poor pose: inliers it rejects come back in round 1
        c["P"] = dict(c["P"], iterations=(1, 10, 10, 10))
    elif name == "behind":                    # one point behind the camera (z < 0)
        c = scene(27, 120, "mixed", has=1.0)
        R, t = quat_to_mat(c["truth"][:4]), c["truth"][4:]
        c["special"] = 5
        c["xw"][5] = ((np.array([0.3, -0.2, -4.0]) - t) @ R).astype(F32)
    elif name == "nan":
        c = scene(28, 120, "mixed", has=1.0)
        c["special"] = 7
        c["xw"][7, 1] = np.nan
    else:
        raise KeyError(name)
    return c


def _exact_case(N=64):
    """errors that are 0.0 at pose0: the identity pose, depths that are powers of two, focal lengths and offsets that are small integers,
    so every projection is a float.  b = 0, x = 0, the trial leaves chi2 at 0 and rho == 0 ends each round after one rejected trial"""
    rng = np.random.default_rng(23)
    P = params(512.0, 512.0, 320.0, 240.0, 48.0, (1.0, 0.5))
    z = 2.0 ** rng.integers(1, 4, N)
    x, y = rng.integers(-200, 200, N) / 128.0, rng.integers(-150, 150, N) / 128.0
    u, v = 512.0 * x / z + 320.0, 512.0 * y / z + 240.0
    stereo = rng.random(N) < 0.5
    uright = np.where(stereo, u - 48.0 / z, -1.0)
    c = {"P": P, "pose0": np.array([0, 0, 0, 1, 0, 0, 0], F32), "kpts": np.stack([u, v], 1).astype(F32), "octave": rng.integers(0, 2, N).astype(np.int32),
         "uright": uright.astype(F32), "xw": np.stack([x, y, z], 1).astype(F32), "has_mp": np.ones(N, np.uint8), "planted": np.zeros(N, bool)}
    c["truth"] = c["pose0"].astype(F64)
    assert np.array_equal(c["kpts"][:, 0].astype(F64), u) and np.array_equal(c["uright"].astype(F64), uright)
    return c
