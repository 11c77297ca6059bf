"""numpy float64 restatement of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4195-4494 over g2o's Levenberg-Marquardt: one free
VertexSim3Expmap, an EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ per matched pair, both linearised by g2o's numeric central
differences), the contract of DESIGN.md 6k: the per-pair arithmetic as array operations in the order the contract writes them, the sums
over pairs in the fixed order of departure (a), the sincos of departure (b) and the pivoted LDLT of departure (c) as 6i has them, the exp
of departure (d), and the serial section (lambda policy, Sim3(update), rounds) in scalar float64.  Shared by test_optimize_sim3_ref.py
(CPU), test_gpu_optimize_sim3.py, test_gpu_optimize_sim3_dropin.py and tools/bench_optimize_sim3.py; holds the case generators."""
import numpy as np

from pose_opt_ref import DBL_MAX, F32, F64, LANES, cross, finite, mat_to_quat, quat_from_rotvec, quat_mul, quat_to_mat, rotate, sincos

MAX_LEVELS = 16
FLAG_ENDED_REJECTED, FLAG_SOLVE_FAILED, FLAG_NONFINITE, FLAG_IDX2, FLAG_EARLY = 1, 2, 4, 8, 16
NUM_DELTA = F64(1e-9)                                  # base_binary_edge.hpp:147-148
NUM_SCALAR = F64(1.0) / (2 * NUM_DELTA)
EPS = F64(0.00001)

# what the departures (a)-(d) cost, measured by test_optimize_sim3_ref.py::test_departure_cost on its cases (the largest absolute difference
# of any of the 8 Sim3 numbers from the transcription with g2o's own choices); the test allows 8 times as much
DEPARTURE_SIM3_MAX = 5.1e-9
# the largest distance of exp_ from libm's exp over [-5, 5], in ulps (test_optimize_sim3_ref.py::test_exp_against_libm)
EXP_MAX_ULP = 1
# how much closer to the planted Sim3 the optimisation gets in test_it_optimises, before / after: 175x in rotation, 72x in translation and
# 12.3x in log scale with the scale free, 579x and 461x with it fixed, measured when the test was written; the test asks for a sixteenth
# of the smallest
OPTIMISES_GAIN = 12.3

# ---------------------------------------------------------------- departure (d): exp
LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
EXP_P = [float.fromhex(h) for h in ("0x1.555555555553ep-3", "-0x1.6c16c16bebd93p-9", "0x1.1566aaf25de2cp-14", "-0x1.bbd41c5d26bf1p-20",
                                    "0x1.6376972bea4d0p-25")]
EXP_OVERFLOW = float.fromhex("0x1.62e42fefa39efp+9")
EXP_UNDERFLOW = float.fromhex("-0x1.74910d52d3051p+9")


def exp_(x):
    """fdlibm's e_exp without fma: k = floor(x / ln 2 + 0.5), r = (x - k ln2_hi) - k ln2_lo, the polynomial in Horner form, the result
    scaled by 2^k exactly.  NaN passes through, overflow gives inf, underflow 0, exp_(0) == 1."""
    x = F64(x)
    if x != x:
        return x
    if x > EXP_OVERFLOW:
        return F64(np.inf)
    if x < EXP_UNDERFLOW:
        return F64(0.0)
    k = np.floor(x * INV_LN2 + 0.5)
    hi = x - k * LN2_HI
    lo = k * LN2_LO
    r = hi - lo
    t = r * r
    p = F64(EXP_P[4])
    for c in (EXP_P[3], EXP_P[2], EXP_P[1], EXP_P[0]):
        p = c + t * p
    c = r - t * p
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    return F64(np.ldexp(y, int(k)))


# ---------------------------------------------------------------- departure (c): the D x D solve (6i's, any dimension)
def ldlt_solve(M, b):
    """M: symmetric D x D (nested lists of float64), b: D.  LDLT with diagonal pivoting -- the largest |diagonal| of the trailing block, the
    first maximum; a negative pivot: not positive, (False, None).  A zero pivot leaves its column of L zero and its y zero."""
    D = len(b)
    A = [[F64(M[i][j]) for j in range(D)] for i in range(D)]
    perm = list(range(D))
    d = [F64(0.0)] * D
    for k in range(D):
        p, best = k, np.abs(A[k][k])
        for j in range(k + 1, D):
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
        for i in range(k + 1, D):
            A[i][k] = A[i][k] / d[k] if d[k] != 0.0 else F64(0.0)
        for i in range(k + 1, D):
            for j in range(k + 1, i + 1):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
                A[j][i] = A[i][j]
    y = [F64(b[perm[i]]) for i in range(D)]
    for i in range(D):
        for j in range(i):
            y[i] = y[i] - A[i][j] * y[j]
    for i in range(D):
        y[i] = y[i] / d[i] if d[i] != 0.0 else F64(0.0)
    for i in range(D - 1, -1, -1):
        for j in range(i + 1, D):
            y[i] = y[i] - A[j][i] * y[j]
    x = [F64(0.0)] * D
    for i in range(D):
        x[perm[i]] = y[i]
    return True, x


# ---------------------------------------------------------------- departure (a): sums over pairs
def tree_sum2(v12, v21, active):
    """v12, v21 [n, C] float64 by row: e12's and e21's terms; active [n] bool.  Partial p takes the active rows i = p (mod 256) in ascending
    i, from +0.0, adding e12's term, then e21's; the 256 partials are combined by stride halving."""
    n, C = v12.shape
    part = np.zeros((LANES, C), F64)
    for c0 in range(0, n, LANES):
        m = min(LANES, n - c0)
        a = active[c0:c0 + m, None]
        part[:m] = (part[:m] + np.where(a, v12[c0:c0 + m], 0.0)) + np.where(a, v21[c0:c0 + m], 0.0)
    s = LANES // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0].copy()


# ---------------------------------------------------------------- Sim3: a list of 8 float64, qx qy qz qw tx ty tz s
def sim3_exp(u):
    """Sim3(update) (sim3.h:70-142): u = omega, upsilon, sigma; returns (q, t, s), q NOT normalised"""
    o, ups, sigma = u[:3], u[3:6], F64(u[6])
    theta = np.sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    zero, one = F64(0.0), F64(1.0)
    Om = [[zero, -o[2], o[1]], [o[2], zero, -o[0]], [-o[1], o[0], zero]]
    Om2 = [[(Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c] for c in range(3)] for r in range(3)]
    eye = [[F64(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    s = exp_(sigma)
    small = theta < EPS
    if small:
        R = [[(eye[r][c] + Om[r][c]) + Om2[r][c] for c in range(3)] for r in range(3)]
    else:
        sn, cs = sincos(theta)
        a, bq = sn / theta, (1.0 - cs) / (theta * theta)
        R = [[(eye[r][c] + a * Om[r][c]) + bq * Om2[r][c] for c in range(3)] for r in range(3)]
    if np.abs(sigma) < EPS:
        C = one
        if small:
            A, B = one / 2.0, one / 6.0
        else:
            theta2 = theta * theta
            A = (1.0 - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b, theta2, sigma2 = s * sn, s * cs, theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2
    W = [[(A * Om[r][c] + B * Om2[r][c]) + C * eye[r][c] for c in range(3)] for r in range(3)]
    t = [(W[r][0] * ups[0] + W[r][1] * ups[1]) + W[r][2] * ups[2] for r in range(3)]
    return mat_to_quat(R), t, s


def sim3_oplus(u, S):
    """Sim3(u) * S (sim3.h:266-272): r = r1 r2, t = s1 (r1 * t2) + t1, s = s1 s2; nothing is normalised"""
    q1, t1, s1 = sim3_exp(u)
    r = rotate(q1, S[4:7])
    return quat_mul(q1, S[:4]) + [s1 * r[i] + t1[i] for i in range(3)] + [s1 * S[7]]


def sim3_inverse(S):
    """(conj r, conj r * ((-1 / s) t), 1 / s) (sim3.h:233-236)"""
    qi = [-S[0], -S[1], -S[2], S[3]]
    c = F64(-1.0) / S[7]
    return qi + rotate(qi, [c * S[4], c * S[5], c * S[6]]) + [F64(1.0) / S[7]]


def sim3_map(S, X):
    r = rotate(S[:4], X)
    return [S[7] * r[i] + S[4 + i] for i in range(3)]


# ---------------------------------------------------------------- pairs
def params(rcw1, tcw1, rcw2, tcw2, cam1, cam2, inv1=(1.0,), inv2=(1.0,), th2=10.0, fix_scale=False, all_points=False, n=0, n2=0,
           iterations=(0, 0, 0), max_trials=0):
    return {"rcw1": np.asarray(rcw1, F32).reshape(3, 3), "tcw1": np.asarray(tcw1, F32).reshape(3), "rcw2": np.asarray(rcw2, F32).reshape(3, 3),
            "tcw2": np.asarray(tcw2, F32).reshape(3), "cam1": tuple(F32(v) for v in cam1), "cam2": tuple(F32(v) for v in cam2),
            "inv1": np.asarray(inv1, F32), "inv2": np.asarray(inv2, F32), "th2": F32(th2), "fix_scale": bool(fix_scale),
            "all_points": bool(all_points), "n": int(n), "n2": int(n2), "iterations": tuple(int(i) for i in iterations), "max_trials": int(max_trials)}


def to_camera(R, t, X):
    """R X + t in float32, ((r0 x + r1 y) + r2 z) + t; X [n, 3] float32"""
    return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


def pairs(P, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, n, n2):
    """the per-row float64 arrays of the n rows, the rows that carry an edge pair (Optimizer.cc:4254-4333) and flag 8"""
    X1 = to_camera(P["rcw1"], P["tcw1"], np.asarray(xw1[:n], F32).reshape(n, 3))
    X2 = to_camera(P["rcw2"], P["tcw2"], np.asarray(xw2[:n], F32).reshape(n, 3))
    val = np.asarray(valid[:n]) != 0
    i2 = np.asarray(idx2[:n], np.int64).copy()
    flag = FLAG_IDX2 if bool(np.any(val & (i2 >= n2))) else 0
    i2[i2 >= n2] = -1
    in2 = i2 >= 0
    pair = val & (P["all_points"] | in2) & ~(X2[:, 2] < 0)
    oc1 = np.zeros(n, np.int64) if octave1 is None else np.asarray(octave1[:n], np.int64).copy()
    oc1[(oc1 < 0) | (oc1 >= len(P["inv1"]))] = 0
    j = np.where(in2, i2, 0)
    k2 = np.zeros((max(n2, 1), 2), F32) if kpts2 is None or n2 == 0 else np.asarray(kpts2, F32).reshape(-1, 2)
    oc2 = np.zeros(max(n2, 1), np.int64) if octave2 is None or n2 == 0 else np.asarray(octave2, np.int64).reshape(-1)
    oc2 = oc2[j].copy()
    oc2[(oc2 < 0) | (oc2 >= len(P["inv2"])) | ~in2] = 0       # a KeyPoint built from a point keeps octave 0
    invz = F32(1.0) / X2[:, 2]                                 # float (:4373-4375)
    o2 = np.where(in2[:, None], k2[j], np.stack([X2[:, 0] * invz, X2[:, 1] * invz], 1)).astype(F64)
    k1 = np.asarray(kpts1[:n], F32).reshape(n, 2)
    return {"P1": X1.astype(F64), "P2": X2.astype(F64), "o1": k1.astype(F64), "o2": o2, "isg1": P["inv1"][oc1].astype(F64),
            "isg2": P["inv2"][oc2].astype(F64), "pair": pair}, flag


def pair_errors(P, f, S, Si):
    """both computeError()s at the estimate S with inverse Si: e12 = obs1 - project1(S.map(P2)), e21 = obs2 - project2(Si.map(P1)); a
    projection is (fx X) / Z + cx"""
    fx1, fy1, cx1, cy1 = (F64(v) for v in P["cam1"])
    fx2, fy2, cx2, cy2 = (F64(v) for v in P["cam2"])
    y = sim3_map(S, [f["P2"][:, 0], f["P2"][:, 1], f["P2"][:, 2]])
    a = [f["o1"][:, 0] - (fx1 * y[0] / y[2] + cx1), f["o1"][:, 1] - (fy1 * y[1] / y[2] + cy1)]
    y = sim3_map(Si, [f["P1"][:, 0], f["P1"][:, 1], f["P1"][:, 2]])
    b = [f["o2"][:, 0] - (fx2 * y[0] / y[2] + cx2), f["o2"][:, 1] - (fy2 * y[1] / y[2] + cy2)]
    return a, b


def huber_delta(th2):
    """`const float deltaHuber = sqrt(th2)` widened; RobustKernelHuber keeps dsqr in a float"""
    delta = F64(F32(np.sqrt(F64(th2))))
    return delta, F64(F32(delta * delta))


def edge_terms(J, e, isg, chi2, robust, delta, dsqr):
    """one edge's 36 terms per row (base_binary_edge.hpp:55-120 with vertex 0 fixed).  J [2][7] arrays, e [2], isg, chi2 arrays."""
    n = len(chi2)
    rho0, rho1 = chi2, np.ones(n, F64)
    if robust:
        sq = np.sqrt(chi2)
        inl = chi2 <= dsqr
        rho0 = np.where(inl, chi2, 2 * sq * delta - dsqr)
        rho1 = np.where(inl, 1.0, delta / sq)
    w = rho1 * isg
    r = [(-(isg * e[0])) * rho1, (-(isg * e[1])) * rho1]
    terms = np.zeros((n, 36), F64)
    col = 0
    for j in range(7):
        for k in range(j, 7):
            terms[:, col] = (J[0][j] * w) * J[0][k] + (J[1][j] * w) * J[1][k]
            col += 1
    for j in range(7):
        terms[:, 28 + j] = J[0][j] * r[0] + J[1][j] * r[1]
    terms[:, 35] = rho0
    return terms


def perturbation(k, fix_scale):
    """the update of estimate k = 1 .. 14: +delta (odd k) or -delta (even k) along dimension (k - 1) // 2; oplusImpl zeroes [6] under fix_scale"""
    u = [F64(0.0)] * 7
    u[(k - 1) // 2] = NUM_DELTA if k & 1 else -NUM_DELTA
    if fix_scale:
        u[6] = F64(0.0)
    return u


# ---------------------------------------------------------------- the optimisation
def optimize_sim3(P, s12_0, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, keep=None, chi2=None):
    """one problem.  s12_0 [8] float64; xw1 / xw2 [N, 3], kpts1 [N, 2] float32; valid [N] uint8; octave1 [N] or None; idx2 [N] int32; kpts2
    [N2, 2], octave2 [N2] or None.  keep / chi2: what the output arrays hold before the call (default ones / zeros).  Returns a dict of
    s12 (float64 [8]), s12_f32, keep (uint8 [N]), chi2 (float64 [N, 2]), trace (float64 [2, 8]), stats (int32 [8]) and ret."""
    with np.errstate(all="ignore"):
        return _optimize_sim3(P, s12_0, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, keep, chi2)


def _optimize_sim3(P, s12_0, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, keep, chi2):
    N = len(valid)
    N2 = 0 if kpts2 is None else len(kpts2)
    n, n2 = min(max(P["n"], 0), N), min(max(P["n2"], 0), N2)
    s12_0 = np.asarray(s12_0, F64)
    out_keep = np.ones(N, np.uint8) if keep is None else np.array(keep, np.uint8)
    out_chi2 = np.zeros((N, 2), F64) if chi2 is None else np.array(chi2, F64).reshape(N, 2)
    trace, stats = np.zeros((2, 8), F64), np.zeros(8, np.int32)
    f, flags = pairs(P, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, n, n2)
    active = f["pair"].copy()
    n_corr = int(active.sum())
    th2 = F64(P["th2"])
    delta, dsqr = huber_delta(P["th2"])
    fix = P["fix_scale"]
    its = [P["iterations"][0] or 5, P["iterations"][1] or 5, P["iterations"][2] or 10]
    max_trials = P["max_trials"] if P["max_trials"] > 0 else 10
    cur = [F64(v) for v in s12_0]
    x = [F64(0.0)] * 7
    over = np.zeros(n, bool)                      # e12 or e21 over th2 in the last pass
    n_bad = n_in = 0
    round1 = s12_0.copy()                         # the estimate after round 1: not an output of the device, for the tests of the stale chi2
    early = n_corr == 0
    rnd = 0
    while rnd < 2 and not early:
        robust = rnd == 0

        def errors(S):
            """a pass: the 36 sums at S, over[] and chi2 of the active pairs"""
            ests = [S] + [sim3_oplus(perturbation(k, fix), S) for k in range(1, 15)]
            invs = [sim3_inverse(e) for e in ests]
            a, b = pair_errors(P, f, ests[0], invs[0])
            c12 = a[0] * (f["isg1"] * a[0]) + a[1] * (f["isg1"] * a[1])
            c21 = b[0] * (f["isg2"] * b[0]) + b[1] * (f["isg2"] * b[1])
            over[active] = ((c12 > th2) | (c21 > th2))[active]
            out_chi2[:n][active] = np.stack([c12, c21], 1)[active]
            J12, J21 = [[None] * 7, [None] * 7], [[None] * 7, [None] * 7]
            for d in range(7):
                pa, pb = pair_errors(P, f, ests[1 + 2 * d], invs[1 + 2 * d])
                ma, mb = pair_errors(P, f, ests[2 + 2 * d], invs[2 + 2 * d])
                for r in range(2):
                    J12[r][d] = NUM_SCALAR * (pa[r] - ma[r])
                    J21[r][d] = NUM_SCALAR * (pb[r] - mb[r])
            return tree_sum2(edge_terms(J12, a, f["isg1"], c12, robust, delta, dsqr), edge_terms(J21, b, f["isg2"], c21, robust, delta, dsqr),
                             active)

        n_its = its[0] if rnd == 0 else (its[2] if n_bad > 0 else its[1])
        lam, ni, nbad_lm = F64(0.0), F64(2.0), 0
        iters = trials = 0
        ended_rejected = False
        current = F64(0.0)
        sums = None                                # the sums of an accepted trial are the sums at the new estimate
        for it in range(n_its):
            iters += 1
            S = sums if sums is not None else errors(cur)
            sums = None
            current = S[35]
            ini = current
            H = [[None] * 7 for _ in range(7)]
            col = 0
            for j in range(7):
                for k in range(j, 7):
                    H[j][k] = H[k][j] = S[col]
                    col += 1
            b = [S[28 + j] for j in range(7)]
            if it == 0:
                maxd = F64(0.0)
                for j in range(7):
                    a = np.abs(H[j][j])
                    maxd = maxd if a < maxd else a
                lam, ni, nbad_lm = 1e-5 * maxd, F64(2.0), 0
            rho, qmax = F64(0.0), 0
            while True:
                trials += 1
                M = [[H[j][k] + lam if j == k else H[j][k] for k in range(7)] for j in range(7)]
                ok, sol = ldlt_solve(M, b)
                if ok:
                    x = sol
                else:
                    flags |= FLAG_SOLVE_FAILED
                if fix:
                    x = list(x)
                    x[6] = F64(0.0)               # oplusImpl writes into the solver's x before computeScale reads it
                trial = sim3_oplus(x, cur)
                if not finite(trial):
                    flags |= FLAG_NONFINITE
                St = errors(trial)
                temp = St[35]
                if not ok:
                    temp = DBL_MAX
                scale = F64(0.0)
                for j in range(7):
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
                    cur = trial
                    sums = St
                    ended_rejected = False
                else:
                    lam = lam * ni
                    ni = ni * 2
                    stats[6] += 1
                    sums = None
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
        if rnd == 0:                              # :4418-4447: the chi2 the last computeActiveErrors left, against (double) th2
            bad = active & over
            n_bad = int(bad.sum())
            out_keep[:n][bad] = 0
            active = active & ~bad
            early = n_corr - n_bad < 10
            left = n_corr - n_bad
            round1 = np.array(cur, F64)
        else:                                     # :4467-4486: every surviving pair again at the final estimate
            a, b = pair_errors(P, f, cur, sim3_inverse(cur))
            c12 = a[0] * (f["isg1"] * a[0]) + a[1] * (f["isg1"] * a[1])
            c21 = b[0] * (f["isg2"] * b[0]) + b[1] * (f["isg2"] * b[1])
            out_chi2[:n][active] = np.stack([c12, c21], 1)[active]
            bad = active & ((c12 > th2) | (c21 > th2))
            out_keep[:n][bad] = 0
            n_in = left = int((active & ~bad).sum())
        stats[3] += 1
        stats[4] += iters
        stats[5] += trials
        trace[rnd, :5] = [iters, trials, lam, current, left]
        rnd += 1
    if early:
        flags |= FLAG_EARLY
    s12 = s12_0.copy() if early else np.array(cur, F64)
    if not finite(s12):
        flags |= FLAG_NONFINITE
    stats[0], stats[1], stats[2], stats[7] = (0 if early else n_in), n_corr, n_bad, flags
    return {"s12": s12, "s12_f32": s12.astype(F32), "keep": out_keep, "chi2": out_chi2, "trace": trace, "stats": stats, "ret": int(stats[0]),
            "round1": round1}


def optimize_sim3_batch(problems, s12_0, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, keep=None, chi2=None):
    """B problems: the arrays of optimize_sim3 with a leading B and a list of B params; returns the outputs stacked"""
    rs = [optimize_sim3(P, s12_0[b], xw1[b], xw2[b], valid[b], kpts1[b], None if octave1 is None else octave1[b], idx2[b],
                        None if kpts2 is None else kpts2[b], None if octave2 is None else octave2[b], None if keep is None else keep[b],
                        None if chi2 is None else chi2[b]) for b, P in enumerate(problems)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in ("s12", "s12_f32", "keep", "chi2", "trace", "stats")}


# ---------------------------------------------------------------- case generators
def _unit(v):
    return v / np.linalg.norm(v)


def sim3_distance(S, truth):
    """(rotation angle in rad, translation distance, |log scale ratio|) between two Sim3 [8]"""
    qa, qb = np.asarray(S[:4], F64), np.asarray(truth[:4], F64)
    qa, qb = qa / np.linalg.norm(qa), qb / np.linalg.norm(qb)
    rel = np.array(quat_mul([-qa[0], -qa[1], -qa[2], qa[3]], list(qb)), F64)
    return (float(2 * np.arctan2(np.linalg.norm(rel[:3]), abs(rel[3]))), float(np.linalg.norm(np.asarray(S[4:7], F64) - np.asarray(truth[4:7], F64))),
            float(abs(np.log(float(S[7]) / float(truth[7])))))


def scene(seed, n, fix_scale=False, mixed=False, N=None, N2=None, noise=0.5, gross=0.2, rot=0.05, trans=0.1, dscale=0.03, nlevels=4, th2=10.0,
          pixel=True, all_points=True, invalid=0.0):
    """two keyframes seeing n matched map points: KF1's points 2 .. 12 m in front of camera 1, the same points through the planted S21 in
    camera 2's frame (scale 1.3, or 1 under fix_scale), world positions through each keyframe's pose, observations with Gaussian pixel
    noise scaled by the level's sigma, a fraction `gross` of KF1's observations displaced by 40 .. 120 px, and a start `rot` rad, `trans`
    and `dscale` off.  mixed: a third of the rows have idx2 = -1 (then cam2 is fx = fy = 1, cx = cy = 0 unless `pixel`, the only setting
    in which the reference's normalised obs2 is consistent).  N / N2: the arrays' capacity."""
    rng = np.random.default_rng(seed)
    N = n if N is None else N
    sig2 = 1.44 ** np.arange(nlevels)
    cam1 = (458.654, 457.296, 367.215, 248.375)
    cam2 = cam1 if (pixel or not mixed) else (1.0, 1.0, 0.0, 0.0)
    q12 = quat_from_rotvec(_unit(rng.standard_normal(3)) * rng.uniform(0.1, 0.4))     # every point stays in front of camera 2
    t12 = rng.standard_normal(3) * 0.5
    s12 = 1.0 if fix_scale else 1.3
    R12 = quat_to_mat(q12)
    z = rng.uniform(2.0, 12.0, n)
    u, v = rng.uniform(40, 700, n), rng.uniform(40, 440, n)
    X1 = np.stack([(u - cam1[2]) / cam1[0] * z, (v - cam1[3]) / cam1[1] * z, z], 1)       # in camera 1
    X2 = ((X1 - t12) @ R12) / s12                                                          # S12^-1: camera 2
    q1w, q2w = quat_from_rotvec(rng.standard_normal(3) * 0.4), quat_from_rotvec(rng.standard_normal(3) * 0.4)
    R1w, R2w = quat_to_mat(q1w).astype(F32), quat_to_mat(q2w).astype(F32)
    t1w, t2w = (rng.standard_normal(3) * 0.7).astype(F32), (rng.standard_normal(3) * 0.7).astype(F32)
    xw1 = np.zeros((N, 3), F32)
    xw2 = np.zeros((N, 3), F32)
    xw1[:n] = ((X1 - t1w.astype(F64)) @ R1w.astype(F64)).astype(F32)
    xw2[:n] = ((X2 - t2w.astype(F64)) @ R2w.astype(F64)).astype(F32)
    oct1, oct2 = rng.integers(0, nlevels, n), rng.integers(0, nlevels, n)
    planted = rng.random(n) < gross
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(40, 120, n)
    k1 = np.stack([u + np.sqrt(sig2)[oct1] * noise * rng.standard_normal(n) + planted * mag * np.cos(ang),
                   v + np.sqrt(sig2)[oct1] * noise * rng.standard_normal(n) + planted * mag * np.sin(ang)], 1)
    sc2 = 1.0 if cam2[0] > 1.0 else 1.0 / 458.0
    k2 = np.stack([cam2[0] * X2[:, 0] / X2[:, 2] + cam2[2] + sc2 * np.sqrt(sig2)[oct2] * noise * rng.standard_normal(n),
                   cam2[1] * X2[:, 1] / X2[:, 2] + cam2[3] + sc2 * np.sqrt(sig2)[oct2] * noise * rng.standard_normal(n)], 1)
    n2 = n
    N2 = n2 if N2 is None else N2
    perm = rng.permutation(n2)                                 # KF2's keypoints in their own order
    idx2 = np.full(N, -1, np.int32)
    idx2[:n] = np.argsort(perm)
    kpts2 = np.zeros((N2, 2), F32)
    octave2 = np.zeros(N2, np.int32)
    kpts2[:n2] = k2[perm].astype(F32)
    octave2[:n2] = oct2[perm]
    if mixed:
        idx2[:n][rng.random(n) < 1.0 / 3.0] = -1
    kpts1 = np.zeros((N, 2), F32)
    octave1 = np.zeros(N, np.int32)
    kpts1[:n] = k1.astype(F32)
    octave1[:n] = oct1
    valid = np.zeros(N, np.uint8)
    valid[:n] = rng.random(n) >= invalid
    dq = quat_from_rotvec(_unit(rng.standard_normal(3)) * rot)
    q0 = np.array(quat_mul(list(dq), list(q12)), F64)
    t0 = t12 + _unit(rng.standard_normal(3)) * trans
    s0 = s12 if fix_scale else s12 * (1.0 + dscale)
    inv = (1.0 / sig2).astype(F32)
    if cam2[0] == 1.0:
        inv2 = (inv.astype(F64) * 458.0 ** 2).astype(F32)      # the same weight in normalised units
    else:
        inv2 = inv
    P = params(R1w, t1w, R2w, t2w, cam1, cam2, inv, inv2, th2, fix_scale, all_points, n, n2)
    pl = np.zeros(N, bool)
    pl[:n] = planted
    return {"P": P, "s12_0": np.concatenate([q0, t0, [s0]]), "xw1": xw1, "xw2": xw2, "valid": valid, "kpts1": kpts1, "octave1": octave1, "idx2": idx2,
            "kpts2": kpts2, "octave2": octave2, "truth": np.concatenate([q12, t12, [s12]]), "planted": pl}


def solve(c, **kw):
    return optimize_sim3(c["P"], c["s12_0"], c["xw1"], c["xw2"], c["valid"], c["kpts1"], c["octave1"], c["idx2"], c["kpts2"], c["octave2"], **kw)


def forced(name):
    """the cases of the paths that random scenes do not take (test_optimize_sim3_ref.py, test_gpu_optimize_sim3.py)"""
    if name == "no_bad":                      # no gross outlier, little noise: nBad == 0, round 2 runs 5 iterations
        c = scene(41, 60, gross=0.0, noise=0.2, th2=50.0)
    elif name == "some_bad":                  # nBad > 0: round 2 runs 10
        c = scene(42, 60, gross=0.2)
    elif name in ("survivors9", "survivors10"):   # 12 pairs of which 3 / 2 are gross: 9 leave through the early exit, 10 go on
        c = scene(43, 12, gross=0.0, noise=0.2)
        k = 3 if name == "survivors9" else 2
        c["kpts1"][:k] += F32(80.0)
        c["planted"][:k] = True
    elif name == "max_trials1":               # qmax == max_trials after the first trial: every round is one iteration of one trial
        c = scene(44, 200)
        c["P"] = dict(c["P"], max_trials=1)
    elif name == "stale":                     # two trials per iteration: round 1 ends on rejected steps, and the stale chi2 removes 65 pairs where the fresh one finds 43
        c = scene(58, 200, rot=0.2, trans=0.4)
        c["P"] = dict(c["P"], max_trials=2)
    elif name == "normalised_pixel":          # idx2 < 0 rows with a pixel-unit camera: the reference's normalised obs2 is off by hundreds of px
        c = scene(46, 120, mixed=True, pixel=True)
    elif name == "normalised_unit":           # ... and with fx = fy = 1, cx = cy = 0, where it is consistent
        c = scene(47, 120, mixed=True, pixel=False)
    elif name == "octave_level0":             # idx2 < 0 rows whose KF2 level would be 3: the KeyPoint built from a point reads level 0
        c = scene(48, 120, mixed=True, pixel=False)
        c["octave2"][:] = 3
    elif name == "behind":                    # z2 < 0: skipped
        c = scene(49, 80)
        c["special"] = 5
        R2, t2 = c["P"]["rcw2"].astype(F64), c["P"]["tcw2"].astype(F64)
        c["xw2"][5] = ((np.array([0.3, -0.2, -4.0]) - t2) @ R2).astype(F32)
    elif name == "z_zero":                    # z2 == 0 passes `z < 0`: a division by zero in the idx2 < 0 observation and in e12
        c = scene(50, 80)
        c["special"] = 5
        c["P"] = dict(c["P"], rcw2=np.eye(3, dtype=F32), tcw2=np.zeros(3, F32))
        c["xw2"][5] = (0.5, 0.25, 0.0)
        c["idx2"][5] = -1
    elif name == "nan":
        c = scene(51, 80)
        c["special"] = 7
        c["xw1"][7, 1] = np.nan
    elif name == "not_all_points":
        c = scene(52, 120, mixed=True, pixel=False, all_points=False)
    elif name == "fix_scale":
        c = scene(53, 100, fix_scale=True)
        c["s12_0"][7] = 1.0625
    elif name == "idx2_range":                # an idx2 at n2 and one far above: flag 8, handled as not in KF2
        c = scene(54, 100)
        c["idx2"][3] = c["P"]["n2"]
        c["idx2"][11] = 1 << 30
    elif name == "invalid":
        c = scene(55, 150, invalid=0.3, mixed=True, pixel=False)
    elif name in TH2_TARGETS:
        c = _th2_case(name)
    else:
        raise KeyError(name)
    return c


TH2_TARGETS = {"th2_below": -np.inf, "th2_equal": None, "th2_above": np.inf}
_th2_found = {}


def pair_chi2(c, S, row):
    """(chi2 of e12, chi2 of e21) of one row at the estimate S, as the final classification computes them"""
    P, n = c["P"], c["P"]["n"]
    with np.errstate(all="ignore"):
        f, _ = pairs(P, c["xw1"], c["xw2"], c["valid"], c["kpts1"], c["octave1"], c["idx2"], c["kpts2"], c["octave2"], n, P["n2"])
        S = [F64(v) for v in S]
        a, b = pair_errors(P, f, S, sim3_inverse(S))
    return (F64(a[0][row] * (f["isg1"][row] * a[0][row]) + a[1][row] * (f["isg1"][row] * a[1][row])),
            F64(b[0][row] * (f["isg2"][row] * b[0][row]) + b[1][row] * (f["isg2"][row] * b[1][row])))


def _th2_case(name):
    """a pair whose e12 chi2 in the FINAL classification is the double next below (double) th2, th2 itself, or the double next above.
    The estimate must not move, so that the chi2 is a function of the inputs alone: row 7 holds a NaN position, every sum is NaN, every
    trial of both rounds is rejected (and round 1's check, on the NaN errors of its last trial, removes nothing), so the final
    classification runs at s12_0 -- which is set to the planted Sim3.  One row's keypoint in KF1 is then moved: u to 1/256 px beside the
    projection, v float by float up to the last value that leaves chi2 below th2; the rest is made up by the translation's x, which
    moves e0 by one ulp of the projection (6e-14 px) at a time -- with e0 below 0.009 px that is a fraction of an ulp of chi2 -- first
    by bisection, then ulp by ulp until the double is hit.  Rows whose v grid leaves more than e0 = 0.009 can make up are passed over."""
    if name not in _th2_found:
        th2 = F64(F32(10.0))
        target = th2 if TH2_TARGETS[name] is None else np.nextafter(th2, TH2_TARGETS[name])
        for row in range(8, 60):
            c = scene(51, 80)
            c["special"], c["th2_row"] = 7, row
            c["xw1"][7, 1] = np.nan
            c["s12_0"] = c["truth"].copy()
            c["planted"][row], c["octave1"][row] = False, 0
            c["kpts1"][row] = (0.0, 0.0)                              # e = 0 - projection
            P, n = c["P"], c["P"]["n"]
            with np.errstate(all="ignore"):
                f, _ = pairs(P, c["xw1"], c["xw2"], c["valid"], c["kpts1"], c["octave1"], c["idx2"], c["kpts2"], c["octave2"], n, P["n2"])
                S = [F64(v) for v in c["s12_0"]]
                a, _ = pair_errors(P, f, S, sim3_inverse(S))
                y2 = sim3_map(S, list(f["P2"][row]))[2]
            c["kpts1"][row] = (F32(-a[0][row] + 1.0 / 256), F32(-a[1][row] + np.sqrt(th2 / f["isg1"][row])))
            while pair_chi2(c, c["s12_0"], row)[0] >= th2 - 1e-9:         # step v down float by float to just below th2
                c["kpts1"][row, 1] = np.nextafter(c["kpts1"][row, 1], F32(-np.inf))

            def at(tx):
                S = c["s12_0"].copy()
                S[4] = tx
                return pair_chi2(c, S, row)[0]
            # e0 = u - proj_u is about +1/256: a smaller tx lowers proj_u and raises e0, up to 0.009 px
            hi = F64(c["s12_0"][4])
            lo = hi - 0.005 * y2 / F64(P["cam1"][0])
            if not (at(lo) > target > at(hi)) or pair_chi2(c, c["s12_0"], row)[1] > 5.0:
                continue
            while np.nextafter(lo, hi) < hi:
                mid = F64(0.5) * (lo + hi)
                if at(mid) >= target:
                    lo = mid
                else:
                    hi = mid
            found = None
            for start, step in ((lo, -np.inf), (hi, np.inf)):
                tx = start
                for _ in range(2000):
                    if at(tx) == target:
                        found = tx
                        break
                    tx = np.nextafter(tx, step)
                if found is not None:
                    break
            if found is None:
                continue
            c["s12_0"][4] = found
            _th2_found[name] = c
            break
        assert name in _th2_found, "no row gives the planted chi2"
    c = _th2_found[name]
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


FORCED = ("no_bad", "some_bad", "survivors9", "survivors10", "max_trials1", "stale", "normalised_pixel", "normalised_unit", "octave_level0",
          "behind", "z_zero", "nan", "not_all_points", "fix_scale", "idx2_range", "invalid", "th2_below", "th2_equal", "th2_above")
