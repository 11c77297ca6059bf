"""numpy float64 restatement of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:4509-4840 over g2o's BlockSolver_7_3 and
Levenberg-Marquardt: one VertexSim3Expmap per keyframe, EdgeSim3 with identity information and numeric Jacobians), the contract of
DESIGN.md 6m: the per-edge arithmetic as array operations over all edges in the order the contract writes them, the per-vertex and
per-block sums sequential in ascending edge order (vectorised ACROSS vertices and blocks), the two global sums in the 256-partial order
of departure (a), the sincos of (d), the log and acos of (e), the 3 x 3 elimination of (f), the dense unpivoted LDLT of (g), and the LM
policy in scalar float64.  Shared by test_essential_graph_ref.py (CPU), test_gpu_essential_graph.py and tools/bench_essential_graph.py;
holds the case generators.  essential_graph_seq.py is the sequential transcription it is compared with."""
import numpy as np

import local_ba_ref as LB
import optimize_sim3_ref as OS
import pose_opt_ref as R6

F32, F64, I64 = np.float32, np.float64, np.int64
MAX_KF, MAX_EDGES, MAX_POINTS, MAX_ITERATIONS = 1024, 16384, 1 << 20, 64
TILE_V, TILE = 4, 28                                   # vertices and rows per tile of the factorisation
DBL_MAX = np.finfo(F64).max
FLAG_ENDED_REJECTED, FLAG_SOLVE_FAILED, FLAG_NONFINITE, FLAG_NO_ITERATION = 1, 2, 4, 16
NUM_DELTA = OS.NUM_DELTA
NUM_SCALAR = OS.NUM_SCALAR
EPS = OS.EPS

# what departures (a)-(g) cost against g2o's own choices, measured by test_essential_graph_ref.py::test_departure_cost on its four graphs:
# the largest absolute difference of any of the 8 numbers of any corrected Sim3; the test allows 8 times as much
DEPARTURE_MAX = 2.3e-7
# how much closer to the planted poses (rotation, translation) the optimisation gets in test_it_optimises, before / after, by fix_scale,
# measured when the test was written; the test asks for a sixteenth
OPTIMISES_GAIN = {True: (19.0, 21.6), False: (20.5, 3.15)}
# the largest |log(exp(x)) - x| over the cases of test_log_branches, measured when it was written; the test allows 8 times as much.  The
# second figure is for a rotation of 1e-5 <= theta < 4.5e-3 rad: there the reference's log() already takes its small-angle forms
# (d > 1 - 1e-5) while its exp does not (theta < 1e-5), and the round trip is off by about theta^2 |t|
LOG_EXP_MAX, LOG_EXP_BAND_MAX = 1.0e-14, 3.1e-5
# the largest distance of log_ and acos_ from libm's, in ulps (test_log_acos_against_libm)
LOG_MAX_ULP, ACOS_MAX_ULP = 1, 1


class Invalid(ValueError):
    """what the entry refuses with RFE_ERR_INVALID"""


def params(iterations=20, max_trials=0, user_lambda_init=1e-16, fix_scale=False):
    return {"iterations": int(iterations), "max_trials": int(max_trials), "user_lambda_init": float(user_lambda_init),
            "fix_scale": bool(fix_scale)}


def tree_sum(v):
    return LB.tree_sum(v)


# ---------------------------------------------------------------- departure (d): sincos on arrays, 6i's operations
def sincos(theta):
    theta = np.asarray(theta, F64)
    k = np.floor(theta * R6.TWO_OVER_PI + 0.5)
    r = (((theta - k * R6.PIO2_1) - k * R6.PIO2_2) - k * R6.PIO2_3) - k * R6.PIO2_4
    r = np.where(np.abs(r) <= R6.R_MAX, r, 0.0)
    q = np.where(np.isfinite(k), k - 4.0 * np.floor(k * 0.25), 0.0)
    z = r * r
    ps = R6.SIN_C[5]
    for c in (R6.SIN_C[4], R6.SIN_C[3], R6.SIN_C[2], R6.SIN_C[1], R6.SIN_C[0]):
        ps = c + z * ps
    s = r + (r * z) * ps
    pc = R6.COS_C[5]
    for c in (R6.COS_C[4], R6.COS_C[3], R6.COS_C[2], R6.COS_C[1], R6.COS_C[0]):
        pc = c + z * pc
    c = (1.0 - 0.5 * z) + (z * z) * pc
    s, c = (np.where(q == 1, c, np.where(q == 2, -s, np.where(q == 3, -c, s))),
            np.where(q == 1, -s, np.where(q == 2, -c, np.where(q == 3, s, c))))
    return np.minimum(np.maximum(s, -1.0), 1.0), np.minimum(np.maximum(c, -1.0), 1.0)


# ---------------------------------------------------------------- departure (e): log and acos
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01, 1.818357216161805012e-01,
      1.531383769920937332e-01, 1.479819860511658591e-01)


def log_(x):
    """fdlibm's e_log without fma and without its short cuts: x = 2^k (1 + f) with sqrt(2)/2 < 1 + f < sqrt(2) (the split on the high
    word as fdlibm has it), s = f / (2 + f), the two interleaved polynomials, the k == 0 and k != 0 sums.  x < 0 and NaN give NaN, 0
    gives -inf, inf gives inf; a subnormal is scaled by 2^54 first."""
    with np.errstate(all="ignore"):
        return _log(np.asarray(x, F64))


def _log(x):
    sub = (x > 0) & (x < 2.2250738585072014e-308)
    xs = np.where(sub, x * 18014398509481984.0, x)
    bits = np.ascontiguousarray(xs).view(I64)
    k = (bits >> 52) - 1023 - np.where(sub, 54, 0)
    m = bits & 0xFFFFFFFFFFFFF
    i = ((m >> 32) + 0x95F64) & 0x100000
    k = k + (i >> 20)
    nb = m | ((0x3FF00000 ^ i) << 32)
    f = np.ascontiguousarray(nb).view(F64) - 1.0
    dk = k.astype(F64)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (LG[1] + w * (LG[3] + w * LG[5]))
    t2 = z * (LG[0] + w * (LG[2] + w * (LG[4] + w * LG[6])))
    R = t2 + t1
    hfsq = (0.5 * f) * f
    r0 = f - (hfsq - s * (hfsq + R))
    rk = dk * LN2_HI - ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f)
    out = np.where(k == 0, r0, rk)
    out = np.where(x == 0, -np.inf, out)
    out = np.where(x == np.inf, np.inf, out)
    return np.where((x < 0) | (x != x), np.nan, out)


PIO2_HI, PIO2_LO, PI = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
PS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
      7.91534994289814532176e-04, 3.47933107596021167570e-05)
QS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)


def _acos_r(z):
    p = z * (PS[0] + z * (PS[1] + z * (PS[2] + z * (PS[3] + z * (PS[4] + z * PS[5])))))
    q = 1.0 + z * (QS[0] + z * (QS[1] + z * (QS[2] + z * QS[3])))
    return p / q


def acos_(x):
    """fdlibm's e_acos without fma: |x| < 0.5 through x^2, x < -0.5 and x > 0.5 through sqrt((1 -+ x) / 2), the latter with the square
    root's low word cleared.  |x| > 1 and NaN give NaN, acos_(1) == 0"""
    with np.errstate(all="ignore"):
        return _acos(np.asarray(x, F64))


def _acos(x):
    # |x| < 0.5
    r = _acos_r(x * x)
    small = PIO2_HI - (x - (PIO2_LO - x * r))
    small = np.where(np.abs(x) < 6.938893903907228e-18, PIO2_HI + PIO2_LO, small)
    # x <= -0.5
    z = (1.0 + x) * 0.5
    s = np.sqrt(z)
    w = _acos_r(z) * s - PIO2_LO
    neg = PI - 2.0 * (s + w)
    # x >= 0.5
    z = (1.0 - x) * 0.5
    s = np.sqrt(z)
    df = np.ascontiguousarray((np.ascontiguousarray(s).view(I64) >> 32) << 32).view(F64)
    c = (z - df * df) / (s + df)
    w = _acos_r(z) * s + c
    pos = 2.0 * (df + w)
    out = np.where(np.abs(x) < 0.5, small, np.where(x < 0, neg, pos))
    out = np.where(x == 1.0, 0.0, np.where(x == -1.0, PI + 2.0 * PIO2_LO, out))
    return np.where(np.abs(x) <= 1.0, out, np.nan)


# ---------------------------------------------------------------- departure (f): W x = t, 3 x 3, partial pivoting
def lu_solve3(W, t):
    """W[r][c], t[r]: arrays.  Column 0: the row with the largest |W[r][0]|, the first maximum, comes first; rows 1 and 2 lose
    l = W[r][0] / W[0][0] times row 0.  Column 1 likewise over rows 1, 2.  Then x2, x1, x0 by back-substitution, each subtraction in
    ascending column order."""
    W = [[np.asarray(W[r][c], F64) for c in range(3)] for r in range(3)]
    t = [np.asarray(v, F64) for v in t]

    def swap(a, b, m):
        for c in range(3):
            W[a][c], W[b][c] = np.where(m, W[b][c], W[a][c]), np.where(m, W[a][c], W[b][c])
        t[a], t[b] = np.where(m, t[b], t[a]), np.where(m, t[a], t[b])

    a0, a1, a2 = np.abs(W[0][0]), np.abs(W[1][0]), np.abs(W[2][0])
    p1 = a1 > a0
    best = np.where(p1, a1, a0)
    p2 = a2 > best
    swap(0, 1, p1 & ~p2)
    swap(0, 2, p2)
    for r in (1, 2):
        l = W[r][0] / W[0][0]
        W[r][1] = W[r][1] - l * W[0][1]
        W[r][2] = W[r][2] - l * W[0][2]
        t[r] = t[r] - l * t[0]
    swap(1, 2, np.abs(W[2][1]) > np.abs(W[1][1]))
    l = W[2][1] / W[1][1]
    W[2][2] = W[2][2] - l * W[1][2]
    t[2] = t[2] - l * t[1]
    x2 = t[2] / W[2][2]
    x1 = (t[1] - W[1][2] * x2) / W[1][1]
    x0 = ((t[0] - W[0][1] * x1) - W[0][2] * x2) / W[0][0]
    return [x0, x1, x2]


# ---------------------------------------------------------------- Sim3 on lists of 8 arrays (qx qy qz qw tx ty tz s)
def quat_to_rot(q):
    """Eigen's toRotationMatrix, not normalised"""
    qx, qy, qz, qw = q
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def sim3_mul(A, B):
    """sim3.h:266-272: r = r1 r2, t = s1 (r1 * t2) + t1, s = s1 s2"""
    r = R6.rotate(A[:4], B[4:7])
    return R6.quat_mul(A[:4], B[:4]) + [A[7] * r[i] + A[4 + i] for i in range(3)] + [A[7] * B[7]]


def sim3_inverse(S):
    return OS.sim3_inverse(S)


def sim3_map(S, X):
    return OS.sim3_map(S, X)


def sim3_log(S):
    """sim3.h:148-230 on arrays: 7 arrays omega, upsilon, sigma.  Both branches are evaluated and selected, which gives each element the
    bits of its own branch"""
    with np.errstate(all="ignore"):
        return _sim3_log(S)


def _sim3_log(S):
    s = np.asarray(S[7], F64)
    sigma = log_(s)
    R = quat_to_rot(S[:4])
    d = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    near = d > 1 - EPS
    ssmall = np.abs(sigma) < EPS
    theta = acos_(d)
    theta2 = theta * theta
    k = np.where(near, 0.5, theta / (2 * np.sqrt(1 - d * d)))
    om = [k * dR[i] for i in range(3)]
    sn, cs = sincos(np.where(near, 0.0, theta))
    # |sigma| < eps
    A0 = np.where(near, 1. / 2., (1 - cs) / theta2)
    B0 = np.where(near, 1. / 6., (theta - sn) / (theta2 * theta))
    # otherwise
    C1 = (s - 1) / sigma
    sigma2 = sigma * sigma
    A1n = ((sigma - 1) * s + 1) / sigma2
    B1n = (((0.5 * sigma2 - sigma) + 1) * s) / (sigma2 * sigma)
    a, b = s * sn, s * cs
    c = theta2 + sigma * sigma
    A1f = (a * sigma + (1 - b) * theta) / (theta * c)
    B1f = ((C1 - ((b - 1) * sigma + a * theta) / c) * 1.) / theta2
    A = np.where(ssmall, A0, np.where(near, A1n, A1f))
    B = np.where(ssmall, B0, np.where(near, B1n, B1f))
    C = np.where(ssmall, 1.0, C1)
    zero = np.zeros_like(d)
    Om = [[zero, -om[2], om[1]], [om[2], zero, -om[0]], [-om[1], om[0], zero]]
    Om2 = [[(Om[r][0] * Om[0][c_] + Om[r][1] * Om[1][c_]) + Om[r][2] * Om[2][c_] for c_ in range(3)] for r in range(3)]
    W = [[(A * Om[r][c_] + B * Om2[r][c_]) + C * (1.0 if r == c_ else 0.0) for c_ in range(3)] for r in range(3)]
    ups = lu_solve3(W, S[4:7])
    return om + ups + [sigma]


def cols(a):
    """[n, 8] -> the list of 8 column arrays"""
    return [a[:, i] for i in range(a.shape[1])]


def perturbations(fix_scale):
    """Sim3(+-delta e_d) for d = 0..6, + first: [14, 8]; under fix_scale update[6] is zeroed first (oplusImpl)"""
    out = np.zeros((14, 8), F64)
    for d in range(7):
        for sgn in range(2):
            u = [F64(0.0)] * 7
            u[d] = NUM_DELTA if sgn == 0 else -NUM_DELTA
            if fix_scale:
                u[6] = F64(0.0)
            q, t, s = OS.sim3_exp(u)
            out[2 * d + sgn] = list(q) + list(t) + [s]
    return out


def edge_error(M, Si, Sj):
    """(M Si) Sj^-1 .log(): lists of arrays -> [7 arrays]"""
    return sim3_log(sim3_mul(sim3_mul(M, Si), sim3_inverse(Sj)))


# ---------------------------------------------------------------- structure
def check(c, P):
    N, E, L = len(c["s_est"]), len(c["edge_i"]), len(c["xw"])
    if not (1 <= N <= MAX_KF and E <= MAX_EDGES and L <= MAX_POINTS):
        raise Invalid("shape")
    if not (0 <= P["iterations"] <= MAX_ITERATIONS and P["max_trials"] >= 0 and np.isfinite(P["user_lambda_init"])):
        raise Invalid("parameter")
    i, j = np.asarray(c["edge_i"], I64), np.asarray(c["edge_j"], I64)
    if np.any((i < 0) | (i >= N) | (j < 0) | (j >= N) | (i == j)):
        raise Invalid("edge index out of range")
    if np.any(np.diff(i * N + j) < 0):
        raise Invalid("edges not ascending")
    r = np.asarray(c["point_ref"], I64)
    if np.any((r < -1) | (r >= N)):
        raise Invalid("point reference out of range")


def tile_fill(free_index, ei, ej, Nf):
    """the tile-level fill of the pattern: (fill [NT, NT] bool, lower triangle with the diagonal, number of tiles marked)"""
    NT = (Nf + TILE_V - 1) // TILE_V
    fill = np.zeros((NT, NT), bool)
    fill[np.arange(NT), np.arange(NT)] = True
    fi, fj = free_index[ei], free_index[ej]
    m = (fi >= 0) & (fj >= 0)
    a, b = np.maximum(fi[m], fj[m]) // TILE_V, np.minimum(fi[m], fj[m]) // TILE_V
    fill[a, b] = True
    for J in range(NT):
        rows = np.nonzero(fill[J + 1:, J])[0] + J + 1
        for n_, I1 in enumerate(rows):
            fill[I1, rows[:n_ + 1]] = True
    return fill, int(np.tril(fill).sum())


def ldlt_dense(S, b):
    """departure (g).  S [n, n] (upper triangle read), b [n].  Entry (i, j) subtracts L_ik (L_jk d_k) for k ascending, then divides by
    d_j -- run right-looking here, which applies the same subtractions to every entry in the same order.  (False, None): a pivot that is
    zero or not finite, an entry of L or of the solution that is not finite.  The solution gets + 0.0 last, which leaves no -0.0"""
    n = len(b)
    if n == 0:
        return True, np.zeros(0, F64)
    A = np.array(S, F64)
    d = np.zeros(n, F64)
    ok = True
    for k in range(n):
        d[k] = A[k, k]
        if not np.isfinite(d[k]) or d[k] == 0.0:
            ok = False
        A[k, k + 1:] = A[k, k + 1:] / d[k]
        if not np.all(np.isfinite(A[k, k + 1:])):
            ok = False
        if k + 1 < n:
            w = A[k, k + 1:] * d[k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - w[:, None] * A[k, k + 1:][None, :]
    if not ok:
        return False, None
    y = np.array(b, F64)
    for k in range(n):
        y[k + 1:] = y[k + 1:] - A[k, k + 1:] * y[k]
    y = y / d
    for k in range(n - 1, -1, -1):
        y[:k] = y[:k] - A[:k, k] * y[k]
    y = y + 0.0
    if not np.all(np.isfinite(y)):
        return False, None
    return True, y


# ---------------------------------------------------------------- the optimisation
def essential_graph(c, P=None):
    """c: a case dict (s_est [N,8], s_meas [N,8], fixed [N], edge_i / edge_j / edge_from_est [E], xw [L,3], point_ref [L]).  Returns
    siw [N,8], tiw_f32 [N,7], swi [N,8], xw_out [L,3], chi2 [E], trace [iterations,4], stats [8], ret"""
    P = params() if P is None else P
    with np.errstate(all="ignore"):
        return _essential_graph(c, P)


def _essential_graph(c, P):
    check(c, P)
    est0 = np.asarray(c["s_est"], F64).reshape(-1, 8)
    meas = np.asarray(c["s_meas"], F64).reshape(-1, 8)
    N = len(est0)
    fixed = np.asarray(c["fixed"]).astype(bool)
    ei, ej, src = np.asarray(c["edge_i"], I64), np.asarray(c["edge_j"], I64), np.asarray(c["edge_from_est"]).astype(bool)
    E = len(ei)
    fix_scale = P["fix_scale"]
    free = np.nonzero(~fixed)[0]
    Nf = len(free)
    free_index = np.full(N, -1, I64)
    free_index[free] = np.arange(Nf)
    n7 = 7 * Nf
    # measurements Sji = Sjw Swi
    Ti = np.where(src[:, None], est0[ei], meas[ei])
    Tj = np.where(src[:, None], est0[ej], meas[ej])
    M = sim3_mul(cols(Tj), sim3_inverse(cols(Ti))) if E else [np.zeros(0, F64)] * 8
    pert = perturbations(fix_scale)
    # incidences (vertex, edge, side), free vertices only, ascending edge inside a vertex
    iv = np.concatenate([free_index[ei], free_index[ej]])
    ie = np.concatenate([np.arange(E), np.arange(E)])
    iside = np.concatenate([np.zeros(E, I64), np.ones(E, I64)])
    keep = iv >= 0
    iv, ie, iside = iv[keep], ie[keep], iside[keep]
    order = np.lexsort((ie, iv))
    iv, ie, iside = iv[order], ie[order], iside[order]
    start = np.searchsorted(iv, np.arange(Nf + 1))
    irank = np.arange(len(iv)) - start[iv] if len(iv) else np.zeros(0, I64)
    # off-diagonal blocks: the edges with both ends free, grouped by the unordered pair
    both = np.nonzero((free_index[ei] >= 0) & (free_index[ej] >= 0))[0]
    fa, fb = np.minimum(free_index[ei[both]], free_index[ej[both]]), np.maximum(free_index[ei[both]], free_index[ej[both]])
    pair_key = fa * (Nf + 1) + fb
    _, pair_id = np.unique(pair_key, return_inverse=True) if len(both) else (None, np.zeros(0, I64))
    pair_rank = np.zeros(len(both), I64)
    seen = {}
    for n_, p in enumerate(pair_id):
        pair_rank[n_] = seen.get(p, 0)
        seen[p] = pair_rank[n_] + 1
    n_pairs = len(seen)
    pair_a, pair_b = np.zeros(n_pairs, I64), np.zeros(n_pairs, I64)
    pair_a[pair_id], pair_b[pair_id] = fa, fb
    fill, tiles = tile_fill(free_index, ei, ej, Nf)
    NT = fill.shape[0]

    def errors_at(est):
        e = edge_error(M, cols(est[ei]), cols(est[ej]))
        chi2 = e[0] * e[0]
        for k in range(1, 7):
            chi2 = chi2 + e[k] * e[k]
        return e, chi2

    def jacobian(est, which):
        """[7 rows][7 columns] arrays: column d = (e(+delta) - e(-delta)) scalar through oplus on vertex `which`"""
        J = [[None] * 7 for _ in range(7)]
        base_i, base_j = cols(est[ei]), cols(est[ej])
        for d in range(7):
            ee = []
            for sgn in range(2):
                p = [np.full(E, v) for v in pert[2 * d + sgn]]
                if which == 0:
                    ee.append(edge_error(M, sim3_mul(p, base_i), base_j))
                else:
                    ee.append(edge_error(M, base_i, sim3_mul(p, base_j)))
            for k in range(7):
                J[k][d] = NUM_SCALAR * (ee[0][k] - ee[1][k])
        return J

    def dot7(X, a, Y, b):
        v = X[0][a] * Y[0][b]
        for k in range(1, 7):
            v = v + X[k][a] * Y[k][b]
        return v

    up7 = [(a, b) for a in range(7) for b in range(a, 7)]
    est = est0.copy()
    max_trials = P["max_trials"] if P["max_trials"] > 0 else 10
    trace, stats = np.zeros((P["iterations"], 4), F64), np.zeros(8, np.int32)
    flags = 0
    x = np.zeros(n7, F64)
    lam, ni, nbad = F64(0.0), F64(2.0), 0
    iters = trials = rejected = failed = 0
    ended_rejected = False
    chi2_stored = np.zeros(E, F64)
    for it in range(P["iterations"]):
        iters += 1
        e, chi2_stored = errors_at(est)
        current = tree_sum(chi2_stored)
        ini = current
        A, B = jacobian(est, 0), jacobian(est, 1)
        ne = [-e[k] for k in range(7)]
        con = np.zeros((E, 2, 35), F64)                        # per side: H's upper triangle (28) | b (7)
        for s_, X in enumerate((A, B)):
            for n_, (a, b) in enumerate(up7):
                con[:, s_, n_] = dot7(X, a, X, b)
            for a in range(7):
                v = X[0][a] * ne[0]
                for k in range(1, 7):
                    v = v + X[k][a] * ne[k]
                con[:, s_, 28 + a] = v
        Hij = np.zeros((E, 7, 7), F64)
        for a in range(7):
            for b in range(7):
                Hij[:, a, b] = dot7(A, a, B, b)
        vs = LB.seq_sum_groups(con[ie, iside], iv, irank, Nf)
        Hm = np.zeros((n7, n7), F64)
        for n_, (a, b) in enumerate(up7):
            Hm[7 * np.arange(Nf) + a, 7 * np.arange(Nf) + b] = vs[:, n_]
        bvec = vs[:, 28:].reshape(-1).copy()
        if len(both):
            # the block of the pair (fa < fb), rows of fa: Hij as it stands when i is fa, its transpose otherwise
            flip = free_index[ei[both]] > free_index[ej[both]]
            blk = np.where(flip[:, None, None], Hij[both].transpose(0, 2, 1), Hij[both]).reshape(-1, 49)
            ps = LB.seq_sum_groups(blk, pair_id, pair_rank, n_pairs).reshape(-1, 7, 7)
            for a in range(7):
                for b in range(7):
                    Hm[7 * pair_a + a, 7 * pair_b + b] = ps[:, a, b]
        if it == 0:
            if P["user_lambda_init"] > 0:
                lam = F64(P["user_lambda_init"])
            else:
                dg = np.concatenate([np.abs(np.diag(Hm)), [0.0]])
                dg = dg[~np.isnan(dg)]
                lam = 1e-5 * F64(dg.max())
            ni, nbad = F64(2.0), 0
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            Sm = Hm.copy()
            Sm[np.arange(n7), np.arange(n7)] = Sm[np.arange(n7), np.arange(n7)] + lam
            ok, sol = ldlt_dense(Sm, bvec)
            if ok:
                x = sol
            else:
                failed += 1
                flags |= FLAG_SOLVE_FAILED
            if fix_scale:
                x[6::7] = 0.0
            new = est.copy()
            for f, v in enumerate(free):
                new[v] = OS.sim3_oplus([F64(u) for u in x[7 * f:7 * f + 7]], [F64(u) for u in est[v]])
            if not np.all(np.isfinite(new)):
                flags |= FLAG_NONFINITE
            sterm = x * (lam * x + bvec)
            _, chi2_stored = errors_at(new)
            temp = tree_sum(chi2_stored)
            if not ok:
                temp = F64(DBL_MAX)
            scale = tree_sum(sterm) + 1e-3
            rho = (current - temp) / scale
            if rho > 0 and np.isfinite(temp):
                v_ = 2 * rho - 1
                alpha = 1.0 - (v_ * v_) * v_
                alpha = F64(2.0 / 3.0) if F64(2.0 / 3.0) < alpha else alpha
                lam = lam * (alpha if F64(1.0 / 3.0) < alpha else F64(1.0 / 3.0))
                ni = F64(2.0)
                current = temp
                est = new
                ended_rejected = False
            else:
                lam = lam * ni
                ni = ni * 2
                rejected += 1
                ended_rejected = True
            qmax += 1
            if not (rho < 0 and qmax < max_trials):
                break
        trace[it] = [qmax, lam, current, 0.0]
        if qmax == max_trials or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            break
    if iters == 0:
        flags |= FLAG_NO_ITERATION
    if ended_rejected:
        flags |= FLAG_ENDED_REJECTED
    # the closing computeActiveErrors(): the stored chi2 is that of the final estimate
    _, chi2_stored = errors_at(est)
    if not np.all(np.isfinite(est)):
        flags |= FLAG_NONFINITE
    swi = np.stack(sim3_inverse(cols(est)), 1)
    tiw = np.concatenate([est[:, :4].astype(F32), est[:, 4:7].astype(F32) / est[:, 7:8].astype(F32)], 1)
    xw = np.asarray(c["xw"], F32).reshape(-1, 3)
    ref = np.asarray(c["point_ref"], I64)
    r = np.maximum(ref, 0)
    X = [xw[:, i].astype(F64) for i in range(3)]
    Y = sim3_map(cols(swi[r]), sim3_map(cols(est0[r]), X)) if len(xw) else X
    xw_out = np.where((ref >= 0)[:, None], np.stack(Y, 1).astype(F32), xw) if len(xw) else xw.copy()
    stats[:] = [iters, trials, rejected, failed, flags, Nf, tiles, NT * (NT + 1) // 2]
    return {"siw": est, "tiw_f32": tiw.astype(F32), "swi": swi, "xw_out": xw_out.astype(F32), "chi2": np.asarray(chi2_stored, F64).copy(),
            "trace": trace, "stats": stats, "ret": iters}


# ---------------------------------------------------------------- case generators
def _sim3(rng, rot, trans, dscale):
    q = R6.quat_from_rotvec(rng.normal(0, rot, 3))
    return np.array(list(q) + list(rng.normal(0, trans, 3)) + [np.exp(rng.normal(0, dscale))], F64)


def _compose(A, B):
    return np.array([F64(v) for v in sim3_mul([F64(v) for v in A], [F64(v) for v in B])], F64)


def graph(seed, N, kind="chain", band=0, loops=0, fixed=0, drift=0.01, dscale=0.0, corrected=0, L=0, dup=0, shuffle=False, radius=5.0,
          walk=True, edges_total=None, arc=2 * np.pi):
    """a planted pose graph: N keyframes on an arc (`arc` rad, a full ring by default) of `radius` m; truth Siw; the estimate carries a drift that grows along the chain
    (a random walk of `drift` rad / m per step, `dscale` in log scale), the last `corrected` keyframes hold the truth in s_est and the
    drifted pose in s_meas (CorrectedSim3 / NonCorrectedSim3).  Edges: kind chain (i, i + 1), star (fixed, every other) or arrowhead
    (chain plus the last 5 to the first 5); `band` adds (i, i + 2 .. i + band); `loops` adds from-est edges between the last `loops`
    and the first `loops` keyframes; `dup` repeats that many edges (edges_total: as many as reach that count).  walk=False: the same drift step
    every keyframe instead of a random walk.  L points around the ring.  shuffle: the keyframe
    indices are permuted.  `fixed`: the index that is fixed, None for no fixed vertex"""
    rng = np.random.default_rng(seed)
    truth = np.zeros((N, 8), F64)
    for i in range(N):
        a = arc * i / max(N, 8)
        q = R6.quat_from_rotvec(np.array([0.0, a, 0.0]) + rng.normal(0, 0.02, 3))
        Rm = np.array(R6.quat_to_mat(q), F64)
        centre = np.array([radius * np.sin(a), 0.1 * rng.normal(), radius * np.cos(a)])
        truth[i] = list(q) + list(-Rm @ centre) + [1.0]
    drifted = truth.copy()
    step = _sim3(rng, drift, drift, dscale)
    for i in range(1, N):                                     # odometry: the true relative pose, then this step's drift in the camera frame
        rel = _compose(truth[i], np.array(OS.sim3_inverse([F64(v) for v in truth[i - 1]]), F64))
        drifted[i] = _compose(_sim3(rng, drift, drift, dscale) if walk else step, _compose(rel, drifted[i - 1]))
    s_est, s_meas = drifted.copy(), drifted.copy()
    if corrected:
        s_est[N - corrected:] = truth[N - corrected:]
    edges = []
    if kind == "star":
        hub = fixed if fixed is not None else 0
        edges += [(hub, j, 0) for j in range(N) if j != hub]
    else:
        edges += [(i, i + 1, 0) for i in range(N - 1)]
        if kind == "arrowhead":
            edges += [(N - 1 - a, b, 0) for a in range(min(5, N // 2)) for b in range(min(5, N // 2))]
    for w in range(2, band + 1):
        edges += [(i, i + w, 0) for i in range(N - w)]
    edges += [(N - 1 - a, b, 1) for a in range(loops) for b in range(loops) if N - 1 - a != b]
    if edges_total is not None:
        dup = edges_total - len(edges)
    edges += [edges[int(k)] for k in rng.integers(0, max(len(edges), 1), dup)] if edges else []
    perm = rng.permutation(N) if shuffle else np.arange(N)
    inv = np.argsort(perm)                                    # old index -> new index
    edges = sorted((int(inv[i]), int(inv[j]), f) for i, j, f in edges)
    fx = np.zeros(N, np.uint8)
    if fixed is not None:
        fx[inv[fixed]] = 1
    ref = rng.integers(0, N, L).astype(np.int32)
    xw = rng.normal(0, radius, (L, 3)).astype(F32)
    if L > 3:
        ref[1] = -1
    e = np.array(edges, I64).reshape(-1, 3)
    return {"s_est": s_est[perm], "s_meas": s_meas[perm], "fixed": fx, "edge_i": e[:, 0].astype(np.int32), "edge_j": e[:, 1].astype(np.int32),
            "edge_from_est": e[:, 2].astype(np.uint8), "xw": xw, "point_ref": ref, "truth": truth[perm]}


def optimises_scene(fix_scale):
    """40 keyframes on a gentle arc, the same odometry drift every step, the last three corrected and tied to the first three"""
    return graph(3, 40, drift=0.004, dscale=0.0 if fix_scale else 0.003, walk=False, L=20, arc=0.05, loops=3, corrected=3)


def pose_error(S, truth):
    """(largest rotation angle, largest camera-centre distance) between Siw and the planted poses, up to the scale in S"""
    rot = trn = 0.0
    for a, b in zip(S, truth):
        qa, qb = a[:4] / np.linalg.norm(a[:4]), b[:4] / np.linalg.norm(b[:4])
        rot = max(rot, 2 * np.arccos(min(1.0, abs(float(qa @ qb)))))
        ca = -np.array(R6.quat_to_mat(list(qa))).T @ (a[4:7] / a[7])
        cb = -np.array(R6.quat_to_mat(list(qb))).T @ (b[4:7] / b[7])
        trn = max(trn, float(np.linalg.norm(ca - cb)))
    return rot, trn


def forced(name):
    """(case, params) for the forced paths"""
    c = graph(11, 12, kind="chain", loops=2, corrected=2, L=9, drift=0.02)
    P = params()
    if name == "ended_rejected":                              # at convergence the noise of the numeric Jacobian ends the run: two trials, both rejected
        P = params(iterations=20, max_trials=2, fix_scale=True)
    elif name == "rho_zero":                                  # every error is exactly zero: H = 0, b = 0, x = 0, rho = 0 / 1e-3
        c = graph(13, 6, kind="chain", drift=0.0, L=3)
        c["s_est"][:] = [0, 0, 0, 1, 0, 0, 0, 1]
        c["s_meas"][:] = c["s_est"]
    elif name == "failed_solve":
        c["s_est"][5, 4] = np.nan
    elif name == "iterations0":
        P = params(iterations=0)
    elif name == "all_fixed":
        c["fixed"][:] = 1
    elif name == "no_fixed":
        c["fixed"][:] = 0
    elif name == "no_edges":
        for k in ("edge_i", "edge_j", "edge_from_est"):
            c[k] = c[k][:0]
    elif name == "duplicates":
        c = graph(14, 9, kind="chain", loops=2, corrected=2, dup=6, L=5)
    elif name == "auto_lambda":
        P = params(user_lambda_init=0.0)
    else:
        raise KeyError(name)
    return c, P


FORCED = ("ended_rejected", "rho_zero", "failed_solve", "iterations0", "all_fixed", "no_fixed", "no_edges", "duplicates", "auto_lambda")


def check_forced(name, r):
    """what each forced path must show in the restatement's result"""
    st = [int(v) for v in r["stats"]]
    iters, trials, rejected, failed, flags = st[:5]
    if name == "ended_rejected":
        assert flags & FLAG_ENDED_REJECTED and rejected >= 1
    elif name == "rho_zero":
        assert (iters, trials, rejected) == (1, 1, 1) and r["trace"][0, 2] == 0.0
    elif name == "failed_solve":
        assert failed == trials and flags & FLAG_SOLVE_FAILED and flags & FLAG_NONFINITE
    elif name == "iterations0":
        assert iters == 0 and flags & FLAG_NO_ITERATION
    elif name == "all_fixed":
        assert st[5] == 0 and st[6] == 0
    elif name == "no_fixed":
        assert st[5] == 12
    elif name == "no_edges":
        assert len(r["chi2"]) == 0 and r["trace"][0, 2] == 0.0
    elif name == "duplicates":
        assert iters >= 1 and failed == 0
    elif name == "auto_lambda":
        assert r["trace"][0, 1] > 1e-8
