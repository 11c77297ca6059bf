"""numpy float64 restatement of Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1857-2150 over g2o's BlockSolver_6_3 and
Levenberg-Marquardt), the contract of DESIGN.md 6l: the per-edge arithmetic as array operations over all edges in the order the contract
writes them, the per-vertex and per-Schur-block sums sequential in ascending edge / point order (vectorised ACROSS vertices and blocks),
the three global sums in the 256-partial order of departure (a), the sincos of departure (b), the dense unpivoted LDLT of departure (c),
the cofactor inverse of departure (d), and the LM policy in scalar float64.  Shared by test_local_ba_ref.py (CPU), test_gpu_local_ba.py,
test_gpu_local_ba_dropin.py and tools/bench_local_ba.py; holds the case generators."""
import numpy as np

import pose_opt_ref as R6

F32, F64 = np.float32, np.float64
MAX_LEVELS = 16
MAX_FREE, MAX_KF, MAX_POINTS, MAX_EDGES, MAX_ITERATIONS = 64, 256, 16384, 131072, 64
DBL_MAX = np.finfo(F64).max
FLAG_ENDED_REJECTED, FLAG_SOLVE_FAILED, FLAG_NONFINITE, FLAG_STOPPED, FLAG_NO_ITERATION = 1, 2, 4, 8, 16
TH2_MONO, TH2_STEREO = 5.991, 7.815


# what departures (a), (c), (d) cost against g2o's own choices, measured by test_local_ba_ref.py::test_departure_cost on its cases: the
# largest absolute difference of any pose number and of any point coordinate; the test allows 8 times as much
DEPARTURE_MAX = (1.3e-12, 4.3e-11)
# how much closer to the planted poses (rotation, translation) and points the optimisation gets in test_it_optimises, before / after,
# measured when the test was written; the test asks for a sixteenth
OPTIMISES_GAIN = (22.5, 10.3, 4.05)


class Invalid(ValueError):
    """what the entry refuses with RFE_ERR_INVALID"""


def params(iterations=10, max_trials=0, user_lambda_init=0.0, th2_mono=TH2_MONO, th2_stereo=TH2_STEREO, stop=False):
    return {"iterations": int(iterations), "max_trials": int(max_trials), "user_lambda_init": float(user_lambda_init),
            "th2_mono": float(th2_mono), "th2_stereo": float(th2_stereo), "stop": bool(stop)}


def huber(th2):
    """`const float thHuberMono = sqrt(5.991)`; RobustKernelHuber keeps dsqr in a float member"""
    delta = F64(F32(np.sqrt(F64(th2))))
    return delta, F64(F32(delta * delta))


def tree_sum(v):
    """departure (a) over a vector"""
    v = np.asarray(v, F64).reshape(-1, 1)
    return R6.tree_sum(v, np.ones(len(v), bool))[0] if len(v) else F64(0.0)


def check(c, P):
    """the refusals; c: a case dict"""
    Pn, Fn, L, E, Nf = c["P"], c["F"], len(c["xw"]), len(c["edge_point"]), len(c["kpts"])
    K = Pn + Fn
    if not (0 <= Pn <= MAX_FREE and Fn >= 0 and 1 <= K <= MAX_KF and L <= MAX_POINTS and E <= MAX_EDGES):
        raise Invalid("shape")
    if not (0 <= P["iterations"] <= MAX_ITERATIONS and P["max_trials"] >= 0):
        raise Invalid("iterations")
    if not np.all(np.isfinite([P["user_lambda_init"], P["th2_mono"], P["th2_stereo"]])):
        raise Invalid("non-finite parameter")
    nl, off = np.asarray(c["kf_nlevels"]), np.asarray(c["kf_feat_off"], np.int64)
    if np.any((nl < 1) | (nl > MAX_LEVELS)) or np.any(off < 0) or np.any(off > Nf) or np.any(np.diff(off) < 0):
        raise Invalid("keyframe table")
    p, k, f = (np.asarray(c[n], np.int64) for n in ("edge_point", "edge_kf", "edge_feat"))
    if np.any((p < 0) | (p >= L) | (k < 0) | (k >= K)):
        raise Invalid("edge index out of range")
    if np.any((f < 0) | (f >= off[k + 1] - off[k])):
        raise Invalid("edge index out of range")
    key = p * (K + 1) + k
    if np.any(np.diff(key) <= 0):
        raise Invalid("edges not strictly ascending")


# ---------------------------------------------------------------- structure
class Structure:
    """per-point edge ranges, per-pose ascending edge lists, per Schur block (i1 <= i2) the ascending (e1, e2) pairs"""

    def __init__(self, c):
        self.P, self.K = c["P"], c["P"] + c["F"]
        self.L, self.E = len(c["xw"]), len(c["edge_point"])
        self.ep, self.ek = np.asarray(c["edge_point"], np.int64), np.asarray(c["edge_kf"], np.int64)
        self.pt_start = np.searchsorted(self.ep, np.arange(self.L + 1))
        self.free = self.ek < self.P
        # rank of every edge inside its point, and inside its pose's list
        self.pt_rank = np.arange(self.E) - self.pt_start[self.ep] if self.E else np.zeros(0, np.int64)
        self.pose_list = [np.nonzero(self.ek == i)[0] for i in range(self.P)]
        P = self.P
        self.blocks = [(i1, i2) for i1 in range(P) for i2 in range(i1, P)]
        bid = {b: n for n, b in enumerate(self.blocks)}
        # pairs: for every point, every (e1, e2) of its free edges with kf(e1) <= kf(e2); ascending e1 inside a block = ascending point
        fe = np.nonzero(self.free)[0]
        pairs = [[] for _ in self.blocks]
        if len(fe):
            cnt = np.bincount(self.ep[fe], minlength=self.L)
            start = np.concatenate([[0], np.cumsum(cnt)])
            for p in np.nonzero(cnt)[0]:
                es = fe[start[p]:start[p + 1]]
                for a in range(len(es)):
                    for b in range(a, len(es)):
                        pairs[bid[(int(self.ek[es[a]]), int(self.ek[es[b]]))]].append((es[a], es[b]))
        self.pairs = [np.asarray(p, np.int64).reshape(-1, 2) for p in pairs]
        self.n_pairs = int(sum(len(p) for p in self.pairs))
        self.n_free = int(self.free.sum())


def seq_sum_groups(values, group, rank, G):
    """values [n, C]; group [n] in 0..G-1, rank [n] the position inside the group.  Every group's rows added in ascending rank from +0.0,
    vectorised across groups"""
    out = np.zeros((G, values.shape[1]), F64)
    if len(group) == 0:
        return out
    for r in range(int(rank.max()) + 1):
        m = rank == r
        out[group[m]] = out[group[m]] + values[m]
    return out


# ---------------------------------------------------------------- edges
def edge_inputs(c):
    K = c["P"] + c["F"]
    ek, ef = np.asarray(c["edge_kf"], np.int64), np.asarray(c["edge_feat"], np.int64)
    E = len(ek)
    f = np.asarray(c["kf_feat_off"], np.int64)[ek] + ef if E else np.zeros(0, np.int64)
    kp = np.asarray(c["kpts"], F32).reshape(-1, 2)
    ur = np.full(len(kp), -1.0, F32) if c.get("uright") is None else np.asarray(c["uright"], F32)
    octv = np.zeros(len(kp), np.int64) if c.get("octave") is None else np.asarray(c["octave"], np.int64)
    o = octv[f].copy()
    nl = np.asarray(c["kf_nlevels"], np.int64)[ek]
    o[(o < 0) | (o >= nl)] = 0
    cam = np.asarray(c["kf_cam"], F32).reshape(K, 5).astype(F64)
    sig = np.asarray(c["kf_sigma2"], F32).reshape(K, MAX_LEVELS)
    urf = ur[f]
    return {"u": kp[f, 0].astype(F64), "v": kp[f, 1].astype(F64), "ur": urf.astype(F64), "stereo": ~(urf < 0), "isg": sig[ek, o].astype(F64),
            "fx": cam[ek, 0], "fy": cam[ek, 1], "cx": cam[ek, 2], "cy": cam[ek, 3], "bf": cam[ek, 4]}


def edge_error(I, hub, q, t, X):
    """q [E, 4] columns, t [E, 3], X [E, 3] per edge.  Returns (x, y, z), e [3 arrays], chi2, rho0, rho1"""
    qs = [q[:, 0], q[:, 1], q[:, 2], q[:, 3]]
    Xc = R6.rotate(qs, [X[:, 0], X[:, 1], X[:, 2]])
    x, y, z = Xc[0] + t[:, 0], Xc[1] + t[:, 1], Xc[2] + t[:, 2]
    st, isg = I["stereo"], I["isg"]
    em0 = I["u"] - (I["fx"] * x / z + I["cx"])
    em1 = I["v"] - (I["fy"] * y / z + I["cy"])
    invzf = (1.0 / z).astype(F32).astype(F64)
    pu = x * invzf * I["fx"] + I["cx"]
    pv = y * invzf * I["fy"] + I["cy"]
    pr = pu - I["bf"] * invzf
    e = [np.where(st, I["u"] - pu, em0), np.where(st, I["v"] - pv, em1), np.where(st, I["ur"] - pr, 0.0)]
    chi2 = e[0] * (isg * e[0]) + e[1] * (isg * e[1])
    chi2 = np.where(st, chi2 + e[2] * (isg * e[2]), chi2)
    delta, dsqr = np.where(st, hub[2], hub[0]), np.where(st, hub[3], hub[1])
    sq = np.sqrt(chi2)
    inl = chi2 <= dsqr
    rho0 = np.where(inl, chi2, 2 * sq * delta - dsqr)
    rho1 = np.where(inl, 1.0, delta / sq)
    return (x, y, z), e, chi2, rho0, rho1


def edge_linearise(I, hub, q, t, X):
    """chi2, rho0 and lin [E, 54]: 0-5 Hll's upper triangle, 6-8 bl, 9-29 Hpp's upper triangle, 30-35 bp, 36-53 the 6 x 3 block
    (Xj^T wOmega) Xi, row-major"""
    (x, y, z), e, chi2, rho0, rho1 = edge_error(I, hub, q, t, X)
    n = len(x)
    st, isg, fx, fy, bf = I["stereo"], I["isg"], I["fx"], I["fy"], I["bf"]
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    Rm = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
    zero, one = np.zeros(n, F64), np.ones(n, F64)
    z_2 = z * z
    # stereo: types_six_dof_expmap.cpp:242-273 as written
    Xis = [[-fx * Rm[0][c] / z + fx * x * Rm[2][c] / z_2 for c in range(3)], [-fy * Rm[1][c] / z + fy * y * Rm[2][c] / z_2 for c in range(3)]]
    Xis.append([Xis[0][c] - bf * Rm[2][c] / z_2 for c in range(3)])
    Xjs = [[x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx, -1. / z * fx, zero, x / z_2 * fx],
           [(1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy, zero, -1. / z * fy, y / z_2 * fy]]
    Xjs.append([Xjs[0][0] - bf * y / z_2, Xjs[0][1] + bf * x / z_2, Xjs[0][2], Xjs[0][3], zero, Xjs[0][5] - bf / z_2])
    # mono: (-projectJac) R and (-projectJac) SE3deriv, every entry the full three-term sum
    nJ = [[-(fx / z), -zero, -(-fx * x / (z * z))], [-zero, -(fy / z), -(-fy * y / (z * z))]]
    Sd = [[zero, z, -y, one, zero, zero], [-z, zero, x, zero, one, zero], [y, -x, zero, zero, zero, one]]
    Xim = [[(nJ[r][0] * Rm[0][c] + nJ[r][1] * Rm[1][c]) + nJ[r][2] * Rm[2][c] for c in range(3)] for r in range(2)]
    Xjm = [[(nJ[r][0] * Sd[0][c] + nJ[r][1] * Sd[1][c]) + nJ[r][2] * Sd[2][c] for c in range(6)] for r in range(2)]
    Xi = [[np.where(st, Xis[r][c], Xim[r][c]) for c in range(3)] for r in range(2)] + [Xis[2]]
    Xj = [[np.where(st, Xjs[r][c], Xjm[r][c]) for c in range(6)] for r in range(2)] + [Xjs[2]]
    w = rho1 * isg
    omr = [(-(isg * e[r])) * rho1 for r in range(3)]
    lin = np.zeros((n, 54), F64)
    col = 0

    def quad(A, a, B, b):
        h = (A[0][a] * w) * B[0][b] + (A[1][a] * w) * B[1][b]
        return np.where(st, h + (A[2][a] * w) * B[2][b], h)

    def grad(A, a):
        g = A[0][a] * omr[0] + A[1][a] * omr[1]
        return np.where(st, g + A[2][a] * omr[2], g)

    for a in range(3):
        for b in range(a, 3):
            lin[:, col] = quad(Xi, a, Xi, b)
            col += 1
    for a in range(3):
        lin[:, col] = grad(Xi, a)
        col += 1
    for a in range(6):
        for b in range(a, 6):
            lin[:, col] = quad(Xj, a, Xj, b)
            col += 1
    for a in range(6):
        lin[:, col] = grad(Xj, a)
        col += 1
    for a in range(6):
        for b in range(3):
            lin[:, col] = 0.0 + quad(Xj, a, Xi, b)
            col += 1
    return chi2, rho0, lin


# ---------------------------------------------------------------- departure (d): 3 x 3 inverse by cofactors, vectorised over points
def inverse3(m):
    """m[r][c]: arrays.  Returns Dinv[r][c]"""
    c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1]
    c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2]
    c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0]
    c10 = m[0][2] * m[2][1] - m[0][1] * m[2][2]
    c11 = m[0][0] * m[2][2] - m[0][2] * m[2][0]
    c12 = m[0][1] * m[2][0] - m[0][0] * m[2][1]
    c20 = m[0][1] * m[1][2] - m[0][2] * m[1][1]
    c21 = m[0][2] * m[1][0] - m[0][0] * m[1][2]
    c22 = m[0][0] * m[1][1] - m[0][1] * m[1][0]
    det = (m[0][0] * c00 + m[1][0] * c10) + m[2][0] * c20
    i = 1.0 / det
    return [[c00 * i, c10 * i, c20 * i], [c01 * i, c11 * i, c21 * i], [c02 * i, c12 * i, c22 * i]]


# ---------------------------------------------------------------- departure (c): dense unpivoted LDLT on the upper triangle
def ldlt_dense(S, b):
    """S [n, n] (upper triangle read), b [n].  Entry (i, j) subtracts L_ik (L_jk d_k) for k ascending, then divides by d_j -- run
    right-looking here, which applies the same subtractions to every entry in the same order.  Returns (ok, x)"""
    n = len(b)
    A = np.array(S, F64)
    d = np.zeros(n, F64)
    for k in range(n):
        d[k] = A[k, k]
        if not np.isfinite(d[k]) or d[k] == 0.0:
            return False, None
        A[k, k + 1:] = A[k, k + 1:] / d[k]                      # L[i][k], i > k
        if k + 1 < n:
            w = A[k, k + 1:] * d[k]                              # L_jk d_k
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - w[:, None] * A[k, k + 1:][None, :]   # entry (row j, column i): L_ik (L_jk d_k)
    y = np.array(b, F64)
    for k in range(n):
        y[k + 1:] = y[k + 1:] - A[k, k + 1:] * y[k]
    y = y / d
    for k in range(n - 1, -1, -1):
        y[:k] = y[:k] - A[:k, k] * y[k]
    return True, y


# ---------------------------------------------------------------- SE3 update of one pose (6i's routines)
def pose_update(x, pose):
    dq, dt = R6.se3_exp([F64(v) for v in x])
    q, t = R6.se3_mul(dq, dt, [F64(v) for v in pose[:4]], [F64(v) for v in pose[4:]])
    return np.array(list(q) + list(t), F64)


# ---------------------------------------------------------------- the optimisation
def local_ba(c, P=None):
    """c: a case dict (P, F, kf_pose [K,7], kf_cam [K,5], kf_nlevels [K], kf_sigma2 [K,16], kf_feat_off [K+1], kpts [Nf,2], octave, uright,
    xw [L,3], edge_point / edge_kf / edge_feat [E]).  Returns pose [P,7], pose_f32, point [L,3], point_f32, erase [E], chi2 [E], trace
    [iterations,4], stats [8], ret."""
    P = params() if P is None else P
    with np.errstate(all="ignore"):
        return _local_ba(c, P)


def _local_ba(c, P):
    check(c, P)
    S = Structure(c)
    Pn, K, L, E = S.P, S.K, S.L, S.E
    I = edge_inputs(c)
    hub = huber(P["th2_mono"]) + huber(P["th2_stereo"])
    pose = np.asarray(c["kf_pose"], F32).reshape(K, 7).astype(F64)
    for k in range(K):
        pose[k, :4] = R6.normalize_rotation(list(pose[k, :4]))
    pt = np.asarray(c["xw"], F32).reshape(L, 3).astype(F64)
    ep, ek = S.ep, S.ek
    fe = np.nonzero(S.free)[0]
    pose_rank = np.zeros(E, np.int64)
    for i in range(Pn):
        pose_rank[S.pose_list[i]] = np.arange(len(S.pose_list[i]))
    fk, fp = ek[fe], ep[fe]
    n6 = 6 * Pn
    max_trials = P["max_trials"] if P["max_trials"] > 0 else 10
    trace, stats = np.zeros((P["iterations"], 4), F64), np.zeros(8, np.int32)
    flags = 0
    chi2_stored = np.zeros(E, F64)
    xp, xl = np.zeros(n6, F64), np.zeros((L, 3), F64)
    lam, ni, nbad = F64(0.0), F64(2.0), 0
    iters = trials = rejected = failed = 0
    ended_rejected = False
    stop = P["stop"]
    ups = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    up6 = [(a, b) for a in range(6) for b in range(a, 6)]

    def errors_at(pose_, pt_):
        _, _, chi2, rho0, _ = edge_error(I, hub, pose_[ek, :4], pose_[ek, 4:], pt_[ep])
        return chi2, tree_sum(rho0)

    for it in range(P["iterations"]):
        if stop and not callable(stop):
            flags |= FLAG_STOPPED
            break
        iters += 1
        chi2_stored, rho0, lin = edge_linearise(I, hub, pose[ek, :4], pose[ek, 4:], pt[ep])
        current = tree_sum(rho0)
        ini = current
        pl = seq_sum_groups(lin[:, :9], ep, S.pt_rank, L)                      # Hll (6) | bl (3)
        pp = seq_sum_groups(lin[fe, 9:36], fk, pose_rank[fe], Pn)              # Hpp (21) | bp (6)
        Hll, bl, Hpp, bp = pl[:, :6], pl[:, 6:], pp[:, :21], pp[:, 21:]
        if it == 0:
            if P["user_lambda_init"] > 0:
                lam = F64(P["user_lambda_init"])
            else:
                # max |diagonal| with a NaN ignored (a > m), so the order does not matter
                dg = np.concatenate([np.abs(Hll[:, [0, 3, 5]]).ravel(), np.abs(Hpp[:, [0, 6, 11, 15, 18, 20]]).ravel(), [0.0]])
                dg = dg[~np.isnan(dg)]
                lam = 1e-5 * F64(dg.max())
            ni, nbad = F64(2.0), 0
        B = lin[:, 36:].reshape(E, 6, 3)
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            # per point: Dinv, db
            m = [[None] * 3 for _ in range(3)]
            for n_, (a, b) in enumerate(ups):
                m[a][b] = m[b][a] = Hll[:, n_]
            for a in range(3):
                m[a][a] = m[a][a] + lam
            D = inverse3(m)
            db = [(D[r][0] * bl[:, 0] + D[r][1] * bl[:, 1]) + D[r][2] * bl[:, 2] for r in range(3)]
            # per free edge: BDinv, B db
            Bf = B[fe]
            BD = np.zeros((len(fe), 6, 3), F64)
            Bdb = np.zeros((len(fe), 6), F64)
            for r in range(6):
                for cc in range(3):
                    BD[:, r, cc] = (Bf[:, r, 0] * D[0][cc][fp] + Bf[:, r, 1] * D[1][cc][fp]) + Bf[:, r, 2] * D[2][cc][fp]
                Bdb[:, r] = (Bf[:, r, 0] * db[0][fp] + Bf[:, r, 1] * db[1][fp]) + Bf[:, r, 2] * db[2][fp]
            fidx = np.full(E, -1, np.int64)
            fidx[fe] = np.arange(len(fe))
            # the reduced system, dense, upper triangle
            Sm = np.zeros((n6, n6), F64)
            for i in range(Pn):
                for n_, (a, b) in enumerate(up6):
                    Sm[6 * i + a, 6 * i + b] = Hpp[i, n_]
                for a in range(6):
                    Sm[6 * i + a, 6 * i + a] = Sm[6 * i + a, 6 * i + a] + lam
            if S.blocks:
                nb = len(S.blocks)
                lens = np.array([len(p) for p in S.pairs])
                acc = np.zeros((nb, 6, 6), F64)
                for bn, (i1, i2) in enumerate(S.blocks):
                    if i1 == i2:
                        acc[bn] = Sm[6 * i1:6 * i1 + 6, 6 * i1:6 * i1 + 6]
                for r_ in range(int(lens.max()) if nb else 0):
                    sel = np.nonzero(lens > r_)[0]
                    e1 = np.array([S.pairs[bn][r_, 0] for bn in sel])
                    e2 = np.array([S.pairs[bn][r_, 1] for bn in sel])
                    a_, b_ = BD[fidx[e1]], B[e2]                            # [m, 6, 3] each
                    v = (a_[:, :, None, 0] * b_[:, None, :, 0] + a_[:, :, None, 1] * b_[:, None, :, 1]) + a_[:, :, None, 2] * b_[:, None, :, 2]
                    acc[sel] = acc[sel] - v
                for bn, (i1, i2) in enumerate(S.blocks):
                    Sm[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6] = acc[bn]
            coeff = seq_sum_groups(Bdb, fk, pose_rank[fe], Pn)
            bs = (bp - coeff).reshape(-1)
            ok, sol = ldlt_dense(Sm, bs)
            if ok:
                xp = sol
                # cl = bl + sum B^T (-xp), ascending pose inside the point = ascending edge
                nx = -xp.reshape(Pn, 6)[fk] if len(fe) else np.zeros((0, 6), F64)
                v = np.zeros((len(fe), 3), F64)
                for cc in range(3):
                    a = Bf[:, 0, cc] * nx[:, 0]
                    for r in range(1, 6):
                        a = a + Bf[:, r, cc] * nx[:, r]
                    v[:, cc] = a
                cl = bl.copy()
                if len(fe):
                    for r_ in range(int(S.pt_rank[fe].max()) + 1):
                        msk = S.pt_rank[fe] == r_
                        cl[fp[msk]] = cl[fp[msk]] + v[msk]
                xl = np.stack([0.0 + ((D[r][0] * cl[:, 0] + D[r][1] * cl[:, 1]) + D[r][2] * cl[:, 2]) for r in range(3)], 1) if L else xl
            else:
                failed += 1
                flags |= FLAG_SOLVE_FAILED
            pt_new = pt + xl
            pose_new = pose.copy()
            for i in range(Pn):
                pose_new[i] = pose_update(xp[6 * i:6 * i + 6], pose[i])
            if not (np.all(np.isfinite(pt_new)) and np.all(np.isfinite(pose_new[:Pn]))):
                flags |= FLAG_NONFINITE
            xs = xp.reshape(Pn, 6)
            sterm = np.concatenate([(xs * (lam * xs + bp)).ravel(), (xl * (lam * xl + bl)).ravel()])
            chi2_stored, temp = errors_at(pose_new, pt_new)
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
                pose, pt = pose_new, pt_new
                ended_rejected = False
            else:
                lam = lam * ni
                ni = ni * 2
                rejected += 1
                ended_rejected = True
            qmax += 1
            if callable(stop):
                stop = stop()                                   # a test's hook: the flag as read after this trial
            if not (rho < 0 and qmax < max_trials and not stop):
                break
        if stop and not callable(stop):
            flags |= FLAG_STOPPED
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
        chi2_stored, _ = errors_at(pose, pt)
    if ended_rejected:
        flags |= FLAG_ENDED_REJECTED
    # classification at the final estimates with the stored chi2
    q, t, X = pose[ek, :4], pose[ek, 4:], pt[ep]
    zc = R6.rotate([q[:, 0], q[:, 1], q[:, 2], q[:, 3]], [X[:, 0], X[:, 1], X[:, 2]])[2] + t[:, 2] if E else np.zeros(0, F64)
    th = np.where(I["stereo"], F64(P["th2_stereo"]), F64(P["th2_mono"]))
    erase = ((chi2_stored > th) | ~(zc > 0.0)).astype(np.uint8)
    if not (np.all(np.isfinite(pose[:Pn])) and np.all(np.isfinite(pt))):
        flags |= FLAG_NONFINITE
    stats[:] = [iters, trials, rejected, failed, int(erase.sum()), flags, S.n_free, S.n_pairs]
    return {"pose": pose[:Pn].copy(), "pose_f32": pose[:Pn].astype(F32), "point": pt.copy(), "point_f32": pt.astype(F32), "erase": erase,
            "chi2": np.asarray(chi2_stored, F64).copy(), "trace": trace, "stats": stats, "ret": int(erase.sum())}


# ---------------------------------------------------------------- case generators
def scene(seed, P, F, L, kind="mixed", obs=None, noise=0.5, gross=0.0, rot=0.02, trans=0.05, pt_noise=0.05, nlevels=4, all_see=False,
          gross_px=(30.0, 100.0), spacing=0.15, depth=(4.0, 12.0)):
    """a planted local map: K = P + F keyframes on a short arc looking at L points 4 .. 12 m ahead; every point is seen by `obs` keyframes
    (default min(K, 4); all_see: every keyframe), its edges spread so that every keyframe is used.  Observations are exact projections
    plus Gaussian noise scaled by the level's sigma; a fraction `gross` of the observations is displaced by gross_px pixels (planted
    outliers); the free poses start `rot` rad and `trans` m off, the points `pt_noise` m off.  kind: mono, stereo or mixed."""
    rng = np.random.default_rng(seed)
    K = P + F
    sig2 = 1.44 ** np.arange(nlevels)
    fx, fy, cx, cy, bf = 458.654, 457.296, 367.215, 248.375, 47.91
    q_true, t_true = np.zeros((K, 4)), np.zeros((K, 3))
    for k in range(K):
        q_true[k] = R6.quat_from_rotvec(np.array([0.02, 0.05, 0.01]) * (k - K / 2) + rng.standard_normal(3) * 0.01)
        t_true[k] = np.array([spacing * (k - K / 2), 0.02 * rng.standard_normal(), 0.05 * rng.standard_normal()])
    Xw = np.stack([rng.uniform(-3, 3, L), rng.uniform(-2, 2, L), rng.uniform(depth[0], depth[1], L)], 1) if L else np.zeros((0, 3))
    nobs = K if all_see else min(K, 4 if obs is None else obs)
    ep, ekf = [], []
    for p in range(L):
        ks = sorted(set(int(v) for v in ((p + np.arange(nobs) * max(K // nobs, 1)) % K))) if not all_see else list(range(K))
        ep += [p] * len(ks)
        ekf += ks
    ep, ekf = np.asarray(ep, np.int64), np.asarray(ekf, np.int64)
    E = len(ep)
    # features: every keyframe lists its observations in edge order
    cnt = np.bincount(ekf, minlength=K) if E else np.zeros(K, np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ef = np.zeros(E, np.int64)
    seen = np.zeros(K, np.int64)
    for e in range(E):
        ef[e] = seen[ekf[e]]
        seen[ekf[e]] += 1
    Nf = int(off[-1])
    kpts, uright, octave = np.zeros((Nf, 2), F32), np.full(Nf, -1.0, F32), np.zeros(Nf, np.int32)
    planted = np.zeros(E, bool)
    for e in range(E):
        k, p = ekf[e], ep[e]
        Rm = R6.quat_to_mat(q_true[k])
        Xc = Rm @ Xw[p] + t_true[k]
        o = int(rng.integers(0, nlevels)) if kind == "mixed" else 0
        s = np.sqrt(sig2[o]) * noise
        u, v = fx * Xc[0] / Xc[2] + cx + s * rng.standard_normal(), fy * Xc[1] / Xc[2] + cy + s * rng.standard_normal()
        ur = fx * Xc[0] / Xc[2] + cx - bf / Xc[2] + s * rng.standard_normal()
        if rng.random() < gross:
            planted[e] = True
            a, m = rng.uniform(0, 2 * np.pi), rng.uniform(gross_px[0], gross_px[1])
            u, v = u + m * np.cos(a), v + m * np.sin(a)
        stereo = {"mono": False, "stereo": True, "mixed": rng.random() < 0.5}[kind]
        f = off[k] + ef[e]
        kpts[f] = [u, v]
        uright[f] = ur if stereo and ur >= 0.0 else -1.0        # no right match left of the image: a mono edge
        octave[f] = o
    pose0 = np.zeros((K, 7), F32)
    for k in range(K):
        if k < P:
            dq = R6.quat_from_rotvec(R6._unit(rng.standard_normal(3)) * rot)
            q0 = np.array(R6.quat_mul(list(dq), list(q_true[k])), F64)
            t0 = t_true[k] + R6._unit(rng.standard_normal(3)) * trans
        else:
            q0, t0 = q_true[k], t_true[k]
        pose0[k] = np.concatenate([q0, t0]).astype(F32)
    xw = (Xw + pt_noise * rng.standard_normal(Xw.shape)).astype(F32)
    sig = np.zeros((K, MAX_LEVELS), F32)
    sig[:, :nlevels] = (1.0 / sig2).astype(F32)
    return {"P": P, "F": F, "kf_pose": pose0, "kf_cam": np.tile(np.array([fx, fy, cx, cy, bf], F32), (K, 1)), "kf_nlevels": np.full(K, nlevels, np.int32),
            "kf_sigma2": sig, "kf_feat_off": off, "kpts": kpts, "octave": octave, "uright": uright, "xw": xw,
            "edge_point": ep.astype(np.int32), "edge_kf": ekf.astype(np.int32), "edge_feat": ef.astype(np.int32),
            "truth_pose": np.concatenate([q_true, t_true], 1), "truth_point": Xw, "planted": planted, "params": params()}


def optimises_scene():
    """test_it_optimises: 6 free and 3 fixed keyframes 0.4 m apart, 240 points 3 .. 8 m ahead seen by eight keyframes each, 0.3 sigma of
    noise, 10 % of the observations displaced by 10 .. 20 px"""
    return scene(61, 6, 3, 240, "mixed", obs=8, noise=0.3, gross=0.1, gross_px=(10.0, 20.0), spacing=0.4, depth=(3.0, 8.0))


def feature_of(c, e):
    return int(c["kf_feat_off"][c["edge_kf"][e]] + c["edge_feat"][e])


def forced(name):
    """the cases of the paths random scenes do not take"""
    if name == "one_trial":                   # max_trials = 1 from far off: qmax == max_trials ends the run after its first trial, rejected here
        c = scene(41, 3, 2, 60, "mixed", rot=0.6, trans=1.0, pt_noise=1.0)
        c["params"] = params(max_trials=1, user_lambda_init=1e-9)
    elif name == "stale":                     # two Gauss-Newton-sized trials from far off, both rejected: the stored chi2 are the second one's
        c = scene(41, 3, 2, 60, "mixed", rot=0.6, trans=1.0, pt_noise=1.0)
        c["params"] = params(max_trials=2, user_lambda_init=1e-9)
    elif name == "exact":
        c = _exact_case()
    elif name == "behind":                    # a point behind one of its cameras
        c = scene(43, 2, 2, 40, "mixed")
        c["special"] = 5
        k = int(c["edge_kf"][np.nonzero(c["edge_point"] == 5)[0][0]])
        Rm, t = R6.quat_to_mat(c["truth_pose"][k, :4]), c["truth_pose"][k, 4:]
        c["xw"][5] = (Rm.T @ (np.array([0.2, -0.1, -3.0]) - t)).astype(F32)
        c["params"] = params(iterations=1)
    elif name == "nan":
        c = scene(44, 2, 2, 40, "mixed")
        c["special"] = 7
        c["xw"][7, 1] = np.nan
    elif name == "fixed_only":                # point 3 is seen by fixed keyframes only
        c = scene(45, 2, 3, 30, "mixed")
        keep = ~((c["edge_point"] == 3) & (c["edge_kf"] < 2))
        c = drop_edges(c, keep)
        c["special"] = 3
    elif name == "single_edge":               # point 4 keeps one edge
        c = scene(46, 2, 2, 30, "mixed")
        first = np.nonzero(c["edge_point"] == 4)[0][0]
        keep = (c["edge_point"] != 4) | (np.arange(len(c["edge_point"])) == first)
        c = drop_edges(c, keep)
        c["special"] = 4
    elif name == "idle_pose":                 # free pose 1 has no edge
        c = scene(47, 3, 2, 30, "mixed")
        c = drop_edges(c, c["edge_kf"] != 1)
        c["special"] = 1
    elif name == "lambda100":
        c = scene(48, 3, 2, 60, "mixed")
        c["params"] = params(user_lambda_init=100.0)
    elif name == "stop":
        c = scene(49, 3, 2, 60, "mixed")
        c["params"] = params(stop=True)
    elif name == "zero_iterations":
        c = scene(50, 3, 2, 60, "mixed", gross=0.1)
        c["params"] = params(iterations=0)
    else:
        raise KeyError(name)
    return c


def drop_edges(c, keep):
    """the case without the edges where keep is False (features stay where they are)"""
    c = dict(c)
    for n in ("edge_point", "edge_kf", "edge_feat", "planted"):
        c[n] = c[n][keep]
    return c


def _exact_case(L=24):
    """errors that are 0.0 at the input: identity rotations, translations and depths that make every projection a float.  b = 0, x = 0,
    the trial leaves chi2 at 0 and rho == 0 ends the run after one rejected trial"""
    rng = np.random.default_rng(51)
    P, F = 2, 1
    K = P + F
    fx = fy = 512.0
    cx, cy, bf = 320.0, 240.0, 48.0
    z = 2.0 ** rng.integers(1, 4, L)
    x, y = rng.integers(-200, 200, L) / 128.0, rng.integers(-150, 150, L) / 128.0
    tks = np.array([[0.0, 0, 0], [0.25, 0, 0], [-0.5, 0.125, 0]])
    ep = np.repeat(np.arange(L), K)
    ek = np.tile(np.arange(K), L)
    ef = np.repeat(np.arange(L), K)
    off = (np.arange(K + 1) * L).astype(np.int32)
    kpts, uright = np.zeros((K * L, 2), F32), np.full(K * L, -1.0, F32)
    stereo = rng.random(L) < 0.5
    for k in range(K):
        xc, yc = x + tks[k, 0], y + tks[k, 1]
        u, v = fx * xc / z + cx, fy * yc / z + cy
        kpts[k * L:(k + 1) * L] = np.stack([u, v], 1)
        uright[k * L:(k + 1) * L] = np.where(stereo, u - bf / z, -1.0)
        assert np.array_equal(kpts[k * L:(k + 1) * L, 0].astype(F64), u)
    pose = np.zeros((K, 7), F32)
    pose[:, 3] = 1.0
    pose[:, 4:] = tks
    sig = np.zeros((K, MAX_LEVELS), F32)
    sig[:, :2] = [1.0, 0.5]
    return {"P": P, "F": F, "kf_pose": pose, "kf_cam": np.tile(np.array([fx, fy, cx, cy, bf], F32), (K, 1)), "kf_nlevels": np.full(K, 2, np.int32),
            "kf_sigma2": sig, "kf_feat_off": off, "kpts": kpts, "octave": rng.integers(0, 2, K * L).astype(np.int32), "uright": uright,
            "xw": np.stack([x, y, z], 1).astype(F32), "edge_point": ep.astype(np.int32), "edge_kf": ek.astype(np.int32),
            "edge_feat": ef.astype(np.int32), "planted": np.zeros(K * L, bool), "params": params(),
            "truth_pose": pose.astype(F64), "truth_point": np.stack([x, y, z], 1)}


def errors_to_truth(c, r):
    """(mean pose rotation error, mean pose translation error, mean point error) of a result, and of the input"""
    P = c["P"]
    def pe(poses):
        d = [R6.pose_distance(poses[i], c["truth_pose"][i]) for i in range(P)]
        return float(np.mean([a for a, _ in d])), float(np.mean([b for _, b in d]))
    out = pe(r["pose"]) + (float(np.mean(np.linalg.norm(r["point"] - c["truth_point"], axis=1))),)
    inp = pe(np.asarray(c["kf_pose"], F64)) + (float(np.mean(np.linalg.norm(np.asarray(c["xw"], F64) - c["truth_point"], axis=1))),)
    return out, inp


# ---------------------------------------------------------------- an edge planted at th2
def input_chi2(c, P, pose=None, point=None):
    """the chi2 every edge has at the input estimate (what a run without an LM iteration classifies), or at the free poses [P,7] and
    points [L,3] given in double"""
    K = c["P"] + c["F"]
    with np.errstate(all="ignore"):
        full = np.asarray(c["kf_pose"], F32).reshape(K, 7).astype(F64)
        for k in range(K):
            full[k, :4] = R6.normalize_rotation(list(full[k, :4]))
        if pose is not None:
            full[:c["P"]] = pose
        pose = full
        pt = np.asarray(c["xw"], F32).reshape(-1, 3).astype(F64) if point is None else np.asarray(point, F64)
        ek, ep = np.asarray(c["edge_kf"], np.int64), np.asarray(c["edge_point"], np.int64)
        hub = huber(P["th2_mono"]) + huber(P["th2_stereo"])
        return edge_error(edge_inputs(c), hub, pose[ek, :4], pose[ek, 4:], pt[ep])[2]


_threshold_found = {}


def threshold_case(stereo, which):
    """(case, edge): one fixed keyframe at the identity, one point, one edge, iterations = 0, whose chi2 is the double next below th2
    (`below`), th2 itself (`at`) or the double next above (`above`).  Found by a search over the ulps of the inputs, coarse to fine: the
    observation's u sets e0 a little too large, the point's x (near 1e-5, so its ulps move the projection by 1e-10 px) brings e0's term
    to 1 .. 2e-9 below the target, and the observation's v (near 4e-5 with cy = 0, so e1 = v) makes up the rest ulp by ulp, each step a
    fraction of an ulp of chi2."""
    key = (bool(stereo), which)
    if key not in _threshold_found:
        th2 = F64(TH2_STEREO if stereo else TH2_MONO)
        target = {"below": np.nextafter(th2, -np.inf), "at": th2, "above": np.nextafter(th2, np.inf)}[which]
        fx, z, cx = 512.0, 8.0, (8.0 if stereo else 0.0)        # stereo: cx keeps uright positive
        sig = np.zeros((1, MAX_LEVELS), F32)
        sig[0, 0] = 1.0
        c = {"P": 0, "F": 1, "kf_pose": np.array([[0, 0, 0, 1, 0, 0, 0]], F32), "kf_cam": np.array([[fx, fx, cx, 0.0, 48.0]], F32),
             "kf_nlevels": np.ones(1, np.int32), "kf_sigma2": sig, "kf_feat_off": np.array([0, 1], np.int32), "kpts": np.zeros((1, 2), F32),
             "octave": np.zeros(1, np.int32), "uright": np.full(1, -1.0, F32), "xw": np.array([[0.0, 0.0, z]], F32),
             "edge_point": np.zeros(1, np.int32), "edge_kf": np.zeros(1, np.int32), "edge_feat": np.zeros(1, np.int32),
             "planted": np.zeros(1, bool), "params": params(iterations=0)}
        P = c["params"]
        if stereo:
            c["uright"][0] = F32(cx - 48.0 / z + 0.25)             # e2 = 0.25 plus what x moves: its term is part of the coarse level
        chi = lambda: input_chi2(c, P)[0]
        # u: the first float that leaves chi2 at x = 0 above the target by a margin x can make up
        c["kpts"][0, 0] = F32(cx + np.sqrt(th2 - (0.0625 if stereo else 0.0)) - 1e-4)
        while chi() < target + 1e-6:
            c["kpts"][0, 0] = np.nextafter(c["kpts"][0, 0], F32(np.inf))
        # x: bisection on its float bits for the largest chi2 at least 1e-9 below the target
        lo, hi = F32(0.0), F32(1e-4)
        def at_x(x):
            c["xw"][0, 0] = x
            return chi()
        assert at_x(hi) < target - 1e-9 < at_x(lo)
        while np.nextafter(lo, hi) < hi:
            mid = F32(0.5) * (lo + hi)
            if at_x(mid) > target - 1e-9:
                lo = mid
            else:
                hi = mid
        gap = target - at_x(hi)
        assert 1e-9 <= gap < 4e-9, gap
        # v: e1 = v makes up the gap; ulp by ulp until the double is hit
        v0 = F32(np.sqrt(gap))
        found = False
        for step in (F32(np.inf), F32(-np.inf)):
            v = v0
            for _ in range(20000):
                c["kpts"][0, 1] = v
                got = chi()
                if got == target:
                    found = True
                    break
                if (got > target) == (step > 0):
                    break
                v = np.nextafter(v, step)
            if found:
                break
        assert found, "no v gives the planted chi2"
        _threshold_found[key] = c
    c = _threshold_found[key]
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}, 0
