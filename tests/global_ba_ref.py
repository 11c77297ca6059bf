"""numpy float64 restatement of Optimizer::BundleAdjustment behind GlobalBundleAdjustemnt (reference src/Optimizer.cc:2832-3220 over g2o's
BlockSolver_6_3 and Levenberg-Marquardt), the contract of DESIGN.md 6n.  It is 6l's arithmetic (tests/local_ba_ref.py, whose routines it
calls) with three changes: the keyframes carry a `fixed` flag instead of standing free-first, so the Hessian order is the free keyframes in
ascending index; `robust == 0` takes base_binary_edge.hpp:75-90 instead of the Huber branch; and the reduced system is factored by the
dense-order unpivoted LDLT over the tiles of the covisibility pattern's fill, with 6m(g)'s failure rule.  The Schur blocks are held
sparsely -- only blocks that have a pair, [NB, 6, 6] -- and the solve's working matrix is touched only inside the tiles of the fill.
Shared by test_global_ba_ref.py (CPU), test_gpu_global_ba.py, test_gpu_global_ba_dropin.py and tools/bench_global_ba.py; holds the case
generators."""
import numpy as np

import local_ba_ref as LR
import pose_opt_ref as R6

F32, F64 = np.float32, np.float64
MAX_LEVELS = LR.MAX_LEVELS
MAX_KF, MAX_POINTS, MAX_EDGES, MAX_ITERATIONS, MAX_PAIRS = 1024, 1 << 18, 1 << 21, 64, 1 << 25
TILE_V, TILE = 4, 24
DBL_MAX = LR.DBL_MAX
FLAG_ENDED_REJECTED, FLAG_SOLVE_FAILED, FLAG_NONFINITE, FLAG_STOPPED, FLAG_NO_ITERATION = 1, 2, 4, 8, 16
HUBER2_MONO, HUBER2_STEREO = 5.99, 7.815              # `sqrt(5.99)` and `sqrt(7.815)` in BundleAdjustment, not LocalBundleAdjustment's 5.991

# what the departures cost against g2o's own choices (sequential global sums, numpy.linalg.solve, numpy.linalg.inv, the edge-less point
# removed), measured by test_global_ba_ref.py::test_departure_cost on its cases: the largest absolute difference of any pose number and
# of any point coordinate; the test allows 8 times as much
DEPARTURE_MAX = (1.1e-11, 1.9e-11)
# how much closer to the planted poses (rotation, translation) and points the optimisation gets in test_it_optimises, before / after,
# measured when the test was written; the test asks for a sixteenth
OPTIMISES_GAIN = (3.10, 1.55, 3.43)


class Invalid(ValueError):
    """what the entry refuses with RFE_ERR_INVALID"""


def params(iterations=10, max_trials=0, user_lambda_init=0.0, robust=False, huber2_mono=HUBER2_MONO, huber2_stereo=HUBER2_STEREO, stop=False):
    return {"iterations": int(iterations), "max_trials": int(max_trials), "user_lambda_init": float(user_lambda_init), "robust": bool(robust),
            "huber2_mono": float(huber2_mono), "huber2_stereo": float(huber2_stereo), "stop": stop}


def check(c, P):
    """the refusals; c: a case dict"""
    K, L, E, Nf = len(c["fixed"]), len(c["xw"]), len(c["edge_point"]), len(c["kpts"])
    if not (1 <= K <= MAX_KF and L <= MAX_POINTS and E <= MAX_EDGES):
        raise Invalid("shape")
    if not (0 <= P["iterations"] <= MAX_ITERATIONS and P["max_trials"] >= 0):
        raise Invalid("iterations")
    if not np.all(np.isfinite([P["user_lambda_init"], P["huber2_mono"], P["huber2_stereo"]])):
        raise Invalid("non-finite parameter")
    nl, off = np.asarray(c["kf_nlevels"]), np.asarray(c["kf_feat_off"], np.int64)
    if np.any((nl < 1) | (nl > MAX_LEVELS)) or np.any(off < 0) or np.any(off > Nf) or np.any(np.diff(off) < 0):
        raise Invalid("keyframe table")
    p, k, f = (np.asarray(c[n], np.int64) for n in ("edge_point", "edge_kf", "edge_feat"))
    if np.any((p < 0) | (p >= L) | (k < 0) | (k >= K)):
        raise Invalid("edge index out of range")
    if np.any((f < 0) | (f >= off[k + 1] - off[k])):
        raise Invalid("edge index out of range")
    if np.any(np.diff(p * (K + 1) + k) <= 0):
        raise Invalid("edges not strictly ascending")
    if schur_pairs(c) > MAX_PAIRS:
        raise Invalid("pairs")


def schur_pairs(c):
    """the Schur pair entries: the sum over the points of n (n + 1) / 2, n the point's edges on free keyframes -- counted from the edge
    table alone, before anything is built"""
    p, k = np.asarray(c["edge_point"], np.int64), np.asarray(c["edge_kf"], np.int64)
    n = np.bincount(p[np.asarray(c["fixed"])[k] == 0], minlength=len(c["xw"])).astype(np.int64) if len(p) else np.zeros(1, np.int64)
    return int(np.sum(n * (n + 1) // 2))


# ---------------------------------------------------------------- structure
def tile_fill(blocks_i1, blocks_i2, Pn):
    """the tile-level fill of the block pattern: (fill [NT, NT] bool, lower triangle with the diagonal, the number of tiles marked)"""
    NT = (Pn + TILE_V - 1) // TILE_V
    fill = np.zeros((NT, NT), bool)
    fill[np.arange(NT), np.arange(NT)] = True
    fill[np.asarray(blocks_i2, np.int64) // TILE_V, np.asarray(blocks_i1, np.int64) // TILE_V] = True
    for J in range(NT):
        rows = np.nonzero(fill[J + 1:, J])[0] + J + 1
        for n_, I1 in enumerate(rows):
            fill[I1, rows[:n_ + 1]] = True
    return fill, int(np.tril(fill).sum())


class Structure:
    """the free keyframes' numbering, per-point edge ranges, every free edge's rank in its pose's ascending list, the non-empty Schur
    blocks (i1 <= i2, every diagonal block among them) in ascending (i1, i2) with their pairs (e1, e2) ascending in the point, and the
    tile fill"""

    def __init__(self, c):
        self.fixed = np.asarray(c["fixed"]).astype(bool)
        self.K, self.L, self.E = len(self.fixed), len(c["xw"]), len(c["edge_point"])
        self.free_list = np.nonzero(~self.fixed)[0]
        self.P = P = len(self.free_list)
        self.free_index = np.full(self.K, -1, np.int64)
        self.free_index[self.free_list] = np.arange(P)
        self.ep, self.ek = np.asarray(c["edge_point"], np.int64), np.asarray(c["edge_kf"], np.int64)
        self.pt_start = np.searchsorted(self.ep, np.arange(self.L + 1))
        self.pt_rank = np.arange(self.E) - self.pt_start[self.ep] if self.E else np.zeros(0, np.int64)
        self.included = (np.diff(self.pt_start) > 0).astype(np.uint8)
        fi = self.free_index[self.ek] if self.E else np.zeros(0, np.int64)
        self.fe = fe = np.nonzero(fi >= 0)[0]
        self.fk, self.fp = fi[fe], self.ep[fe]
        nfe = len(fe)
        order = np.argsort(self.fk, kind="stable")
        cnt = np.bincount(self.fk, minlength=P) if nfe else np.zeros(P, np.int64)
        start = np.concatenate([[0], np.cumsum(cnt)])
        self.pose_rank = np.zeros(nfe, np.int64)
        self.pose_rank[order] = np.arange(nfe) - start[self.fk[order]]
        # pairs: free edge a (a position in fe) with every free edge b >= a of the same point
        if nfe:
            pend = np.searchsorted(self.fp, self.fp, side="right")
            m = pend - np.arange(nfe)
            a = np.repeat(np.arange(nfe), m)
            b = a + (np.arange(len(a)) - np.repeat(np.cumsum(m) - m, m))
        else:
            a = b = np.zeros(0, np.int64)
        key = self.fk[a] * P + self.fk[b] if len(a) else np.zeros(0, np.int64)
        o = np.lexsort((a, key))
        a, b, key = a[o], b[o], key[o]
        bkeys = np.union1d(key, np.arange(P) * (P + 1))
        self.blk_i1, self.blk_i2 = bkeys // max(P, 1), bkeys % max(P, 1)
        self.NB = len(bkeys)
        self.pair_a, self.pair_b = a, b
        self.pair_blk = np.searchsorted(bkeys, key)
        first = np.searchsorted(key, key, side="left")
        self.pair_rank = np.arange(len(a)) - first
        ro = np.argsort(self.pair_rank, kind="stable")          # the pairs by rank, so that rank r is one slice
        self.rank_order = ro
        self.rank_start = np.searchsorted(self.pair_rank[ro], np.arange((int(self.pair_rank.max()) + 2) if len(a) else 1))
        self.n_pairs = len(a)
        self.fill, self.tiles = tile_fill(self.blk_i1, self.blk_i2, P)
        NT = self.fill.shape[0]
        self.tiles_dense = NT * (NT + 1) // 2


# ---------------------------------------------------------------- edges
NO_HUBER = (F64(np.inf), F64(np.inf), F64(np.inf), F64(np.inf))


def huber(th2):
    """`const float thHuber2D = sqrt(5.99)`; RobustKernelHuber keeps dsqr in a float member"""
    return LR.huber(th2)


def edge_error(I, hub, q, t, X, robust):
    """6l's edge_error; without a robust kernel activeChi2 sums chi2 itself"""
    xyz, e, chi2, rho0, rho1 = LR.edge_error(I, hub if robust else NO_HUBER, q, t, X)
    if not robust:
        rho0 = chi2
    return xyz, e, chi2, rho0, rho1


def edge_linearise(I, hub, q, t, X, robust):
    """chi2, rho0 and lin [E, 54] in 6l's layout.  robust: 6l's, entry for entry.  Otherwise base_binary_edge.hpp:75-90 with Omega =
    invSigma2 I: omega_r = -(Omega e); AtO = A^T Omega, rounded first; the point gets AtO A and A^T omega_r; the pose gets (B^T Omega) B
    and B^T omega_r; the stored block (_hessianRowMajor) is B^T AtO^T, entry (a, b) = sum_k B[k][a] AtO[b][k]"""
    if robust:
        return LR.edge_linearise(I, hub, q, t, X)
    (x, y, z), e, chi2, _, _ = LR.edge_error(I, NO_HUBER, q, t, X)
    n = len(x)
    st, isg, fx, fy, bf = I["stereo"], I["isg"], I["fx"], I["fy"], I["bf"]
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    Rm = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
    zero, one = np.zeros(n, F64), np.ones(n, F64)
    z_2 = z * z
    Xis = [[-fx * Rm[0][c] / z + fx * x * Rm[2][c] / z_2 for c in range(3)], [-fy * Rm[1][c] / z + fy * y * Rm[2][c] / z_2 for c in range(3)]]
    Xis.append([Xis[0][c] - bf * Rm[2][c] / z_2 for c in range(3)])
    Xjs = [[x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx, -1. / z * fx, zero, x / z_2 * fx],
           [(1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy, zero, -1. / z * fy, y / z_2 * fy]]
    Xjs.append([Xjs[0][0] - bf * y / z_2, Xjs[0][1] + bf * x / z_2, Xjs[0][2], Xjs[0][3], zero, Xjs[0][5] - bf / z_2])
    nJ = [[-(fx / z), -zero, -(-fx * x / (z * z))], [-zero, -(fy / z), -(-fy * y / (z * z))]]
    Sd = [[zero, z, -y, one, zero, zero], [-z, zero, x, zero, one, zero], [y, -x, zero, zero, zero, one]]
    Xim = [[(nJ[r][0] * Rm[0][c] + nJ[r][1] * Rm[1][c]) + nJ[r][2] * Rm[2][c] for c in range(3)] for r in range(2)]
    Xjm = [[(nJ[r][0] * Sd[0][c] + nJ[r][1] * Sd[1][c]) + nJ[r][2] * Sd[2][c] for c in range(6)] for r in range(2)]
    A = [[np.where(st, Xis[r][c], Xim[r][c]) for c in range(3)] for r in range(2)] + [Xis[2]]
    B = [[np.where(st, Xjs[r][c], Xjm[r][c]) for c in range(6)] for r in range(2)] + [Xjs[2]]
    omr = [-(isg * e[r]) for r in range(3)]
    AtO = [[A[k][a] * isg for k in range(3)] for a in range(3)]        # AtO[a][k]
    BtO = [[B[k][a] * isg for k in range(3)] for a in range(6)]
    lin = np.zeros((n, 54), F64)
    col = 0

    def dot3(u, v):                                  # u[k], v[k]
        h = u[0] * v[0] + u[1] * v[1]
        return np.where(st, h + u[2] * v[2], h)

    for a in range(3):
        for b in range(a, 3):
            lin[:, col] = dot3(AtO[a], [A[k][b] for k in range(3)])
            col += 1
    for a in range(3):
        lin[:, col] = dot3([A[k][a] for k in range(3)], omr)
        col += 1
    for a in range(6):
        for b in range(a, 6):
            lin[:, col] = dot3(BtO[a], [B[k][b] for k in range(3)])
            col += 1
    for a in range(6):
        lin[:, col] = dot3([B[k][a] for k in range(3)], omr)
        col += 1
    for a in range(6):
        for b in range(3):
            lin[:, col] = 0.0 + dot3([B[k][a] for k in range(3)], AtO[b])
            col += 1
    return chi2, chi2, lin


# ---------------------------------------------------------------- the solve
def ldlt_tiled(S, b, fill, T=TILE):
    """6l(c)'s dense-order unpivoted LDLT with 6m(g)'s failure rule, run over the tiles of `fill` only: entry (i, j) subtracts
    L_ik (L_jk d_k) for k ascending and divides by d_j; an operand inside a tile the fill leaves out is structurally zero and its term is
    skipped.  S [n, n] (upper triangle read, modified in place), b [n].  (False, None): a pivot that is zero or not finite, an entry of L
    or of the solution that is not finite.  The solution gets + 0.0 last"""
    n = len(b)
    if n == 0:
        return True, np.zeros(0, F64)
    NT = fill.shape[0]
    A = S
    span = lambda I: np.arange(I * T, min((I + 1) * T, n))
    below = [np.concatenate([span(I) for I in range(K, NT) if fill[I, K]]) for K in range(NT)]
    left = [np.concatenate([span(J) for J in range(K + 1) if fill[K, J]]) for K in range(NT)]
    d = np.zeros(n, F64)
    ok = True
    for k in range(n):
        idx = below[k // T]
        idx = idx[idx > k]
        d[k] = A[k, k]
        if not np.isfinite(d[k]) or d[k] == 0.0:
            ok = False
        if len(idx) == 0:
            continue
        l = A[k, idx] / d[k]
        A[k, idx] = l
        if not np.all(np.isfinite(l)):
            ok = False
        w = l * d[k]
        ix = np.ix_(idx, idx)
        A[ix] = A[ix] - w[:, None] * l[None, :]
    if not ok:
        return False, None
    y = np.array(b, F64)
    for k in range(n):
        idx = below[k // T]
        idx = idx[idx > k]
        y[idx] = y[idx] - A[k, idx] * y[k]
    y = y / d
    for k in range(n - 1, -1, -1):
        idx = left[k // T]
        idx = idx[idx < k]
        y[idx] = y[idx] - A[idx, k] * y[k]
    y = y + 0.0
    if not np.all(np.isfinite(y)):
        return False, None
    return True, y


def seq_sum(v):
    """g2o's own choice for a global sum: one accumulator, ascending"""
    acc = F64(0.0)
    for x in np.asarray(v, F64).ravel():
        acc = acc + x
    return acc


# ---------------------------------------------------------------- the optimisation
def global_ba(c, P=None, g2o=False):
    """c: a case dict (fixed [K], kf_pose [K,7], kf_cam [K,5], kf_nlevels [K], kf_sigma2 [K,16], kf_feat_off [K+1], kpts [Nf,2], octave,
    uright, xw [L,3], edge_point / edge_kf / edge_feat [E]).  Returns pose [K,7], pose_f32, point [L,3], point_f32, included [L], chi2 [E],
    trace [iterations,4], stats [8], ret.  g2o: the departures' cost -- sequential global sums, numpy.linalg.inv, numpy.linalg.solve"""
    P = params() if P is None else P
    with np.errstate(all="ignore"):
        return _global_ba(c, P, g2o)


def _global_ba(c, P, g2o):
    check(c, P)
    S = Structure(c)
    Pn, K, L, E = S.P, S.K, S.L, S.E
    robust = P["robust"]
    I = LR.edge_inputs({**c, "P": K, "F": 0})
    hub = huber(P["huber2_mono"]) + huber(P["huber2_stereo"])
    total = seq_sum if g2o else LR.tree_sum
    pose = np.asarray(c["kf_pose"], F32).reshape(K, 7).astype(F64)
    for k in range(K):
        pose[k, :4] = R6.normalize_rotation(list(pose[k, :4]))
    pt = np.asarray(c["xw"], F32).reshape(L, 3).astype(F64)
    ep, ek, fe, fk, fp = S.ep, S.ek, S.fe, S.fk, S.fp
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
    diag_blk = np.searchsorted(S.blk_i1 * max(Pn, 1) + S.blk_i2, np.arange(Pn) * (Pn + 1))

    def errors_at(pose_, pt_):
        _, _, chi2, rho0, _ = edge_error(I, hub, pose_[ek, :4], pose_[ek, 4:], pt_[ep], robust)
        return chi2, total(rho0)

    for it in range(P["iterations"]):
        if stop and not callable(stop):
            flags |= FLAG_STOPPED
            break
        iters += 1
        chi2_stored, rho0, lin = edge_linearise(I, hub, pose[ek, :4], pose[ek, 4:], pt[ep], robust)
        current = total(rho0)
        ini = current
        pl = LR.seq_sum_groups(lin[:, :9], ep, S.pt_rank, L)
        pp = LR.seq_sum_groups(lin[fe, 9:36], fk, S.pose_rank, Pn)
        Hll, bl, Hpp, bp = pl[:, :6], pl[:, 6:], pp[:, :21], pp[:, 21:]
        if it == 0:
            if P["user_lambda_init"] > 0:
                lam = F64(P["user_lambda_init"])
            else:
                dg = np.concatenate([np.abs(Hll[:, [0, 3, 5]]).ravel(), np.abs(Hpp[:, [0, 6, 11, 15, 18, 20]]).ravel(), [0.0]])
                dg = dg[~np.isnan(dg)]
                lam = 1e-5 * F64(dg.max())
            ni, nbad = F64(2.0), 0
        B = lin[:, 36:].reshape(E, 6, 3)
        Bf = B[fe]
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            m = [[None] * 3 for _ in range(3)]
            for n_, (a, b) in enumerate(ups):
                m[a][b] = m[b][a] = Hll[:, n_]
            for a in range(3):
                m[a][a] = m[a][a] + lam
            if g2o:
                Dm = np.linalg.inv(np.stack([np.stack(r, 1) for r in m], 1)) if L else np.zeros((0, 3, 3))
                D = [[Dm[:, r, cc] for cc in range(3)] for r in range(3)]
            else:
                D = LR.inverse3(m)
            db = [(D[r][0] * bl[:, 0] + D[r][1] * bl[:, 1]) + D[r][2] * bl[:, 2] for r in range(3)]
            BD = np.zeros((len(fe), 6, 3), F64)
            Bdb = np.zeros((len(fe), 6), F64)
            for r in range(6):
                for cc in range(3):
                    BD[:, r, cc] = (Bf[:, r, 0] * D[0][cc][fp] + Bf[:, r, 1] * D[1][cc][fp]) + Bf[:, r, 2] * D[2][cc][fp]
                Bdb[:, r] = (Bf[:, r, 0] * db[0][fp] + Bf[:, r, 1] * db[1][fp]) + Bf[:, r, 2] * db[2][fp]
            # the reduced system: the blocks of the pattern
            acc = np.zeros((S.NB, 6, 6), F64)
            for n_, (a, b) in enumerate(up6):
                acc[diag_blk, a, b] = Hpp[:, n_]
            for a in range(6):
                acc[diag_blk, a, a] = acc[diag_blk, a, a] + lam
            if S.n_pairs:
                a_, b_ = BD[S.pair_a], Bf[S.pair_b]
                v = (a_[:, :, None, 0] * b_[:, None, :, 0] + a_[:, :, None, 1] * b_[:, None, :, 1]) + a_[:, :, None, 2] * b_[:, None, :, 2]
                for r_ in range(len(S.rank_start) - 1):
                    sel = S.rank_order[S.rank_start[r_]:S.rank_start[r_ + 1]]
                    acc[S.pair_blk[sel]] = acc[S.pair_blk[sel]] - v[sel]
            Sm = np.zeros((n6, n6), F64)
            for bn in range(S.NB):
                i1, i2 = S.blk_i1[bn], S.blk_i2[bn]
                Sm[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6] = np.triu(acc[bn]) if i1 == i2 else acc[bn]
            coeff = LR.seq_sum_groups(Bdb, fk, S.pose_rank, Pn)
            bs = (bp - coeff).reshape(-1)
            if g2o:
                full = np.triu(Sm) + np.triu(Sm, 1).T
                sol = np.linalg.solve(full, bs) if n6 else np.zeros(0, F64)
                ok = bool(np.all(np.isfinite(sol)))
            else:
                ok, sol = ldlt_tiled(Sm, bs, S.fill)
            if ok:
                xp = sol
                nx = -xp.reshape(Pn, 6)[fk] if len(fe) else np.zeros((0, 6), F64)
                v = np.zeros((len(fe), 3), F64)
                for cc in range(3):
                    a = Bf[:, 0, cc] * nx[:, 0]
                    for r in range(1, 6):
                        a = a + Bf[:, r, cc] * nx[:, r]
                    v[:, cc] = a
                cl = bl.copy()
                if len(fe):
                    # ascending free edge inside the point
                    prank = np.arange(len(fe)) - np.searchsorted(fp, fp, side="left")
                    for r_ in range(int(prank.max()) + 1):
                        msk = prank == r_
                        cl[fp[msk]] = cl[fp[msk]] + v[msk]
                xl = np.stack([0.0 + ((D[r][0] * cl[:, 0] + D[r][1] * cl[:, 1]) + D[r][2] * cl[:, 2]) for r in range(3)], 1) if L else xl
            else:
                failed += 1
                flags |= FLAG_SOLVE_FAILED
            pt_new = pt + xl
            pose_new = pose.copy()
            for i in range(Pn):
                pose_new[S.free_list[i]] = LR.pose_update(xp[6 * i:6 * i + 6], pose[S.free_list[i]])
            if not (np.all(np.isfinite(pt_new)) and np.all(np.isfinite(pose_new[S.free_list]))):
                flags |= FLAG_NONFINITE
            xs = xp.reshape(Pn, 6)
            sterm = np.concatenate([(xs * (lam * xs + bp)).ravel(), (xl * (lam * xl + bl)).ravel()])
            chi2_stored, temp = errors_at(pose_new, pt_new)
            if not ok:
                temp = F64(DBL_MAX)
            scale = total(sterm) + 1e-3
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
            if callable(stop) and stop():                       # a test's hook: the flag as read after this trial; asked until it says yes
                stop = True
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
    if not (np.all(np.isfinite(pose)) and np.all(np.isfinite(pt))):
        flags |= FLAG_NONFINITE
    stats[:] = [iters, trials, rejected, failed, flags, Pn, S.tiles, S.tiles_dense]
    return {"pose": pose.copy(), "pose_f32": pose.astype(F32), "point": pt.copy(), "point_f32": pt.astype(F32), "included": S.included,
            "chi2": np.asarray(chi2_stored, F64).copy(), "trace": trace, "stats": stats, "ret": iters}


# ---------------------------------------------------------------- case generators
def from_local(c, P=None):
    """a 6l case (P free keyframes first, then F fixed) as a case of this contract; the parameters carry over with equal Huber values"""
    g = {k: v for k, v in c.items() if k not in ("P", "F", "params")}
    g["fixed"] = np.concatenate([np.zeros(c["P"], np.uint8), np.ones(c["F"], np.uint8)])
    lp = c["params"] if P is None else P
    g["params"] = params(lp["iterations"], lp["max_trials"], lp["user_lambda_init"], True, lp["th2_mono"], lp["th2_stereo"], lp["stop"])
    return g


def pattern(name, K, ppk=3, seed=0):
    """per point the ascending keyframes that see it.  chain: ppk points per keyframe, each seen by three consecutive keyframes; loop: the
    chain closed by points on (K-2, K-1, 0) and (K-1, 0, 1); star: keyframe K-1 sees every point, each with one other keyframe; hub: the
    same with keyframe 0 as the hub (the fill is dense); dense: four random keyframes per point; pairs5: the ten pairs of five keyframes"""
    rng = np.random.default_rng(seed)
    vis = []
    if name in ("chain", "loop"):
        for s in range(max(K - 2, 1)):
            vis += [sorted(set(min(s + j, K - 1) for j in range(3)))] * ppk
        if name == "loop" and K >= 4:
            vis += [[0, K - 2, K - 1]] * ppk + [[0, 1, K - 1]] * ppk
    elif name in ("star", "hub"):
        hub = K - 1 if name == "star" else 0
        for k in range(K):
            if k != hub:
                vis += [sorted((k, hub))] * ppk
    elif name == "dense":
        for _ in range(ppk * K):
            vis.append(sorted(int(v) for v in rng.choice(K, min(4, K), replace=False)))
    elif name == "pairs5":
        prs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
        vis = [list(prs[j % 10]) for j in range(ppk)]
    else:
        raise KeyError(name)
    return vis


def scene(seed, K, fixed, vis, kind="mixed", ring=False, noise=0.5, gross=0.0, rot=0.02, trans=0.05, pt_noise=0.05, nlevels=4, spacing=0.3,
          depth=(4.0, 12.0), edgeless=()):
    """a planted map: K keyframes looking along +z, `spacing` apart on a line (or on a ring in the image plane, so that the last ones
    stand next to the first); point p is seen by the keyframes vis[p] and lies 4 .. 12 m ahead of their middle; the points listed in
    `edgeless` lose their edges.  Observations are exact projections plus Gaussian noise scaled by the level's sigma; the free poses
    start `rot` rad and `trans` m off, the points `pt_noise` m off.  fixed: the indices of the fixed keyframes"""
    rng = np.random.default_rng(seed)
    L = len(vis)
    sig2 = 1.44 ** np.arange(nlevels)
    fx, fy, cx, cy, bf = 458.654, 457.296, 367.215, 248.375, 47.91
    q_true, t_true, centre = np.zeros((K, 4)), np.zeros((K, 3)), np.zeros((K, 3))
    rad = max(K * spacing / (2 * np.pi), spacing)
    for k in range(K):
        q_true[k] = R6.quat_from_rotvec(rng.standard_normal(3) * 0.01)
        a = 2 * np.pi * k / K
        centre[k] = np.array([rad * np.cos(a), rad * np.sin(a), 0.0]) if ring else np.array([spacing * k, 0.0, 0.0])
        centre[k] += np.array([0.0, 0.02, 0.05]) * rng.standard_normal(3)
        t_true[k] = -(R6.quat_to_mat(q_true[k]) @ centre[k])
    Xw = np.zeros((L, 3))
    ep, ekf = [], []
    for p in range(L):
        ks = list(vis[p])
        Xw[p] = centre[ks].mean(0) + np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(depth[0], depth[1])])
        if p not in edgeless:
            ep += [p] * len(ks)
            ekf += ks
    ep, ekf = np.asarray(ep, np.int64), np.asarray(ekf, np.int64)
    E = len(ep)
    cnt = np.bincount(ekf, minlength=K) if E else np.zeros(K, np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    order = np.argsort(ekf, kind="stable")
    ef = np.zeros(E, np.int64)
    ef[order] = np.arange(E) - off[ekf[order]]
    Nf = int(off[-1])
    kpts, uright, octave = np.zeros((Nf, 2), F32), np.full(Nf, -1.0, F32), np.zeros(Nf, np.int32)
    Rk = [R6.quat_to_mat(q_true[k]) for k in range(K)]
    for e in range(E):
        k, p = ekf[e], ep[e]
        Xc = Rk[k] @ Xw[p] + t_true[k]
        o = int(rng.integers(0, nlevels)) if kind == "mixed" else 0
        s = np.sqrt(sig2[o]) * noise
        u, v = fx * Xc[0] / Xc[2] + cx + s * rng.standard_normal(), fy * Xc[1] / Xc[2] + cy + s * rng.standard_normal()
        ur = fx * Xc[0] / Xc[2] + cx - bf / Xc[2] + s * rng.standard_normal()
        if rng.random() < gross:
            a, m = rng.uniform(0, 2 * np.pi), rng.uniform(10.0, 20.0)
            u, v = u + m * np.cos(a), v + m * np.sin(a)
        stereo = {"mono": False, "stereo": True, "mixed": rng.random() < 0.5}[kind]
        f = off[k] + ef[e]
        kpts[f] = [u, v]
        uright[f] = ur if stereo and ur >= 0.0 else -1.0
        octave[f] = o
    fx_flag = np.zeros(K, np.uint8)
    fx_flag[list(fixed)] = 1
    pose0 = np.zeros((K, 7), F32)
    for k in range(K):
        if fx_flag[k]:
            q0, t0 = q_true[k], t_true[k]
        else:
            dq = R6.quat_from_rotvec(R6._unit(rng.standard_normal(3)) * rot)
            q0 = np.array(R6.quat_mul(list(dq), list(q_true[k])), F64)
            t0 = t_true[k] + R6._unit(rng.standard_normal(3)) * trans
        pose0[k] = np.concatenate([q0, t0]).astype(F32)
    xw = (Xw + pt_noise * rng.standard_normal(Xw.shape)).astype(F32)
    sig = np.zeros((K, MAX_LEVELS), F32)
    sig[:, :nlevels] = (1.0 / sig2).astype(F32)
    return {"fixed": fx_flag, "kf_pose": pose0, "kf_cam": np.tile(np.array([fx, fy, cx, cy, bf], F32), (K, 1)),
            "kf_nlevels": np.full(K, nlevels, np.int32), "kf_sigma2": sig, "kf_feat_off": off, "kpts": kpts, "octave": octave, "uright": uright,
            "xw": xw, "edge_point": ep.astype(np.int32), "edge_kf": ekf.astype(np.int32), "edge_feat": ef.astype(np.int32),
            "truth_pose": np.concatenate([q_true, t_true], 1), "truth_point": Xw, "params": params()}


def optimises_scene():
    """test_it_optimises: a ring of 24 keyframes, keyframe 0 fixed, six points per keyframe seen by three consecutive keyframes, the ring
    closed by the points the last and the first keyframes share; keyframes 0.6 m apart, stereo and mono mixed, 0.3 sigma of noise, the
    points 0.3 m off"""
    K = 24
    c = scene(71, K, [0], pattern("loop", K, ppk=6), "mixed", ring=True, noise=0.3, rot=0.03, trans=0.08, pt_noise=0.3, spacing=0.6)
    c["params"] = params(iterations=10, robust=False)
    return c


def errors_to_truth(c, r):
    """(mean pose rotation error, mean pose translation error, mean point error) of a result's free keyframes and points, and of the input"""
    free = np.nonzero(np.asarray(c["fixed"]) == 0)[0]

    def pe(poses):
        d = [R6.pose_distance(poses[i], c["truth_pose"][i]) for i in free]
        return float(np.mean([a for a, _ in d])), float(np.mean([b for _, b in d]))
    out = pe(r["pose"]) + (float(np.mean(np.linalg.norm(r["point"] - c["truth_point"], axis=1))),)
    inp = pe(np.asarray(c["kf_pose"], F64)) + (float(np.mean(np.linalg.norm(np.asarray(c["xw"], F64) - c["truth_point"], axis=1))),)
    return out, inp


def drop_edges(c, keep):
    c = dict(c)
    for n in ("edge_point", "edge_kf", "edge_feat"):
        c[n] = c[n][keep]
    return c


FORCED = ("stop", "stop_after_trial", "ended_rejected", "stale", "rho_zero", "nan", "iterations0", "all_fixed", "no_fixed", "fixed_middle", "edgeless",
          "fixed_only", "robust")


def forced(name):
    """the cases of the paths random scenes do not take"""
    K = 6
    vis = pattern("dense", K, ppk=8, seed=3)
    if name == "stop":
        c = scene(81, K, [0], vis)
        c["params"] = params(stop=True)
    elif name == "stop_after_trial":                  # the flag reads set after the first trial
        c = scene(82, K, [0], vis)
        c["params"] = params(stop=("after", 1))
    elif name == "ended_rejected":                    # one Gauss-Newton-sized trial from far off, rejected: qmax == max_trials ends the run
        c = scene(84, K, [0], vis, rot=1.0, trans=2.0, pt_noise=2.0)
        c["params"] = params(max_trials=1, user_lambda_init=1e-9)
    elif name == "stale":                             # two such trials, both rejected: the stored chi2 are the second one's
        c = scene(84, K, [0], vis, rot=1.0, trans=2.0, pt_noise=2.0)
        c["params"] = params(max_trials=2, user_lambda_init=1e-9)
    elif name == "rho_zero":                          # 6l's exact case: every error is 0.0 at the input
        c = from_local(LR.forced("exact"))
        c["params"] = params(robust=False)
    elif name == "nan":
        c = scene(84, K, [0], vis)
        c["special"] = 7
        c["xw"][7, 1] = np.nan
    elif name == "iterations0":
        c = scene(85, K, [0], vis)
        c["params"] = params(iterations=0)
    elif name == "all_fixed":                         # P = 0
        c = scene(86, K, range(K), vis)
    elif name == "no_fixed":                          # F = 0: the gauge is free, lambda holds the system
        c = scene(87, K, [], vis)
    elif name == "fixed_middle":
        c = scene(88, K, [2, 3], vis)
    elif name == "edgeless":
        c = scene(89, K, [0], vis, edgeless=(5, len(vis) - 1))
        c["special"] = 5
    elif name == "fixed_only":                        # the first point a fixed keyframe sees keeps its edges on fixed keyframes only
        c = scene(90, K, [0, 4], vis)
        p = int(c["edge_point"][np.nonzero(c["fixed"][c["edge_kf"]] != 0)[0][0]])
        c = drop_edges(c, ~((c["edge_point"] == p) & (c["fixed"][c["edge_kf"]] == 0)))
        c["special"] = p
    elif name == "robust":
        c = scene(91, K, [0], vis, gross=0.15)
        c["params"] = params(robust=True)
    else:
        raise KeyError(name)
    return c


def run_params(c):
    """the case's parameters with an ("after", n) stop turned into the hook the restatement takes"""
    P = dict(c["params"])
    if isinstance(P["stop"], tuple):                  # ("after", n): the flag reads set after the n-th trial
        seen, n = [], P["stop"][1]
        P["stop"] = lambda: seen.append(1) or len(seen) >= n
    return P


def without_points(c, drop):
    """(keep mask, the case without the points listed); their edges must be gone already"""
    keep = np.ones(len(c["xw"]), bool)
    keep[list(drop)] = False
    new = np.cumsum(keep) - 1
    return keep, dict(c, xw=c["xw"][keep], edge_point=new[c["edge_point"]].astype(np.int32))


def over_pairs_case(K=520, L=250):
    """more Schur pair entries than the cap within every other cap: K free keyframes all seeing L points, L K (K + 1) / 2 pairs"""
    c = scene(12, 2, [], [[0, 1]] * L, "mono")
    ep, ek = np.repeat(np.arange(L), K).astype(np.int32), np.tile(np.arange(K), L).astype(np.int32)
    return {"fixed": np.zeros(K, np.uint8), "kf_pose": np.tile(c["kf_pose"][:1], (K, 1)), "kf_cam": np.tile(c["kf_cam"][:1], (K, 1)),
            "kf_nlevels": np.full(K, 4, np.int32), "kf_sigma2": np.tile(c["kf_sigma2"][:1], (K, 1)), "kf_feat_off": (np.arange(K + 1) * L).astype(np.int32),
            "kpts": np.zeros((K * L, 2), F32), "octave": np.zeros(K * L, np.int32), "uright": np.full(K * L, -1, F32), "xw": c["xw"],
            "edge_point": ep, "edge_kf": ek, "edge_feat": ep.copy(), "params": params(iterations=1)}
