"""The contract of DESIGN.md 6o restated in numpy: what rfe_two_view computes, bit for bit.  fp32 with one rounding per operation, the
sums in the orders two_view.hip states; every hypothesis of a problem at once, then the reference's sequential choices
(TwoViewReconstruction.cc:49-1221, GeometricTools::Triangulate).  The sweep counts are arguments, so that the study of departure (a)
can move them; SWEEPS is what the kernels use."""
import numpy as np

from essential_graph_ref import acos_

F32, F64, I32 = np.float32, np.float64, np.int32
SWEEPS = {"H": 9, "F": 10, "S3": 6, "TRI": 6}   # where tests/test_two_view_ref.py sees every output settle (7, 8, 4, 4), plus two
TH_H, TH_F, TH_SCORE = F32(5.991), F32(3.841), F32(5.991)
COS_99998 = F32(float.fromhex("0x1.fffd62p-1"))       # (double)c < 0.99998  <=>  c < COS_99998
RATIO_100001 = F32(float.fromhex("0x1.0000a8p+0"))    # (double)q < 1.00001  <=>  q < RATIO_100001
assert float(np.nextafter(COS_99998, F32(0))) < 0.99998 < float(COS_99998) and float(np.nextafter(RATIO_100001, F32(0))) < 1.00001 < float(RATIO_100001)
FLAG_FEW, FLAG_INDEX, FLAG_NONFINITE = 1, 2, 4
EXIT_OK, EXIT_NO_SCORE, EXIT_SINGULAR, EXIT_NO_WINNER, EXIT_FEW, EXIT_PARALLAX = range(6)
OUT = {"R21": F32, "t21": F32, "p3d": F32, "triangulated": np.uint8, "inliers_h": np.uint8, "inliers_f": np.uint8, "scores": F32,
       "models": F32, "cand": F32, "stats": I32}
ONE, TWO, ZERO = F32(1), F32(2), F32(0)


def params(fx=500.0, fy=500.0, cx=320.0, cy=240.0, sigma=0.0, rh_threshold=0.0, min_parallax=0.0, min_triangulated=0, its=0, n1=0, n2=0):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, sigma=sigma, rh_threshold=rh_threshold, min_parallax=min_parallax,
                min_triangulated=min_triangulated, its=its, n1=n1, n2=n2)


# ---------------------------------------------------------------- 3 x 3 helpers on [..., 9] arrays, sums left to right
def mul3(A, B):
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    return np.stack([(A[..., 3 * r] * B[..., c] + A[..., 3 * r + 1] * B[..., 3 + c]) + A[..., 3 * r + 2] * B[..., 6 + c]
                     for r in range(3) for c in range(3)], -1)


def transpose3(A):
    return np.stack([A[..., 3 * c + r] for r in range(3) for c in range(3)], -1)


def det3(M):
    return (M[..., 0] * (M[..., 4] * M[..., 8] - M[..., 5] * M[..., 7]) - M[..., 1] * (M[..., 3] * M[..., 8] - M[..., 5] * M[..., 6])) + \
        M[..., 2] * (M[..., 3] * M[..., 7] - M[..., 4] * M[..., 6])


def inv3(M):
    """departure (b): the cofactor inverse, every entry divided by the determinant"""
    M = np.asarray(M, F32)
    m = [M[..., k] for k in range(9)]
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    with np.errstate(all="ignore"):
        return np.stack([c00 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                         c01 / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                         c02 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det], -1)


def tmat(T):
    z, o = np.zeros_like(T[..., 0]), np.ones_like(T[..., 0])
    return np.stack([T[..., 0], z, T[..., 2], z, T[..., 1], T[..., 3], z, z, o], -1)


def seqsum(x):
    """left to right along the last axis"""
    acc = x[..., 0]
    for k in range(1, x.shape[-1]):
        acc = acc + x[..., k]
    return acc


# ---------------------------------------------------------------- departure (a): one-sided Jacobi on the columns
TOL2 = F32(2.0 ** -40)   # a pair is rotated unless gamma^2 <= TOL2 alpha beta: columns orthogonal to 2^-20 are left alone


def jacobi(A, sweeps, tol2=None):
    """A [..., m, n] -> the rotated columns and V [..., n, n]: cyclic pairs (p, q), p < q.  tol2 None (the 4 x 4 null vector, as in
    triangulate.hip): a rotation is skipped when the columns' inner product gamma is exactly zero.  Otherwise (9 and 3 columns) it is
    skipped when gamma^2 <= tol2 (alpha beta), so that the iteration reaches a fixed point.  A NaN rotates (and spreads) in both."""
    A = np.array(A, F32)
    n = A.shape[-1]
    V = np.broadcast_to(np.eye(n, dtype=F32), A.shape[:-2] + (n, n)).copy()
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    ap, aq = A[..., p].copy(), A[..., q].copy()
                    alpha, beta, gamma = seqsum(ap * ap), seqsum(aq * aq), seqsum(ap * aq)
                    rot = ((gamma != 0) if tol2 is None else ~(gamma * gamma <= tol2 * (alpha * beta)))[..., None]
                    zeta = (beta - alpha) / (TWO * gamma)
                    t = np.where(zeta >= 0, ONE, -ONE) / (np.abs(zeta) + np.sqrt(ONE + zeta * zeta))
                    c = ONE / np.sqrt(ONE + t * t)
                    s = c * t
                    c, s = c[..., None], s[..., None]
                    A[..., p], A[..., q] = np.where(rot, c * ap - s * aq, ap), np.where(rot, s * ap + c * aq, aq)
                    vp, vq = V[..., p].copy(), V[..., q].copy()
                    V[..., p], V[..., q] = np.where(rot, c * vp - s * vq, vp), np.where(rot, s * vp + c * vq, vq)
    return A, V


def null_vector(A, sweeps, tol2=None):
    """the column of V whose rotated column has the smallest squared norm; the first minimum wins, a NaN norm is never smaller"""
    A, V = jacobi(A, sweeps, tol2)
    nb = seqsum((A[..., 0] * A[..., 0]))
    h = V[..., 0].copy()
    for c in range(1, A.shape[-1]):
        nc = seqsum(A[..., c] * A[..., c])
        less = nc < nb
        nb = np.where(less, nc, nb)
        h = np.where(less[..., None], V[..., c], h)
    return h


def svd3(M, sweeps):
    """M [..., 9] -> U [..., 9], w [..., 3], V [..., 9]: singular values = norms of the rotated columns, sorted descending by a stable
    three-element network; U's columns the rotated columns over their norms, u2 = u0 x u1 where w2 == 0"""
    A, W = jacobi(np.asarray(M, F32).reshape(M.shape[:-1] + (3, 3)), sweeps, TOL2)
    with np.errstate(all="ignore"):
        n = [np.sqrt((A[..., 0, c] * A[..., 0, c] + A[..., 1, c] * A[..., 1, c]) + A[..., 2, c] * A[..., 2, c]) for c in range(3)]
        for a, b in ((0, 1), (1, 2), (0, 1)):
            sw = n[b] > n[a]
            n[a], n[b] = np.where(sw, n[b], n[a]), np.where(sw, n[a], n[b])
            s3 = sw[..., None]
            A[..., a], A[..., b] = np.where(s3, A[..., b], A[..., a]), np.where(s3, A[..., a], A[..., b])
            W[..., a], W[..., b] = np.where(s3, W[..., b], W[..., a]), np.where(s3, W[..., a], W[..., b])
        U = np.stack([A[..., r, c] / n[c] for r in range(3) for c in range(3)], -1)
    V = np.stack([W[..., r, c] for r in range(3) for c in range(3)], -1)
    zero = n[2] == 0
    U[..., 2] = np.where(zero, U[..., 3] * U[..., 7] - U[..., 6] * U[..., 4], U[..., 2])
    U[..., 5] = np.where(zero, U[..., 6] * U[..., 1] - U[..., 0] * U[..., 7], U[..., 5])
    U[..., 8] = np.where(zero, U[..., 0] * U[..., 4] - U[..., 3] * U[..., 1], U[..., 8])
    return U, np.stack(n, -1), V


# ---------------------------------------------------------------- the gates
def check_h(H, Hi, u1, v1, u2, v2, invs2):
    """CheckHomography of matches [..., N] under models [..., 9] (broadcast by the caller): the two score terms and bIn"""
    with np.errstate(all="ignore"):
        w2 = ONE / ((Hi[6] * u2 + Hi[7] * v2) + Hi[8])
        a, b = ((Hi[0] * u2 + Hi[1] * v2) + Hi[2]) * w2, ((Hi[3] * u2 + Hi[4] * v2) + Hi[5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * invs2
        w1 = ONE / ((H[6] * u1 + H[7] * v1) + H[8])
        c, d = ((H[0] * u1 + H[1] * v1) + H[2]) * w1, ((H[3] * u1 + H[4] * v1) + H[5]) * w1
        chi2 = ((u2 - c) * (u2 - c) + (v2 - d) * (v2 - d)) * invs2
        o1, o2 = chi1 > TH_H, chi2 > TH_H
        return np.where(o1, ZERO, TH_H - chi1), np.where(o2, ZERO, TH_H - chi2), ~(o1 | o2)


def check_f(F, u1, v1, u2, v2, invs2):
    with np.errstate(all="ignore"):
        a2, b2, c2 = (F[0] * u1 + F[1] * v1) + F[2], (F[3] * u1 + F[4] * v1) + F[5], (F[6] * u1 + F[7] * v1) + F[8]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * invs2
        a1, b1, c1 = (F[0] * u2 + F[3] * v2) + F[6], (F[1] * u2 + F[4] * v2) + F[7], (F[2] * u2 + F[5] * v2) + F[8]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * invs2
        o1, o2 = chi1 > TH_F, chi2 > TH_F
        return np.where(o1, ZERO, TH_SCORE - chi1), np.where(o2, ZERO, TH_SCORE - chi2), ~(o1 | o2)


def check(model, M, pts, sigma=1.0):
    """the hook rfe_k_two_view_check: ONE model M [9] over pts [n,4] -> contrib [n] (0 + term1 + term2), inl [n]"""
    M, pts = np.asarray(M, F32), np.asarray(pts, F32).reshape(-1, 4)
    s2 = F32(sigma) * F32(sigma)
    invs2 = ONE / s2
    u1, v1, u2, v2 = (pts[:, k] for k in range(4))
    t1, t2, inl = check_h(M, inv3(M), u1, v1, u2, v2, invs2) if model == 0 else check_f(M, u1, v1, u2, v2, invs2)
    return (ZERO + t1) + t2, inl.astype(np.uint8)


def check_rt(R, t, fx, fy, cx, cy, th2, u1, v1, u2, v2, sweeps=None):
    """CheckRT of matches [N] under motion hypotheses R [C,9], t [C,3]: code [C,N] (0 not counted, 1 counted without vbGood, 2 counted
    and vbGood), cosParallax [C,N], p [C,N,3]"""
    sweeps = SWEEPS["TRI"] if sweeps is None else sweeps
    R, t = np.asarray(R, F32).reshape(-1, 9, 1), np.asarray(t, F32).reshape(-1, 3, 1)
    fx, fy, cx, cy, th2 = F32(fx), F32(fy), F32(cx), F32(cy), F32(th2)
    C, N = R.shape[0], len(u1)
    u1, v1, u2, v2 = (np.broadcast_to(np.asarray(x, F32)[None, :], (C, N)) for x in (u1, v1, u2, v2))
    with np.errstate(all="ignore"):
        P1 = [[fx, ZERO, cx, ZERO], [ZERO, fy, cy, ZERO], [ZERO, ZERO, ONE, ZERO]]
        A = np.zeros((C, N, 4, 4), F32)
        for c in range(4):
            r0, r1, r2 = (R[:, c], R[:, 3 + c], R[:, 6 + c]) if c < 3 else (t[:, 0], t[:, 1], t[:, 2])
            p20 = (fx * r0 + ZERO * r1) + cx * r2
            p21 = (ZERO * r0 + fy * r1) + cy * r2
            p22 = (ZERO * r0 + ZERO * r1) + ONE * r2
            A[..., 0, c] = u1 * P1[2][c] - P1[0][c]
            A[..., 1, c] = v1 * P1[2][c] - P1[1][c]
            A[..., 2, c] = u2 * p22 - p20
            A[..., 3, c] = v2 * p22 - p21
        h = null_vector(A, sweeps, TOL2)
        ok = h[..., 3] != 0                                               # departure (e)
        p = np.stack([h[..., 0] / h[..., 3], h[..., 1] / h[..., 3], h[..., 2] / h[..., 3]], -1)
        p = np.where(ok[..., None], p, ZERO)
        fin = np.isfinite(p).all(-1)
        O2 = [-((R[:, k] * t[:, 0] + R[:, 3 + k] * t[:, 1]) + R[:, 6 + k] * t[:, 2]) for k in range(3)]
        dist1 = np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
        n2 = [p[..., k] - O2[k] for k in range(3)]
        dist2 = np.sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2])
        cosp = ((p[..., 0] * n2[0] + p[..., 1] * n2[1]) + p[..., 2] * n2[2]) / (dist1 * dist2)
        below = cosp < COS_99998
        alive = ok & fin
        alive &= ~((p[..., 2] <= 0) & below)
        x2 = ((R[:, 0] * p[..., 0] + R[:, 1] * p[..., 1]) + R[:, 2] * p[..., 2]) + t[:, 0]
        y2 = ((R[:, 3] * p[..., 0] + R[:, 4] * p[..., 1]) + R[:, 5] * p[..., 2]) + t[:, 1]
        z2 = ((R[:, 6] * p[..., 0] + R[:, 7] * p[..., 1]) + R[:, 8] * p[..., 2]) + t[:, 2]
        alive &= ~((z2 <= 0) & below)
        iz1 = ONE / p[..., 2]
        e1x, e1y = ((fx * p[..., 0]) * iz1 + cx) - u1, ((fy * p[..., 1]) * iz1 + cy) - v1
        alive &= ~(e1x * e1x + e1y * e1y > th2)
        iz2 = ONE / z2
        e2x, e2y = ((fx * x2) * iz2 + cx) - u2, ((fy * y2) * iz2 + cy) - v2
        alive &= ~(e2x * e2x + e2y * e2y > th2)
    code = np.where(alive, np.where(below, 2, 1), 0).astype(np.uint8)
    # what the kernel leaves in its workspace where it returned early: the cosine and point as far as they had been formed
    formed = ok & fin
    cosp = np.where(formed, cosp, ZERO).astype(F32)
    return code, cosp, p.astype(F32)


# ---------------------------------------------------------------- the front
def block_sum(x):
    """256 thread-strided partials in element order, then the tree s = 128 .. 1 with v[t] = v[t] + v[t + s]"""
    x = np.asarray(x, F32)
    pad = (-len(x)) % 256
    x = np.concatenate([x, np.zeros(pad, F32)]).reshape(-1, 256)
    v = np.zeros(256, F32)
    for row in x:
        v = v + row
    s = 128
    while s >= 1:
        v[:s] = v[:s] + v[s:2 * s]
        s >>= 1
    return v[0]


def normalize(k):
    """Normalize (:949-1000) over ALL n keypoints: (sX, sY, -meanX sX, -meanY sY)"""
    k = np.asarray(k, F32).reshape(-1, 2)
    n = F32(len(k))
    with np.errstate(all="ignore"):
        mx, my = block_sum(k[:, 0]) / n, block_sum(k[:, 1]) / n
        ax, ay = block_sum(np.abs(k[:, 0] - mx)) / n, block_sum(np.abs(k[:, 1] - my)) / n
        sx, sy = ONE / ax, ONE / ay
        return np.array([sx, sy, -mx * sx, -my * sy], F32)


def resolve_draws(d, N):
    """one iteration's 8 raw rand() results -> its 8-set, through the swap-with-back list of :99-115 kept as its displaced entries"""
    pos, val, out = [], [], []
    for j in range(8):
        sz = N - j
        r = int((float(int(d[j])) / 2147483648.0) * float(sz))
        r = min(max(r, 0), sz - 1)
        idx, back = r, sz - 1
        for e in range(j):
            if pos[e] == r:
                idx = val[e]
            if pos[e] == sz - 1:
                back = val[e]
        pos.append(r)
        val.append(back)
        out.append(idx)
    return out


def lane_tree_score(t1, t2, N):
    """t1, t2 [its, N] the two terms of every match: lane l of 64 takes the matches 4 (l + 64 j) .. + 3 in order, adding both terms of
    each; then the tree d = 32 .. 1 with v[l] = v[l] + v[l + d]"""
    its = t1.shape[0]
    pad = (-N) % 256
    x = np.stack([t1, t2], -1)
    x = np.concatenate([x, np.zeros((its, pad, 2), F32)], 1).reshape(its, -1, 64, 4, 2).transpose(0, 2, 1, 3, 4).reshape(its, 64, -1)
    v = np.zeros((its, 64), F32)
    for k in range(x.shape[-1]):
        v = v + x[..., k]
    d = 32
    while d >= 1:
        v[:, :d] = v[:, :d] + v[:, d:2 * d]
        d >>= 1
    return v[:, 0].copy()


def key_of(c):
    u = np.ascontiguousarray(c, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def parallax_of(cos_counted):
    """the min(50, size - 1)-th smallest cosine in the total order of the bit patterns, as degrees: departure (c)"""
    if len(cos_counted) == 0:
        return ZERO
    c = np.asarray(cos_counted, F32)
    cv = c[np.argsort(key_of(c), kind="stable")][min(50, len(c) - 1)]
    return F32((np.asarray(acos_(F64(cv))).reshape(-1)[0] * 180.0) / 3.141592653589793)


# ---------------------------------------------------------------- the call, one problem
def two_view(P, kpts1, kpts2, S, pairs, draws, fill=None, sweeps=None, detail=False):
    """rfe_two_view for one problem: kpts1 [N1max,2], kpts2 [N2max,2], S, pairs [Kmax,2], draws [H,8] -> the dict of OUT.  fill: what
    the arrays hold where the call does not write (default 0)."""
    sw = dict(SWEEPS, **(sweeps or {}))
    kpts1, kpts2 = np.asarray(kpts1, F32).reshape(-1, 2), np.asarray(kpts2, F32).reshape(-1, 2)
    pairs, draws = np.asarray(pairs, I32).reshape(-1, 2), np.asarray(draws, I32).reshape(-1, 8)
    N1max, Kmax, H = len(kpts1), len(pairs), len(draws)
    shape = {"R21": (9,), "t21": (3,), "p3d": (N1max, 3), "triangulated": (N1max,), "inliers_h": (Kmax,), "inliers_f": (Kmax,),
             "scores": (H, 2), "models": (2, 9), "cand": (8, 16), "stats": (16,)}
    o = {k: np.zeros(shape[k], OUT[k]) for k in OUT}
    for k, v in (fill or {}).items():
        o[k][...] = v
    n1, n2 = int(P["n1"]), int(P["n2"])
    N = min(max(int(S), 0), Kmax)
    its = 200 if int(P["its"]) == 0 else int(P["its"])
    assert its <= H
    sigma = ONE if F32(P["sigma"]) == 0 else F32(P["sigma"])
    sigma2 = sigma * sigma
    invs2, th2 = ONE / sigma2, F32(4) * sigma2
    rh_thr = F32(0.5) if F32(P["rh_threshold"]) == 0 else F32(P["rh_threshold"])
    min_par = ONE if F32(P["min_parallax"]) == 0 else F32(P["min_parallax"])
    min_tri = 50 if int(P["min_triangulated"]) == 0 else int(P["min_triangulated"])
    fx, fy, cx, cy = (F32(P[k]) for k in ("fx", "fy", "cx", "cy"))
    i, j = pairs[:N, 0], pairs[:N, 1]
    ok = (i >= 0) & (i < n1) & (j >= 0) & (j < n2)
    flags = (FLAG_FEW if N < 8 else 0) | (FLAG_INDEX if not ok.all() else 0)
    T1, T2 = normalize(kpts1[:n1]), normalize(kpts2[:n2])
    T1m, T2m = tmat(T1), tmat(T2)
    T2inv = inv3(T2m)
    if flags:
        its_run = 0
        u1 = v1 = u2 = v2 = np.zeros(N, F32)
    else:
        its_run = its
        u1, v1, u2, v2 = kpts1[i, 0], kpts1[i, 1], kpts2[j, 0], kpts2[j, 1]
    hm = np.zeros((its_run, 2, 9), F32)
    sc = np.zeros((its_run, 2), F32)
    sets = np.zeros((its_run, 8), np.int64)
    if its_run:
        sets = np.array([resolve_draws(draws[h], N) for h in range(its)], np.int64)
        with np.errstate(all="ignore"):
            a1, b1 = u1[sets] * T1[0] + T1[2], v1[sets] * T1[1] + T1[3]       # [its, 8]
            a2, b2 = u2[sets] * T2[0] + T2[2], v2[sets] * T2[1] + T2[3]
            z, one = np.zeros_like(a1), np.ones_like(a1)
            even = np.stack([z, z, z, -a1, -b1, -one, b2 * a1, b2 * b1, b2], -1)
            odd = np.stack([a1, b1, one, z, z, z, -a2 * a1, -a2 * b1, -a2], -1)
            AH = np.stack([even, odd], 2).reshape(its, 16, 9)
            AF = np.stack([a2 * a1, a2 * b1, a2, b2 * a1, b2 * b1, b2, a1, b1, one], -1)
            Hn, Fpre = null_vector(AH, sw["H"], TOL2), null_vector(AF, sw["F"], TOL2)
            hm[:, 0] = mul3(mul3(T2inv, Hn), T1m)
            U, w, V = svd3(Fpre, sw["S3"])
            Fn = np.stack([(U[:, 3 * r] * w[:, 0]) * V[:, 3 * c] + (U[:, 3 * r + 1] * w[:, 1]) * V[:, 3 * c + 1] for r in range(3) for c in range(3)], -1)
            hm[:, 1] = mul3(mul3(transpose3(T2m), Fn), T1m)
            Hm = [hm[:, 0, k][:, None] for k in range(9)]
            Hi = inv3(hm[:, 0])
            Hi = [Hi[:, k][:, None] for k in range(9)]
            Fm = [hm[:, 1, k][:, None] for k in range(9)]
            pts = [x[None, :] for x in (u1, v1, u2, v2)]
            t1, t2, _ = check_h(Hm, Hi, *pts, invs2)
            sc[:, 0] = lane_tree_score(t1, t2, N)
            t1, t2, _ = check_f(Fm, *pts, invs2)
            sc[:, 1] = lane_tree_score(t1, t2, N)
        o["scores"][:its] = sc
    # the first maximum of each model; a NaN never wins
    best, win = [ZERO, ZERO], [-1, -1]
    for m in range(2):
        for h in range(its_run):
            if sc[h, m] > best[m]:
                best[m], win[m] = sc[h, m], h
    if not np.isfinite(sc).all():
        flags |= FLAG_NONFINITE
    Mw = [hm[win[m], m] if win[m] >= 0 else np.zeros(9, F32) for m in range(2)]
    inl = [np.zeros(N, bool), np.zeros(N, bool)]
    if win[0] >= 0:
        inl[0] = check_h(Mw[0], inv3(Mw[0]), u1, v1, u2, v2, invs2)[2]
    if win[1] >= 0:
        inl[1] = check_f(Mw[1], u1, v1, u2, v2, invs2)[2]
    o["inliers_h"][:N], o["inliers_f"][:N] = inl[0], inl[1]
    o["models"][0], o["models"][1] = Mw
    SH, SF = best
    RH, model, exit_code, chosen = ZERO, 0, EXIT_OK, -1
    candR, candt = np.zeros((0, 9), F32), np.zeros((0, 3), F32)
    Km = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], F32)
    with np.errstate(all="ignore"):
        if SH + SF == 0:
            exit_code = EXIT_NO_SCORE
        else:
            RH = SH / (SH + SF)
            if RH > rh_thr:
                model = 1
                A = mul3(mul3(inv3(Km), Mw[0]), Km)
                U, w, V = svd3(A, sw["S3"])
                Vt = transpose3(V)
                s = det3(U) * det3(Vt)
                d1, d2, d3 = w
                if d1 / d2 < RATIO_100001 or d2 / d3 < RATIO_100001:
                    exit_code = EXIT_SINGULAR
                else:
                    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
                    aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
                    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
                    root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
                    aux_st, ctheta = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
                    aux_sp, cphi = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
                    sgn = [ONE, -ONE, -ONE, ONE]
                    sU = s * U
                    Rs, ts = [], []
                    for c in range(8):
                        k, second = c & 3, c >= 4
                        sn = sgn[k] * (aux_sp if second else aux_st)
                        Rp = np.array([cphi, 0, sn, 0, -1, 0, sn, 0, -cphi] if second else [ctheta, 0, -sn, 0, 1, 0, sn, 0, ctheta], F32)
                        Rs.append(mul3(mul3(sU, Rp), Vt))
                        scale = d1 + d3 if second else d1 - d3
                        tp = [x1[k] * scale, ZERO * scale, (x3[k] if second else -x3[k]) * scale]
                        t = [(U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2] for r in range(3)]
                        nrm = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
                        ts.append(np.array([t[0] / nrm, t[1] / nrm, t[2] / nrm], F32))
                    candR, candt = np.array(Rs, F32), np.array(ts, F32)
            else:
                model = 2
                A = mul3(mul3(transpose3(Km), Mw[1]), Km)
                U, w, V = svd3(A, sw["S3"])
                Vt = transpose3(V)
                nrm = np.sqrt((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8])
                t = np.array([U[2] / nrm, U[5] / nrm, U[8] / nrm], F32)
                UW = np.array([U[1], -U[0], U[2], U[4], -U[3], U[5], U[7], -U[6], U[8]], F32)
                R1 = mul3(UW, Vt)
                if det3(R1) < 0:
                    R1 = -R1
                UWt = np.array([-U[1], U[0], U[2], -U[4], U[3], U[5], -U[7], U[6], U[8]], F32)
                R2 = mul3(UWt, Vt)
                if det3(R2) < 0:
                    R2 = -R2
                candR, candt = np.array([R1, R2, R1, R2], F32), np.array([t, t, -t, -t], F32)
    ncand = len(candR)
    good, par = [0] * ncand, [ZERO] * ncand
    code = np.zeros((ncand, N), np.uint8)
    pts3 = np.zeros((ncand, N, 3), F32)
    if ncand:
        sel = inl[model - 1]
        code, cosp, pts3 = check_rt(candR, candt, fx, fy, cx, cy, th2, u1, v1, u2, v2, sw["TRI"])
        code = np.where(sel[None, :], code, 0).astype(np.uint8)
        for c in range(ncand):
            good[c] = int((code[c] != 0).sum())
            par[c] = parallax_of(cosp[c][code[c] != 0])
        Ninl = int(sel.sum())
        if model == 2:
            maxGood = max(good)
            nMinGood = max(int(0.9 * Ninl), min_tri)
            nsimilar = sum(1 for g in good if g > 0.7 * maxGood)
            if maxGood < nMinGood:
                exit_code = EXIT_FEW
            elif nsimilar > 1:
                exit_code = EXIT_NO_WINNER
            else:
                c = good.index(maxGood)
                if par[c] > min_par:
                    chosen = c
                else:
                    exit_code = EXIT_PARALLAX
        else:
            bestGood, second, bestIdx, bestPar = 0, 0, -1, F32(-1)
            for c in range(8):
                if good[c] > bestGood:
                    second, bestGood, bestIdx, bestPar = bestGood, good[c], c, par[c]
                elif good[c] > second:
                    second = good[c]
            if not second < 0.75 * bestGood:
                exit_code = EXIT_NO_WINNER
            elif not bestPar >= min_par:
                exit_code = EXIT_PARALLAX
            elif not (bestGood > min_tri and bestGood > 0.9 * Ninl):
                exit_code = EXIT_FEW
            else:
                chosen = bestIdx
        for c in range(ncand):
            o["cand"][c] = np.concatenate([candR[c], candt[c], np.array([good[c], float(par[c]), 0, 0], F32)])
    o["R21"][:] = candR[chosen] if chosen >= 0 else np.eye(3, dtype=F32).reshape(-1)
    o["t21"][:] = candt[chosen] if chosen >= 0 else 0
    o["p3d"][:n1], o["triangulated"][:n1] = 0, 0
    if chosen >= 0:
        m = code[chosen] != 0
        o["p3d"][i[m]] = pts3[chosen][m]
        o["triangulated"][i[m]] = code[chosen][m] == 2
    bits = lambda v: int(np.array(v, F32).view(I32))   # noqa: E731
    o["stats"][:13] = [int(chosen >= 0), model, N, win[0], win[1], int(inl[0].sum()), int(inl[1].sum()), chosen, bits(SH), bits(SF), bits(RH),
                       exit_code, flags]
    o["stats"][13:] = 0
    if detail:
        o["_detail"] = {"sets": sets, "good": good, "parallax": par, "RH": float(RH), "SH": float(SH), "SF": float(SF)}
    return o


# ---------------------------------------------------------------- planted scenes
def rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


KINDS = {   # R21 as (axis, degrees) pairs, t21, rh_threshold: what tests/test_two_view_ref.py chose on the CPU
    "general": dict(R=(("y", 4.0), ("x", -2.0)), t=(1.0, 0.1, 0.2), rh=0.0),
    "plane": dict(R=(("y", 3.0), ("z", 2.0)), t=(1.5, 0.3, -0.8), rh=0.3),        # the plane z = 3 + 0.7 x + 0.3 y of scene()
    "rotation": dict(R=(("y", 8.0), ("x", 3.0)), t=(0.0, 0.0, 0.0), rh=0.55),
    "rotation_h": dict(R=(("y", 8.0), ("x", 3.0)), t=(0.0, 0.0, 0.0), rh=0.3),
    "low_parallax": dict(R=(("y", 1.0),), t=(0.09, 0.01, 0.0), rh=0.0),
}


def scene(seed, n=300, kind="general", noise=0.2, outliers=0.05, its=200, extra1=17, extra2=29, plane=(0.7, 0.3, 3.0), **over):
    """n matches between two views of a planted scene, `extra` unmatched keypoints per frame, shuffled indices (i ascending); the case
    dict of two_view(): P, kpts1, kpts2, S, pairs, draws, and the planted R, t"""
    g = np.random.default_rng(seed)
    K = KINDS[kind]
    fx = fy = 500.0
    cx, cy = 320.0, 240.0
    uv = np.stack([g.uniform(20, 620, n), g.uniform(20, 460, n)], 1)
    xn, yn = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    z = plane[2] / (1.0 - plane[0] * xn - plane[1] * yn) if kind == "plane" else g.uniform(6.0, 10.0, n)
    X = np.stack([xn * z, yn * z, z], 1)
    Rm = np.eye(3)
    for ax, deg in K["R"]:
        Rm = rot(ax, deg) @ Rm
    t = np.array(K["t"], F64)
    X2 = X @ Rm.T + t
    uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    uv, uv2 = uv + g.normal(0, noise, uv.shape), uv2 + g.normal(0, noise, uv2.shape)
    bad = g.random(n) < outliers
    uv2[bad] = np.stack([g.uniform(0, 640, bad.sum()), g.uniform(0, 480, bad.sum())], 1)
    n1, n2 = n + extra1, n + extra2
    i = np.sort(g.choice(n1, n, replace=False))
    j = g.permutation(n2)[:n]
    k1 = np.stack([g.uniform(0, 640, n1), g.uniform(0, 480, n1)], 1)
    k2 = np.stack([g.uniform(0, 640, n2), g.uniform(0, 480, n2)], 1)
    k1[i], k2[j] = uv, uv2
    P = params(fx=fx, fy=fy, cx=cx, cy=cy, rh_threshold=K["rh"], its=its, n1=n1, n2=n2)
    P.update(over)
    return {"P": P, "kpts1": k1.astype(F32), "kpts2": k2.astype(F32), "S": n, "pairs": np.stack([i, j], 1).astype(I32),
            "draws": g.integers(0, 2 ** 31, (its if its else 200, 8)).astype(I32), "R": Rm, "t": t}


def run(c, **kw):
    return two_view(c["P"], c["kpts1"], c["kpts2"], c["S"], c["pairs"], c["draws"], **kw)


# ---------------------------------------------------------------- forced paths: name -> (case, what stats must say)
def forced(name):
    """the case of a forced path and the (ret, model, exit, flags) its stats must show (None: not pinned)"""
    if name == "s7":                                                      # departure (d)
        c = scene(11, n=7, its=5)
        return c, (0, 0, EXIT_NO_SCORE, FLAG_FEW)
    if name == "nan_keypoint":                                            # an UNMATCHED keypoint: Normalize spreads it to every score
        c = scene(12, its=5)
        free = np.setdiff1d(np.arange(c["P"]["n2"]), c["pairs"][:, 1])
        c["kpts2"][free[0], 1] = np.nan
        return c, (0, 0, EXIT_NO_SCORE, FLAG_NONFINITE)
    if name == "identical_sets":                                          # equal scores: the first wins
        c = scene(13, its=4, noise=0.0, outliers=0.0)
        c["draws"][1:4] = c["draws"][0]
        return c, (None, 2, None, 0)
    if name == "p2_equals_p1":                                            # H21 = I: the singular-value exit of ReconstructH
        c = scene(14, its=5, outliers=0.0, rh_threshold=0.1)
        c["kpts2"][c["pairs"][:, 1]] = c["kpts1"][c["pairs"][:, 0]]
        return c, (0, 1, EXIT_SINGULAR, 0)
    if name == "index_out_of_range":
        c = scene(15, its=5)
        c["pairs"][100, 1] = c["P"]["n2"]
        return c, (0, 0, EXIT_NO_SCORE, FLAG_INDEX)
    table = {"f_success": ("general", {}, (1, 2, EXIT_OK, 0)), "f_few": ("general", {"min_triangulated": 4000}, (0, 2, EXIT_FEW, 0)),
             "f_no_winner": ("rotation", {}, (0, 2, EXIT_NO_WINNER, 0)), "f_parallax": ("low_parallax", {}, (0, 2, EXIT_PARALLAX, 0)),
             "h_success": ("plane", {}, (1, 1, EXIT_OK, 0)), "h_few": ("plane", {"min_triangulated": 4000}, (0, 1, EXIT_FEW, 0)),
             "h_no_winner": ("rotation_h", {}, (0, 1, EXIT_NO_WINNER, 0)), "h_parallax": ("plane", {"min_parallax": 60.0}, (0, 1, EXIT_PARALLAX, 0))}
    kind, over, want = table[name]
    return scene(16, kind=kind, its=60, **over), want


FORCED = ("s7", "nan_keypoint", "identical_sets", "p2_equals_p1", "index_out_of_range", "f_success", "f_few", "f_no_winner", "f_parallax",
          "h_success", "h_few", "h_no_winner", "h_parallax")
