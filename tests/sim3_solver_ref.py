"""The contract of DESIGN.md 6j (Sim3Solver, reference src/Sim3Solver.cc:61-483) restated in numpy, operation by operation: what
rfe_sim3_ransac computes, bit for bit.  Three forms live here:
  * sim3_ransac():  the vectorised restatement -- every hypothesis at once, then "the first count above min_inliers, otherwise the last
                    maximum".  The GPU tests compare against this one.
  * Sequential:     a scalar transcription of the cited lines as the reference runs them: np.float32 scalars, a real vAvailableIndices
                    list with swap and pop, the iterate(n) loop with mnBestInliers carried across chunks.  mode="contract" makes the
                    contract's choices and must equal sim3_ransac() in every bit; mode="reference" makes the reference's own
                    (numpy.linalg.eigh on float64, the angle-axis / half-angle sin cos route, float64 sums) and measures departures (a)-(c).
  * scene() / forced(): planted problems and the forced paths both test files run."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
HYP_NAN, HYP_CLAMPED = 1, 8
FLAG_FEW, FLAG_BELOW_THREE, FLAG_CLAMPED = 1, 2, 8
INT_MIN = -2 ** 31
OUT = {"T12": F32, "R": F32, "t": F32, "s": F32, "inliers": np.uint8, "best_inliers": np.uint8, "counts": np.int32, "hyps": F32,
       "stats": np.int32}
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ---------------------------------------------------------------- SetRansacParameters (:126-150)
def ransac_iterations(probability, min_inliers, n, max_its):
    if min_inliers == n:
        it = 1
    else:
        with np.errstate(**_ERR):
            epsilon = float(F32(min_inliers) / F32(n))
        try:
            v = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(epsilon, 3)))
        except (ValueError, ZeroDivisionError, OverflowError):     # what the C library answers with NaN or an infinity
            v = None
        it = v if v is not None and INT_MIN <= v <= 2 ** 31 - 1 else INT_MIN
    return max(1, min(it, max_its))


def params(rcw1, tcw1, rcw2, tcw2, cam1, cam2, fix_scale, min_inliers, its, n):
    return {"rcw1": np.asarray(rcw1, F32).reshape(3, 3), "tcw1": np.asarray(tcw1, F32).reshape(3), "rcw2": np.asarray(rcw2, F32).reshape(3, 3),
            "tcw2": np.asarray(tcw2, F32).reshape(3), "cam1": np.asarray(cam1, F32), "cam2": np.asarray(cam2, F32), "fix_scale": int(fix_scale),
            "min_inliers": int(min_inliers), "its": int(its), "n": int(n)}


# ---------------------------------------------------------------- the vectorised restatement
def dot3(a0, a1, a2, x, y, z):
    return (a0 * x + a1 * y) + a2 * z


def project(cam, x, y, z):
    """Pinhole::project (src/CameraModels/Pinhole.cpp:61-68)"""
    return (cam[0] * x) / z + cam[2], (cam[1] * y) / z + cam[3]


def bound(sigma2):
    """mvnMaxError is a vector<size_t> (:102-103, include/Sim3Solver.h:78-79): the double product truncated, compared as a float"""
    return (9.210 * np.asarray(sigma2, F32).astype(F64)).astype(np.uint64).astype(F32)


def front(P, xw1, xw2, s1, s2):
    """:61-121 for the n correspondences handed in"""
    with np.errstate(**_ERR):
        out = {}
        for side, xw, R, t, cam, sg in ((1, xw1, P["rcw1"], P["tcw1"], P["cam1"], s1), (2, xw2, P["rcw2"], P["tcw2"], P["cam2"], s2)):
            x, y, z = (np.asarray(xw, F32)[:, k] for k in range(3))
            X = np.stack([dot3(R[r, 0], R[r, 1], R[r, 2], x, y, z) + t[r] for r in range(3)], 1)
            u, v = project(cam, X[:, 0], X[:, 1], X[:, 2])
            out[f"X{side}"], out[f"p{side}"], out[f"max{side}"] = X, np.stack([u, v], 1), bound(sg)
        return out


def resolve_draws(draws, n):
    """the three reads of vAvailableIndices (:175-189) without the list: at most two entries are displaced.  [H,3] indices, [H] clamped"""
    d = np.asarray(draws, np.int64).reshape(-1, 3)
    r = [np.clip(d[:, k], 0, n - 1 - k) for k in range(3)]
    clamped = (r[0] != d[:, 0]) | (r[1] != d[:, 1]) | (r[2] != d[:, 2])
    back1 = np.where(r[0] == n - 2, n - 1, n - 2)
    i1 = np.where(r[1] == r[0], n - 1, r[1])
    i2 = np.where(r[2] == r[1], back1, np.where(r[2] == r[0], n - 1, r[2]))
    return np.stack([r[0], i1, i2], 1), clamped


def jacobi_quaternion(Nf):
    """departure (a): [H,4,4] float32 symmetric -> [H,4] float32 (w, x, y, z), and the eigenvalue (double)"""
    A = np.array(Nf, F64)
    H = A.shape[0]
    V = np.zeros((H, 4, 4), F64)
    V[:, range(4), range(4)] = 1.0
    for _ in range(SWEEPS):
        for p, r in PAIRS:
            apq = A[:, p, r].copy()
            rot = apq != 0.0
            theta = (A[:, r, r] - A[:, p, p]) / (2.0 * apq)
            tt = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(tt * tt + 1.0)
            s = tt * c
            app, arr = A[:, p, p] - tt * apq, A[:, r, r] + tt * apq
            for k in range(4):
                if k != p and k != r:
                    akp, akr = A[:, k, p].copy(), A[:, k, r].copy()
                    np_, nr = c * akp - s * akr, s * akp + c * akr
                    A[:, k, p] = A[:, p, k] = np.where(rot, np_, akp)
                    A[:, k, r] = A[:, r, k] = np.where(rot, nr, akr)
                vkp, vkr = V[:, k, p].copy(), V[:, k, r].copy()
                V[:, k, p] = np.where(rot, c * vkp - s * vkr, vkp)
                V[:, k, r] = np.where(rot, s * vkp + c * vkr, vkr)
            A[:, p, p] = np.where(rot, app, A[:, p, p])
            A[:, r, r] = np.where(rot, arr, A[:, r, r])
            A[:, p, r] = A[:, r, p] = np.where(rot, 0.0, apq)
    best, v = A[:, 0, 0].copy(), V[:, :, 0].copy()
    for c in range(1, 4):
        more = A[:, c, c] > best
        best = np.where(more, A[:, c, c], best)
        v = np.where(more[:, None], V[:, :, c], v)
    nrm = np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + v[:, 3] * v[:, 3])
    v = v / nrm[:, None]
    neg = (v[:, 0] < 0) | ((v[:, 0] == 0) & ((v[:, 1] < 0) | ((v[:, 1] == 0) & ((v[:, 2] < 0) | ((v[:, 2] == 0) & (v[:, 3] < 0))))))
    return np.where(neg[:, None], -v, v).astype(F32), best


def horn_n(Pr1, Pr2):
    """M (:336) and N (:343-357): [H,3,3] x 2 -> [H,4,4] float32"""
    M = [[(Pr2[:, r, 0] * Pr1[:, c, 0] + Pr2[:, r, 1] * Pr1[:, c, 1]) + Pr2[:, r, 2] * Pr1[:, c, 2] for c in range(3)] for r in range(3)]
    m = [[M[r][c].astype(F64) for c in range(3)] for r in range(3)]
    N11, N12, N13, N14 = (m[0][0] + m[1][1]) + m[2][2], m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]
    N22, N23, N24 = (m[0][0] - m[1][1]) - m[2][2], m[0][1] + m[1][0], m[2][0] + m[0][2]
    N33, N34, N44 = (-m[0][0] + m[1][1]) - m[2][2], m[1][2] + m[2][1], (-m[0][0] - m[1][1]) + m[2][2]
    rows = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    return np.stack([np.stack([e.astype(F32) for e in row], 1) for row in rows], 1)


def quat_to_rotation(q):
    """departure (b): Eigen's toRotationMatrix products on the float (w, x, y, z); NaN where the vector part has norm exactly 0"""
    w, x, y, z = (q[:, k] for k in range(4))
    nan_rot = np.sqrt((x * x + y * y) + z * z) == 0
    tx, ty, tz = F32(2.0) * x, F32(2.0) * y, F32(2.0) * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = F32(1.0)
    R = np.stack([one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)], 1)
    R[nan_rot] = np.nan
    return R.reshape(-1, 3, 3).astype(F32), nan_rot


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 (:319-420) for [H,3,3] triples (columns are the points): R [H,3,3], t [H,3], s [H], nan_rot [H]"""
    with np.errstate(**_ERR):
        three = F32(3.0)
        O1 = ((P1[:, :, 0] + P1[:, :, 1]) + P1[:, :, 2]) / three
        O2 = ((P2[:, :, 0] + P2[:, :, 1]) + P2[:, :, 2]) / three
        Pr1, Pr2 = P1 - O1[:, :, None], P2 - O2[:, :, None]
        q, _ = jacobi_quaternion(horn_n(Pr1, Pr2))
        R, nan_rot = quat_to_rotation(q)
        P3 = np.stack([np.stack([(R[:, r, 0] * Pr2[:, 0, k] + R[:, r, 1] * Pr2[:, 1, k]) + R[:, r, 2] * Pr2[:, 2, k] for k in range(3)], 1)
                       for r in range(3)], 1)
        if fix_scale:
            s = np.ones(len(P1), F32)
        else:
            nom, den = np.zeros(len(P1), F32), np.zeros(len(P1), F32)
            for k in range(3):
                for r in range(3):
                    nom = nom + Pr1[:, r, k] * P3[:, r, k]
                    den = den + P3[:, r, k] * P3[:, r, k]
            s = (nom.astype(F64) / den.astype(F64)).astype(F32)
        t = np.stack([O1[:, r] - dot3(s * R[:, r, 0], s * R[:, r, 1], s * R[:, r, 2], O2[:, 0], O2[:, 1], O2[:, 2]) for r in range(3)], 1)
        return R, t.astype(F32), s, nan_rot


def transforms(R, s, t):
    """:406-419: sR, sRinv, tinv"""
    with np.errstate(**_ERR):
        inv = (1.0 / s.astype(F64)).astype(F32)
        sR = s[:, None, None] * R
        sRi = inv[:, None, None] * R.transpose(0, 2, 1)
        ti = np.stack([-dot3(sRi[:, r, 0], sRi[:, r, 1], sRi[:, r, 2], t[:, 0], t[:, 1], t[:, 2]) for r in range(3)], 1)
        return sR, sRi, ti


def errors(P, f, sR, t, sRi, ti):
    """CheckInliers' e1, e2 (:423-447, Project :469-483): [H,n] each"""
    with np.errstate(**_ERR):
        X1, X2 = f["X1"][None], f["X2"][None]
        Y = [dot3(sR[:, r, 0, None], sR[:, r, 1, None], sR[:, r, 2, None], X2[..., 0], X2[..., 1], X2[..., 2]) + t[:, r, None] for r in range(3)]
        u, v = project(P["cam1"], *Y)
        d1x, d1y = f["p1"][None, :, 0] - u, f["p1"][None, :, 1] - v
        Z = [dot3(sRi[:, r, 0, None], sRi[:, r, 1, None], sRi[:, r, 2, None], X1[..., 0], X1[..., 1], X1[..., 2]) + ti[:, r, None] for r in range(3)]
        u, v = project(P["cam2"], *Z)
        d2x, d2y = u - f["p2"][None, :, 0], v - f["p2"][None, :, 1]
        return d1x * d1x + d1y * d1y, d2x * d2x + d2y * d2y


def hypotheses(P, f, draws, n):
    """every hypothesis h < its: a dict of [its, ...] arrays"""
    its = P["its"]
    idx, clamped = resolve_draws(np.asarray(draws)[:its], n)
    P1 = f["X1"][idx].transpose(0, 2, 1)          # [its, 3 (component), 3 (point)]
    P2 = f["X2"][idx].transpose(0, 2, 1)
    R, t, s, nan_rot = compute_sim3(P1, P2, P["fix_scale"])
    sR, sRi, ti = transforms(R, s, t)
    mask = np.zeros((its, n), bool)
    for a in range(0, its, 64):
        sl = slice(a, min(a + 64, its))
        e1, e2 = errors(P, f, sR[sl], t[sl], sRi[sl], ti[sl])
        mask[sl] = (e1 < f["max1"][None]) & (e2 < f["max2"][None])
    T12 = np.zeros((its, 4, 4), F32)
    T12[:, :3, :3], T12[:, :3, 3], T12[:, 3, 3] = sR, t, 1.0
    flags = (nan_rot * HYP_NAN + clamped * HYP_CLAMPED).astype(np.int32)
    hyps = np.zeros((its, 32), F32)
    hyps[:, :16], hyps[:, 16:25], hyps[:, 25:28], hyps[:, 28], hyps[:, 29] = T12.reshape(its, 16), R.reshape(its, 9), t, s, flags.view(F32)
    return {"idx": idx, "flags": flags, "hyps": hyps, "mask": mask, "counts": mask.sum(1).astype(np.int32)}


def sim3_ransac(P, xw1, xw2, s1, s2, draws, N=None, H=None, fill=None):
    """rfe_sim3_ransac for one problem: the dict of OUT.  fill: what inliers / best_inliers [N], counts [H] and hyps [H,32] hold where
    the call does not write (default 0)"""
    xw1, xw2 = np.asarray(xw1, F32).reshape(-1, 3), np.asarray(xw2, F32).reshape(-1, 3)
    N = len(xw1) if N is None else N
    draws = np.asarray(draws, np.int32).reshape(-1, 3)
    H = len(draws) if H is None else H
    n = min(max(P["n"], 0), N)
    its, mn = P["its"], P["min_inliers"]
    assert 1 <= its <= H and mn >= 0
    fill = fill or {}
    o = {"inliers": np.array(fill.get("inliers", np.zeros(N)), np.uint8).reshape(N), "best_inliers": np.array(fill.get("best_inliers", np.zeros(N)), np.uint8).reshape(N),
         "counts": np.array(fill.get("counts", np.zeros(H)), np.int32).reshape(H), "hyps": np.array(fill.get("hyps", np.zeros((H, 32))), F32).reshape(H, 32)}
    if n < 3 or n < mn:
        o["inliers"][:n] = 0
        o["best_inliers"][:n] = 0
        o.update(T12=np.eye(4, dtype=F32).reshape(16), R=np.eye(3, dtype=F32).reshape(9), t=np.zeros(3, F32), s=np.ones((), F32),
                 stats=np.array([0, 0, 0, -1, 0, 1, 0, (FLAG_FEW if n < mn else 0) | (FLAG_BELOW_THREE if n < 3 else 0)], np.int32))
        return o
    f = front(P, xw1[:n], xw2[:n], np.asarray(s1, F32).reshape(-1)[:n], np.asarray(s2, F32).reshape(-1)[:n])
    hy = hypotheses(P, f, draws, n)
    cnt = hy["counts"]
    above = np.flatnonzero(cnt > mn)
    conv = len(above) > 0
    chosen = int(above[0]) if conv else int(np.flatnonzero(cnt == cnt.max())[-1])
    iters = chosen + 1 if conv else its
    o["counts"][:its], o["hyps"][:its] = cnt, hy["hyps"]
    o["best_inliers"][:n] = hy["mask"][chosen]
    o["inliers"][:n] = hy["mask"][chosen] if conv else 0
    rec = hy["hyps"][chosen]
    o.update(T12=rec[:16].copy(), R=rec[16:25].copy(), t=rec[25:28].copy(), s=rec[28].copy(),
             stats=np.array([conv, cnt[chosen] if conv else 0, cnt[chosen], chosen, iters, not conv, ((hy["flags"][:iters] & HYP_NAN) != 0).sum(),
                             FLAG_CLAMPED if (hy["flags"] & HYP_CLAMPED).any() else 0], np.int32))
    return o


def solve(c, **kw):
    return sim3_ransac(c["P"], c["xw1"], c["xw2"], c["s1"], c["s2"], c["draws"], **kw)


# ---------------------------------------------------------------- the sequential transcription
def _rot_from_quat64(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], F64)


class Sequential:
    """Sim3Solver as the reference runs it, on one case.  mode "contract": float32 scalars and the contract's choices; mode "reference":
    float64 throughout with numpy.linalg.eigh and the angle-axis route (:370-376)"""

    def __init__(self, c, mode="contract"):
        self.c, self.mode, self.P = c, mode, c["P"]
        P = self.P
        self.T = F32 if mode == "contract" else F64
        T = self.T
        n = self.N = P["n"]
        self.cam1, self.cam2 = [T(v) for v in P["cam1"]], [T(v) for v in P["cam2"]]
        self.X1, self.X2, self.p1, self.p2, self.max1, self.max2 = [], [], [], [], [], []
        with np.errstate(**_ERR):
            for i in range(n):                                       # :71-118 (the pointer chasing is the drop-in's), :120-121
                for xw, R, t, cam, Xs, ps in ((c["xw1"], P["rcw1"], P["tcw1"], self.cam1, self.X1, self.p1),
                                              (c["xw2"], P["rcw2"], P["tcw2"], self.cam2, self.X2, self.p2)):
                    x, y, z = (T(v) for v in np.asarray(xw, F32).reshape(-1, 3)[i])
                    X = [((T(R[r, 0]) * x + T(R[r, 1]) * y) + T(R[r, 2]) * z) + T(t[r]) for r in range(3)]
                    Xs.append(X)
                    ps.append(self.project(cam, X))
                self.max1.append(int(9.210 * float(F32(c["s1"][i]))))   # size_t
                self.max2.append(int(9.210 * float(F32(c["s2"][i]))))
        self.all_indices = list(range(n))
        self.min_inliers, self.max_its = P["min_inliers"], P["its"]    # SetRansacParameters has run: its is its result
        self.iterations, self.best_inliers_n = 0, 0
        self.best_mask, self.best = None, None
        self.counts, self.nan_rots, self.clamped, self.residuals, self.margin = [], 0, False, [], np.inf
        self.log, self.gaps = [], []                                 # per hypothesis (R, t, s); reference mode: the gap under the top eigenvalue

    def project(self, cam, X):
        return [(cam[0] * X[0]) / X[2] + cam[2], (cam[1] * X[1]) / X[2] + cam[3]]

    def rand(self, k, size):
        r = int(self.c["draws"][self.iterations - 1][k])
        cl = min(max(r, 0), size - 1)
        self.clamped |= cl != r
        return cl

    def compute_sim3(self, P1, P2):
        T = self.T
        O1 = [((P1[r][0] + P1[r][1]) + P1[r][2]) / T(3.0) for r in range(3)]
        O2 = [((P2[r][0] + P2[r][1]) + P2[r][2]) / T(3.0) for r in range(3)]
        Pr1 = [[P1[r][k] - O1[r] for k in range(3)] for r in range(3)]
        Pr2 = [[P2[r][k] - O2[r] for k in range(3)] for r in range(3)]
        M = [[(Pr2[r][0] * Pr1[c][0] + Pr2[r][1] * Pr1[c][1]) + Pr2[r][2] * Pr1[c][2] for c in range(3)] for r in range(3)]
        m = [[F64(M[r][c]) for c in range(3)] for r in range(3)]
        N11, N12, N13, N14 = (m[0][0] + m[1][1]) + m[2][2], m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]
        N22, N23, N24 = (m[0][0] - m[1][1]) - m[2][2], m[0][1] + m[1][0], m[2][0] + m[0][2]
        N33, N34, N44 = (-m[0][0] + m[1][1]) - m[2][2], m[1][2] + m[2][1], (-m[0][0] - m[1][1]) + m[2][2]
        Nm = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], T)   # Matrix4f
        if self.mode == "contract":
            q, lam, qd = self.jacobi(Nm)
            R, nan_rot = self.rotation(q)
            nn = np.linalg.norm(Nm.astype(F64))                          # the residual of the double eigenpair, relative to |N|
            self.residuals.append(float(np.linalg.norm(Nm.astype(F64) @ qd - lam * qd) / nn) if nn > 0 else 0.0)
        else:
            ev, evec = np.linalg.eigh(Nm)
            q = evec[:, int(np.argmax(ev))]
            self.gaps.append(float((ev[3] - ev[2]) / max(np.linalg.norm(Nm), 1e-300)))
            vec = q[1:4]
            nv = np.sqrt(vec @ vec)
            nan_rot = nv == 0
            ang = math.atan2(nv, q[0])
            vec = 2 * ang * vec / nv                                     # :375
            theta = np.sqrt(vec @ vec)                                   # Sophus::SO3::exp
            half = 0.5 * theta
            im = (math.sin(half) / theta) * vec if theta > 0 else 0.5 * vec
            qq = np.array([math.cos(half), im[0], im[1], im[2]], F64)
            R = _rot_from_quat64(qq / np.sqrt(qq @ qq))
        P3 = [[(R[r][0] * Pr2[0][k] + R[r][1] * Pr2[1][k]) + R[r][2] * Pr2[2][k] for k in range(3)] for r in range(3)]
        if self.P["fix_scale"]:
            s = T(1.0)
        else:
            nom, den = T(0.0), T(0.0)
            for k in range(3):
                for r in range(3):
                    nom = nom + Pr1[r][k] * P3[r][k]
                    den = den + P3[r][k] * P3[r][k]
            s = T(F64(nom) / F64(den))
        sR = [[s * R[r][c] for c in range(3)] for r in range(3)]
        t = [O1[r] - ((sR[r][0] * O2[0] + sR[r][1] * O2[1]) + sR[r][2] * O2[2]) for r in range(3)]
        inv = T(1.0 / F64(s))
        sRi = [[inv * R[c][r] for c in range(3)] for r in range(3)]
        ti = [-((sRi[r][0] * t[0] + sRi[r][1] * t[1]) + sRi[r][2] * t[2]) for r in range(3)]
        return np.array(R, T), np.array(t, T), s, sR, sRi, ti, bool(nan_rot)

    def jacobi(self, Nm):
        A = [[F64(Nm[r][c]) for c in range(4)] for r in range(4)]
        V = [[F64(r == c) for c in range(4)] for r in range(4)]
        for _ in range(SWEEPS):
            for p, r in PAIRS:
                apq = A[p][r]
                if apq != 0.0:
                    theta = (A[r][r] - A[p][p]) / (2.0 * apq)
                    tt = (F64(1.0) if theta >= 0.0 else F64(-1.0)) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(tt * tt + 1.0)
                    s = tt * c
                    app, arr = A[p][p] - tt * apq, A[r][r] + tt * apq
                    for k in range(4):
                        if k != p and k != r:
                            akp, akr = A[k][p], A[k][r]
                            A[k][p] = A[p][k] = c * akp - s * akr
                            A[k][r] = A[r][k] = s * akp + c * akr
                        vkp, vkr = V[k][p], V[k][r]
                        V[k][p], V[k][r] = c * vkp - s * vkr, s * vkp + c * vkr
                    A[p][p], A[r][r] = app, arr
                    A[p][r] = A[r][p] = F64(0.0)
        best, col = A[0][0], 0
        for c in range(1, 4):
            if A[c][c] > best:
                best, col = A[c][c], c
        v = [V[k][col] for k in range(4)]
        nrm = np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
        v = [e / nrm for e in v]
        first = next((e for e in v if e != 0), F64(0.0))
        if first < 0:
            v = [-e for e in v]
        return np.array(v, F64).astype(F32), best, np.array(v, F64)

    def rotation(self, q):
        w, x, y, z = (F32(e) for e in q)
        if np.sqrt((x * x + y * y) + z * z) == 0:
            return [[F32(np.nan)] * 3 for _ in range(3)], True
        tx, ty, tz = F32(2.0) * x, F32(2.0) * y, F32(2.0) * z
        twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
        one = F32(1.0)
        return [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]], False

    def check_inliers(self, sR, t, sRi, ti):
        mask = []
        for i in range(self.N):
            X1, X2 = self.X1[i], self.X2[i]
            q1 = self.project(self.cam1, [((sR[r][0] * X2[0] + sR[r][1] * X2[1]) + sR[r][2] * X2[2]) + t[r] for r in range(3)])
            q2 = self.project(self.cam2, [((sRi[r][0] * X1[0] + sRi[r][1] * X1[1]) + sRi[r][2] * X1[2]) + ti[r] for r in range(3)])
            d1, d2 = [self.p1[i][k] - q1[k] for k in range(2)], [q2[k] - self.p2[i][k] for k in range(2)]
            e1, e2 = d1[0] * d1[0] + d1[1] * d1[1], d2[0] * d2[0] + d2[1] * d2[1]
            b1, b2 = self.T(F32(self.max1[i])), self.T(F32(self.max2[i]))
            for e, b in ((e1, b1), (e2, b2)):
                if np.isfinite(e) and b > 0:
                    self.margin = min(self.margin, abs(float(e) - float(b)) / float(b))
            mask.append(bool(e1 < b1 and e2 < b2))
        return mask

    def iterate(self, n_iterations):
        """the five-argument overload (:221-302); returns (T or None for the uninitialised bestSim3, bNoMore, inliers, nInliers, bConverge)"""
        T = self.T
        if self.N < self.min_inliers:
            return np.eye(4, dtype=T), True, [False] * self.N, 0, False
        cur, best_sim3 = 0, None
        with np.errstate(**_ERR):
            while self.iterations < self.max_its and cur < n_iterations:
                cur += 1
                self.iterations += 1
                avail = list(self.all_indices)
                P1, P2 = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
                for k in range(3):
                    randi = self.rand(k, len(avail))
                    idx = avail[randi]
                    for r in range(3):
                        P1[r][k], P2[r][k] = self.X1[idx][r], self.X2[idx][r]
                    avail[randi] = avail[-1]
                    avail.pop()
                R, t, s, sR, sRi, ti, nan_rot = self.compute_sim3(P1, P2)
                self.nan_rots += nan_rot
                mask = self.check_inliers(sR, t, sRi, ti)
                cnt = sum(mask)
                self.counts.append(cnt)
                self.log.append((R, t, s))
                if cnt >= self.best_inliers_n:
                    T12 = np.zeros((4, 4), T)
                    T12[:3, :3], T12[:3, 3], T12[3, 3] = np.array(sR, T), t, 1
                    self.best_mask, self.best_inliers_n, self.best = mask, cnt, (T12, R, t, s, self.iterations - 1)
                    if cnt > self.min_inliers:
                        return T12, False, list(mask), cnt, True
                    best_sim3 = T12
        return best_sim3, self.iterations >= self.max_its, [False] * self.N, 0, False

    def run(self, chunk=20):
        """while(!bConverge && !bNoMore) iterate(chunk): the dict of sim3_ransac() (counts as far as the loop got)"""
        N = self.N
        if N < 3 or N < self.min_inliers:
            return None
        while True:
            T12, no_more, inl, n_inl, conv = self.iterate(chunk)
            if conv or no_more:
                break
        bT, bR, bt, bs, bh = self.best
        return {"T12": bT.reshape(16), "R": np.array(bR).reshape(9), "t": np.array(bt), "s": np.array(bs), "inliers": np.array(inl, np.uint8),
                "best_inliers": np.array(self.best_mask, np.uint8), "counts": np.array(self.counts, np.int32),
                "stats": np.array([conv, n_inl, self.best_inliers_n, bh, self.iterations, no_more, self.nan_rots, FLAG_CLAMPED if self.clamped else 0], np.int32)}


DEGENERATE = 1e-5


def measure(cases):
    """departures (a)-(c): the contract against the reference-mode transcription over every hypothesis the cases run.  Returns the
    largest rotation angle between the two R (rad), the largest relative differences of s and t, the largest Jacobi residual
    |N q - lambda q| / |N|, the smallest relative distance of any e1 / e2 of the float64 run to its bound, and whether every
    hypothesis' count and every final flag agreed.  A hypothesis whose two largest eigenvalues lie within DEGENERATE |N| of each other
    (a collinear triple: the rotation about the line is free, and every solver picks its own) is counted apart and not compared"""
    m = {"angle": 0.0, "s": 0.0, "t": 0.0, "residual": 0.0, "margin": np.inf, "hypotheses": 0, "degenerate": 0, "same_inliers": True}
    for c in cases:
        a, b = Sequential(c, "contract"), Sequential(c, "reference")
        ra, rb = a.run(), b.run()
        if ra is None:
            continue
        m["margin"] = min(m["margin"], b.margin)
        m["same_inliers"] &= bool(a.counts == b.counts and np.array_equal(ra["inliers"], rb["inliers"])
                                  and np.array_equal(ra["best_inliers"], rb["best_inliers"]) and np.array_equal(ra["stats"], rb["stats"]))
        m["residual"] = max([m["residual"]] + a.residuals)
        for (Ra, ta, sa), (Rb, tb, sb), gap in zip(a.log, b.log, b.gaps):
            if not np.isfinite(Ra).all():
                continue
            if gap < DEGENERATE:
                m["degenerate"] += 1
                continue
            m["hypotheses"] += 1
            cs = (np.trace(Ra.astype(F64).T @ Rb) - 1) / 2
            sn = np.linalg.norm(Ra.astype(F64) - Rb) / math.sqrt(2)      # the chord: resolves angles the cosine cannot
            m["angle"] = max(m["angle"], float(sn if cs > 0.5 else math.acos(max(-1.0, cs))))
            m["s"] = max(m["s"], abs(float(sa) - float(sb)) / abs(float(sb)))
            m["t"] = max(m["t"], float(np.linalg.norm(ta.astype(F64) - tb) / max(np.linalg.norm(tb), 1e-30)))
    return m


# ---------------------------------------------------------------- planted problems
def rotvec_to_mat(w):
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


CAM1, CAM2 = (520.0, 515.0, 320.5, 240.25), (480.0, 485.0, 310.0, 250.0)


def scene(seed, n, outliers=0.4, s=1.3, angle=0.4, its=300, min_inliers=None, fix_scale=False, sigma2=(1.0, 1.44, 2.0736), H=None, identity_poses=False):
    """n correspondences under a planted Sim3 (X1c = s R X2c + t): exact inliers, gross outliers at least 50 px off in image 1"""
    rng = np.random.default_rng(seed)
    if fix_scale:
        s = 1.0
    R12 = rotvec_to_mat(angle * np.array([0.3, 0.9, -0.3]) / np.linalg.norm([0.3, 0.9, -0.3]))
    t12 = np.array([0.4, -0.2, 0.3])
    X1c = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 8, n)], 1)
    n_out = int(round(outliers * n)) if n > 3 else 0
    is_out = np.zeros(n, bool)
    is_out[rng.permutation(n)[:n_out]] = True
    X1p = X1c.copy()                                                 # what pMP2 really sees: displaced for the outliers
    shift = rng.uniform(60, 200, n) * rng.choice([-1, 1], n) * X1c[:, 2] / CAM1[0]
    X1p[is_out, 0] += shift[is_out]
    X2c = (X1p - t12) @ R12 / s                                      # R^T (X - t) / s
    if identity_poses:
        R1 = R2 = np.eye(3); t1 = t2 = np.zeros(3)
    else:
        R1, t1 = rotvec_to_mat(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)
        R2, t2 = rotvec_to_mat(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)
    xw1, xw2 = (X1c - t1) @ R1, (X2c - t2) @ R2
    H = its if H is None else H
    n_in = n - n_out
    mn = max(3, int(0.75 * n_in)) if min_inliers is None else min_inliers
    draws = np.stack([rng.integers(0, max(n - k, 1), H) for k in range(3)], 1).astype(np.int32)
    lv1, lv2 = rng.integers(0, len(sigma2), n), rng.integers(0, len(sigma2), n)
    return {"P": params(R1, t1, R2, t2, CAM1, CAM2, fix_scale, mn, its, n), "xw1": xw1.astype(F32), "xw2": xw2.astype(F32),
            "s1": np.asarray(sigma2, F32)[lv1], "s2": np.asarray(sigma2, F32)[lv2], "draws": draws, "is_out": is_out,
            "truth": {"R": R12, "t": t12, "s": s}}


def triple(i0, i1, i2, n):
    """the draws that make the list hand out i0, i1, i2 directly (no displaced entry involved)"""
    assert len({i0, i1, i2}) == 3 and i0 <= n - 1 and i1 <= n - 2 and i2 <= n - 3
    return [i0, i1, i2]


def forced(name):
    """the forced paths of the issue; each a case dict (some carry `expect`)"""
    if name in ("conv_first", "conv_last", "max_three_times"):
        n = 30
        c = scene(7, n, outliers=1 / 3, its=5 if name != "max_three_times" else 6, min_inliers=15 if name != "max_three_times" else 25)
        good, bad = np.flatnonzero(~c["is_out"] & (np.arange(n) < n - 3)), np.flatnonzero(c["is_out"] & (np.arange(n) < n - 3))
        g = [triple(*good[3 * k:3 * k + 3], n) for k in range(3)]
        b = [triple(bad[k], bad[k + 1], good[-1 - k], n) for k in range(4)]
        c["draws"] = np.array({"conv_first": [g[0], b[0], b[1], g[1], b[2]], "conv_last": [b[0], b[1], b[2], b[3], g[0]],
                               "max_three_times": [b[0], g[0], b[1], g[1], g[2], b[2]]}[name], np.int32)
        return c
    if name == "n_eq_min":
        c = scene(8, 12, outliers=0.0, min_inliers=12)
        c["P"]["its"] = ransac_iterations(0.99, 12, 12, 300)
        return c
    if name == "n_lt_min":
        return scene(9, 5, outliers=0.0, min_inliers=6, its=4)
    if name in ("pure_translation", "pure_translation_only"):
        # integer camera-frame points whose sums are multiples of 3, identity poses: Pr1 == Pr2 bit for bit, M is symmetric, N's first row
        # and column vanish off the diagonal and the eigenvector is (1, 0, 0, 0)
        c = scene(10, 12, outliers=0.0, min_inliers=3, its=3, identity_poses=True)
        X2 = np.array([[0, 0, 4], [3, 0, 4], [0, 3, 7]], F32)
        c["xw2"][:3], c["xw1"][:3] = X2, X2 + np.array([1, 2, 0], F32)
        c["draws"] = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
        if name == "pure_translation_only":
            c["P"]["its"] = 1
            c["draws"] = c["draws"][:1]
        return c
    if name == "collinear":
        c = scene(11, 12, outliers=0.0, min_inliers=3, its=2, identity_poses=True)
        line = np.array([[0, 0, 4], [1, 0.5, 5], [2, 1, 6]], F64)
        tr = c["truth"]
        c["xw1"][:3], c["xw2"][:3] = line.astype(F32), ((line - tr["t"]) @ tr["R"] / tr["s"]).astype(F32)
        c["draws"] = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
        return c
    if name == "threshold":
        # sigma2 = 1.44: 9.210 * 1.44 = 13.26 truncates to 13.  Correspondences 0 and 1 are moved 3.6194 px (e = 13.1) and 3.5917 px
        # (e = 12.9) in image 1; side 2 is given a bound far away
        c = scene(12, 12, outliers=0.0, min_inliers=3, its=1, identity_poses=True, sigma2=(1.44,))
        c["s2"][:] = 100.0
        for i, px in ((0, math.sqrt(13.1)), (1, math.sqrt(12.9))):
            c["xw1"][i, 0] += F32(px * float(c["xw1"][i, 2]) / CAM1[0])
        c["draws"] = np.array([[3, 4, 5]], np.int32)
        return c
    if name == "behind":
        c = scene(13, 12, outliers=0.0, min_inliers=3, its=2, identity_poses=True)
        tr = c["truth"]
        c["xw2"][0] = ((np.array([0.5, 0.2, -3.0]) - tr["t"]) @ tr["R"] / tr["s"]).astype(F32)     # lands at z = -3 in camera 1
        c["draws"] = np.array([[3, 4, 5], [6, 7, 8]], np.int32)
        return c
    if name == "nan":
        c = scene(14, 12, outliers=0.0, min_inliers=3, its=2)
        c["xw1"][0], c["xw2"][1, 2] = np.nan, np.nan
        c["draws"] = np.array([[3, 4, 5], [6, 7, 8]], np.int32)
        return c
    if name == "displaced":
        n = 12
        c = scene(15, n, outliers=0.0, min_inliers=n, its=7)           # never converges: every hypothesis runs
        c["draws"] = np.array([[5, 5, 1], [n - 1, 3, 3], [n - 2, 2, 2], [n - 2, n - 2, n - 3], [4, 7, 4], [n - 1, n - 2, n - 3], [0, 0, 0]], np.int32)
        return c
    if name == "out_of_range":
        n = 12
        c = scene(16, n, outliers=0.0, min_inliers=n, its=4)
        c["draws"] = np.array([[-1, 3, 5], [2, n - 1, 4], [1, 2, 1 << 30], [n + 5, -(1 << 31), n - 2]], np.int32)
        return c
    raise KeyError(name)


FORCED = ("conv_first", "conv_last", "max_three_times", "n_eq_min", "n_lt_min", "pure_translation", "pure_translation_only", "collinear",
          "threshold", "behind", "nan", "displaced", "out_of_range")
