"""numpy restatement of LocalMapping::CreateNewMapPoints behind the matcher (reference src/LocalMapping.cc:579-943, the filter of
SPmatcher::SearchForTriangulation at src/Matchers/SPmatcher.cc:1376-1393, GeometricTools::Triangulate, KeyFrame::UnprojectStereo), the
contract of DESIGN.md 6g: every match slot of every neighbour as single np.float32 operations in the order the contract writes them (the
three double expressions of the reference in float64), the one-sided Jacobi null vector with its fixed schedule, then the rule "the lowest
passing neighbour takes the feature" and the list in creation order.  Shared by test_triangulation_ref.py (CPU), test_gpu_triangulation.py
and tools/bench_triangulate.py; holds the case generators."""
import numpy as np

F32 = np.float32
F64 = np.float64
MAX_LEVELS = 16
SWEEPS = 6                                  # outputs stop changing from 4 sweeps on over the generators below, plus two
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
CODES = ("created", "neighbour skipped", "index out of range", "existing map point", "Triangulate: w == 0", "no stereo and low parallax",
         "UnprojectStereo: depth <= 0", "z1 <= 0", "z2 <= 0", "reprojection, view 1 mono", "reprojection, view 1 stereo",
         "reprojection, view 2 mono", "reprojection, view 2 stereo", "dist == 0", "far point", "scale consistency",
         "claimed by an earlier neighbour")
NO_SLOT = -1                                # k >= S[n]
CLAIMED = 16
# `cosParallaxRays < 0.9998` / `< 0.9996` compare the float with DOUBLE literals (LocalMapping.cc:792).  fl32(0.9998) = 0x1.ffe5cap-1 lies
# above its literal, fl32(0.9996) = 0x1.ffcb92p-1 below: the float comparisons with the same truth table are `< COS_9998` and `< COS_9996`
COS_9998 = F32(0.9998)
COS_9996 = np.nextafter(F32(0.9996), F32(2))
assert float(COS_9998) > 0.9998 > float(np.nextafter(COS_9998, F32(0))) and COS_9998.view(np.uint32) == 0x3F7FF2E5
assert float(COS_9996) > 0.9996 > float(np.nextafter(COS_9996, F32(0))) and COS_9996.view(np.uint32) == 0x3F7FE5CA
CHI2_MONO, CHI2_STEREO = 5.991, 7.8         # double literals; the products with sigma2 are double products
VIEW_KEYS = ("rcw", "tcw", "ow", "fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")


def _f(a):
    return np.asarray(a, F32)


def view(rcw, tcw, ow, fx, fy, cx, cy, mb, mbf, invfx=None, invfy=None):
    """rfe_tri_view: invfx / invfy default to the float quotients 1.0f / fx, 1.0f / fy (KeyFrame's values)"""
    return {"rcw": _f(rcw).reshape(3, 3).copy(), "tcw": _f(tcw).copy(), "ow": _f(ow).copy(), "fx": F32(fx), "fy": F32(fy), "cx": F32(cx), "cy": F32(cy),
            "invfx": F32(1) / F32(fx) if invfx is None else F32(invfx), "invfy": F32(1) / F32(fy) if invfy is None else F32(invfy),
            "mb": F32(mb), "mbf": F32(mbf)}


def params(inertial, far_points, th_far, ratio_factor, scale_factors, level_sigma2):
    return {"inertial": bool(inertial), "far_points": bool(far_points), "th_far": F32(th_far), "ratio_factor": F32(ratio_factor),
            "nlevels": len(scale_factors), "scale_factors": _f(scale_factors), "level_sigma2": _f(level_sigma2)}


def stereo_parallax(mb, depth):
    """cos(2 atan2(mb / 2, depth)) as (d d - h h) / (d d + h h), h = mb / 2, in fp32 (departure (a) of 6g)"""
    h = _f(mb) / F32(2)
    d = _f(depth)
    dd, hh = d * d, h * h
    return (dd - hh) / (dd + hh)


def jacobi_null(A, sweeps=SWEEPS):
    """A: 4 rows of 4 float32 arrays.  One-sided Jacobi on the columns in the fixed pair order, `sweeps` sweeps, V accumulated; returns the
    column of V whose column of the rotated A has the smallest squared norm (the first minimum), as 4 arrays."""
    A = [[np.array(a, F32) for a in row] for row in A]
    one, zero = np.ones_like(A[0][0]), np.zeros_like(A[0][0])
    V = [[one.copy() if r == c else zero.copy() for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            alpha = ((A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p]) + A[3][p] * A[3][p]
            beta = ((A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q]) + A[3][q] * A[3][q]
            gamma = ((A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q]) + A[3][p] * A[3][q]
            rot = gamma != 0                                           # NaN rotates (and spreads)
            zeta = (beta - alpha) / (F32(2) * gamma)
            t = np.where(zeta >= 0, F32(1), F32(-1)).astype(F32) / (np.abs(zeta) + np.sqrt(F32(1) + zeta * zeta))
            c = F32(1) / np.sqrt(F32(1) + t * t)
            s = c * t
            for M in (A, V):
                for r in range(4):
                    ap, aq = M[r][p], M[r][q]
                    M[r][p] = np.where(rot, c * ap - s * aq, ap)
                    M[r][q] = np.where(rot, s * ap + c * aq, aq)
    nrm = [((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]) + A[3][c] * A[3][c] for c in range(4)]
    best = [V[r][0] for r in range(4)]
    nb = nrm[0]
    for c in range(1, 4):
        less = nrm[c] < nb                                             # the first minimum stays; a NaN norm is never smaller
        nb = np.where(less, nrm[c], nb)
        best = [np.where(less, V[r][c], best[r]) for r in range(4)]
    for a in best:
        assert a.dtype == np.float32
    return best


def _level(table, octave):
    """table[octave]; an octave outside 0..15 reads level 0 (nothing out of range is dereferenced)"""
    t = np.zeros((MAX_LEVELS,), F32)
    t[:len(table)] = table
    o = np.asarray(octave)
    return t[np.where((o >= 0) & (o < MAX_LEVELS), o, 0)]


def evaluate(P, c, sweeps=SWEEPS):
    """Every slot on its own: code (a passing slot has 0, CLAIMED comes later), x3d, point_stereo, stereo attempt, by slot [Nn,Kmax]."""
    v1 = c["view1"]
    Nn, Kmax = c["pairs"].shape[:2]
    N1 = len(c["kpts1"])
    N2max = c["kpts2"].shape[1] if Nn else 0
    S = np.clip(np.asarray(c["S"], np.int64), 0, Kmax)
    nn, kk = np.meshgrid(np.arange(Nn), np.arange(Kmax), indexing="ij")
    nvalid = np.ones((Nn,), bool) if c.get("neighbour_valid") is None else np.asarray(c["neighbour_valid"]) != 0
    code = np.zeros((Nn, Kmax), np.int32)
    slot = kk < S[:, None] if Nn else np.zeros((0, Kmax), bool)
    pi, pj = c["pairs"][..., 0].astype(np.int64), c["pairs"][..., 1].astype(np.int64)
    n2 = np.minimum(np.asarray(c["n2"], np.int64), N2max)
    inr = (pi >= 0) & (pi < N1) & (pj >= 0) & (pj < n2[:, None]) if Nn else slot
    i, j = np.where(inr, pi, 0), np.where(inr, pj, 0)
    if N1 == 0 or N2max == 0 or Nn == 0:
        z3 = np.zeros((Nn, Kmax, 3), F32)
        code[...] = np.where(slot, np.where(nvalid[:, None], 2, 1), NO_SLOT)
        return {"code": code, "x3d": z3, "point_stereo": np.zeros((Nn, Kmax), np.uint8), "attempt": np.zeros((Nn, Kmax), bool), "S": S, "nvalid": nvalid}
    has_mp = (c["has_mp1"][i] != 0) | (c["has_mp2"][nn, j] != 0)
    k1 = c["kpts1"][i]
    k1r = (c["kpts1"] if c.get("kpts1_raw") is None else c["kpts1_raw"])[i]
    k2 = c["kpts2"][nn, j]
    k2r = (c["kpts2"] if c.get("kpts2_raw") is None else c["kpts2_raw"])[nn, j]
    ur1, ur2, d1, d2 = c["uright1"][i], c["uright2"][nn, j], c["depth1"][i], c["depth2"][nn, j]
    o1, o2 = c["octave1"][i], c["octave2"][nn, j]
    v2 = {k: np.stack([_f(v[k]) for v in c["views2"]])[nn] for k in VIEW_KEYS}       # per slot
    R1, t1, ow1 = v1["rcw"], v1["tcw"], v1["ow"]
    R2, t2, ow2 = v2["rcw"], v2["tcw"], v2["ow"]
    with np.errstate(all="ignore"):
        st1, st2 = ur1 >= 0, ur2 >= 0
        xn1x, xn1y = (k1[..., 0] - v1["cx"]) / v1["fx"], (k1[..., 1] - v1["cy"]) / v1["fy"]
        xn2x, xn2y = (k2[..., 0] - v2["cx"]) / v2["fx"], (k2[..., 1] - v2["cy"]) / v2["fy"]
        one = np.ones_like(xn1x)
        ray1 = [(R1[0, a] * xn1x + R1[1, a] * xn1y) + R1[2, a] * one for a in range(3)]          # Rwc = Rcw^T
        ray2 = [(R2[..., 0, a] * xn2x + R2[..., 1, a] * xn2y) + R2[..., 2, a] * one for a in range(3)]
        dot = (ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2]
        na = np.sqrt((ray1[0] * ray1[0] + ray1[1] * ray1[1]) + ray1[2] * ray1[2])
        nb = np.sqrt((ray2[0] * ray2[0] + ray2[1] * ray2[1]) + ray2[2] * ray2[2])
        cosr = dot / (na * nb)
        cs = cosr + F32(1)
        cs1 = np.where(st1, stereo_parallax(v1["mb"], d1), cs)
        cs2 = np.where(~st1 & st2, stereo_parallax(v2["mb"], d2), cs)                          # `else if (bStereo2)`
        cst = np.where(cs2 < cs1, cs2, cs1)                                                    # std::min
        low = cosr < (COS_9996 if P["inertial"] else COS_9998)
        tri = (cosr < cst) & (cosr > 0) & (st1 | st2 | low)
        un1 = ~tri & st1 & (cs1 < cs2)
        un2 = ~tri & ~un1 & st2 & (cs2 < cs1)
        # GeometricTools::Triangulate
        T1 = [[R1[r, 0] * one, R1[r, 1] * one, R1[r, 2] * one, t1[r] * one] for r in range(3)]
        T2 = [[R2[..., r, 0], R2[..., r, 1], R2[..., r, 2], t2[..., r]] for r in range(3)]
        A = [[xn1x * T1[2][cc] - T1[0][cc] for cc in range(4)], [xn1y * T1[2][cc] - T1[1][cc] for cc in range(4)],
             [xn2x * T2[2][cc] - T2[0][cc] for cc in range(4)], [xn2y * T2[2][cc] - T2[1][cc] for cc in range(4)]]
        h = jacobi_null(A, sweeps)
        w0 = h[3] == 0
        xt = [h[a] / h[3] for a in range(3)]
        # KeyFrame::UnprojectStereo, either view
        ux = ((k1r[..., 0] - v1["cx"]) * d1) * v1["invfx"]
        uy = ((k1r[..., 1] - v1["cy"]) * d1) * v1["invfy"]
        xu1 = [((R1[0, a] * ux + R1[1, a] * uy) + R1[2, a] * d1) + ow1[a] for a in range(3)]
        ux = ((k2r[..., 0] - v2["cx"]) * d2) * v2["invfx"]
        uy = ((k2r[..., 1] - v2["cy"]) * d2) * v2["invfy"]
        xu2 = [((R2[..., 0, a] * ux + R2[..., 1, a] * uy) + R2[..., 2, a] * d2) + ow2[..., a] for a in range(3)]
        bad1, bad2 = un1 & ~(d1 > 0), un2 & ~(d2 > 0)
        have = (tri & ~w0) | (un1 & ~bad1) | (un2 & ~bad2)
        X = [np.where(tri, xt[a], np.where(un1, xu1[a], xu2[a])) for a in range(3)]
        X = [np.where(have, x, F32(0)).astype(F32) for x in X]
        z1 = ((R1[2, 0] * X[0] + R1[2, 1] * X[1]) + R1[2, 2] * X[2]) + t1[2]
        z2 = ((R2[..., 2, 0] * X[0] + R2[..., 2, 1] * X[1]) + R2[..., 2, 2] * X[2]) + t2[..., 2]
        s1, s2 = _level(P["level_sigma2"], o1), _level(P["level_sigma2"], o2)

        def reproj(R, t, z, fx, fy, cx, cy, kp, ur, st, sig):
            if R.ndim == 2:
                x = ((R[0, 0] * X[0] + R[0, 1] * X[1]) + R[0, 2] * X[2]) + t[0]
                y = ((R[1, 0] * X[0] + R[1, 1] * X[1]) + R[1, 2] * X[2]) + t[1]
            else:
                x = ((R[..., 0, 0] * X[0] + R[..., 0, 1] * X[1]) + R[..., 0, 2] * X[2]) + t[..., 0]
                y = ((R[..., 1, 0] * X[0] + R[..., 1, 1] * X[1]) + R[..., 1, 2] * X[2]) + t[..., 1]
            invz = (F64(1.0) / z.astype(F64)).astype(F32)
            ex, ey = ((fx * x) / z + cx) - kp[..., 0], ((fy * y) / z + cy) - kp[..., 1]                  # Pinhole::project
            em = ex * ex + ey * ey
            u = (fx * x) * invz + cx
            ur_ = u - v1["mbf"] * invz                                                          # the CURRENT keyframe's mbf in both views (:886)
            ex, ey, er = u - kp[..., 0], ((fy * y) * invz + cy) - kp[..., 1], ur_ - ur
            es = (ex * ex + ey * ey) + er * er
            for a in (x, invz, em, es):
                assert a.dtype == np.float32
            return (~st & (em.astype(F64) > CHI2_MONO * sig.astype(F64)), st & (es.astype(F64) > CHI2_STEREO * sig.astype(F64)))
        m1, g1 = reproj(R1, t1, z1, v1["fx"], v1["fy"], v1["cx"], v1["cy"], k1, ur1, st1, s1)
        m2, g2 = reproj(R2, t2, z2, v2["fx"], v2["fy"], v2["cx"], v2["cy"], k2, ur2, st2, s2)
        e1 = [X[a] - ow1[a] for a in range(3)]
        e2 = [X[a] - ow2[..., a] for a in range(3)]
        dist1 = np.sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2])
        dist2 = np.sqrt((e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2])
        rd = dist2 / dist1
        ro = _level(P["scale_factors"], o1) / _level(P["scale_factors"], o2)
        for a in (cosr, cs1, cst, X[0], z1, z2, dist1, rd, ro):
            assert a.dtype == np.float32
        gates = [(15, (rd * P["ratio_factor"] < ro) | (rd > ro * P["ratio_factor"])),
                 (14, (dist1 >= P["th_far"]) | (dist2 >= P["th_far"]) if P["far_points"] else np.zeros_like(slot)),
                 (13, (dist1 == 0) | (dist2 == 0)), (12, g2), (11, m2), (10, g1), (9, m1), (8, z2 <= 0), (7, z1 <= 0),
                 (6, bad1 | bad2), (5, ~tri & ~un1 & ~un2), (4, tri & w0), (3, has_mp), (2, ~inr), (1, ~nvalid[:, None] & slot)]
    for cd, g in gates:                                                # the first failure stays
        code[g] = cd
    code[~slot] = NO_SLOT
    reached = slot & ((code == 0) | (code >= 4))                       # the slot got as far as the branches of :791-816
    x3d = np.stack(X, -1).astype(F32)
    x3d[~(slot & ((code == 0) | (code >= 7)))] = 0
    ps = ((un1 | un2) & reached).astype(np.uint8)
    return {"code": code, "x3d": np.ascontiguousarray(x3d), "point_stereo": ps, "attempt": (un1 | un2) & reached, "S": S, "nvalid": nvalid,
            "cosr": cosr}


KEYS = ("code", "x3d", "point_stereo", "out_n", "out_idx1", "out_idx2", "out_x3d", "out_stereo", "matches")


def triangulate(P, c, sweeps=SWEEPS):
    """Everything one call returns: KEYS, stats [8] and created."""
    e = evaluate(P, c, sweeps)
    code, N1 = e["code"].copy(), len(c["kpts1"])
    Nn, Kmax = code.shape
    pi = c["pairs"][..., 0].astype(np.int64)
    claim = np.full((max(N1, 1),), np.iinfo(np.int32).max, np.int64)
    ns, ks = np.nonzero(code == 0)
    np.minimum.at(claim, pi[ns, ks], ns)
    inr = (pi >= 0) & (pi < N1)
    owner = claim[np.where(inr, pi, 0)]
    nn = np.arange(Nn)[:, None]
    code[(code == 0) & (owner != nn)] = CLAIMED
    # the reference never looks at a slot whose feature an earlier neighbour took (it holds a map point by then): no stereo attempt there
    attempt = e["attempt"] & ~(inr & (owner < nn))
    ns, ks = np.nonzero(code == 0)                                     # row-major: n ascending, then k
    x3d, ps = e["x3d"], e["point_stereo"]
    out = {"code": code, "x3d": x3d, "point_stereo": ps, "out_n": ns.astype(np.int32), "out_idx1": c["pairs"][ns, ks, 0].astype(np.int32),
           "out_idx2": c["pairs"][ns, ks, 1].astype(np.int32), "out_x3d": np.ascontiguousarray(x3d[ns, ks]), "out_stereo": ps[ns, ks],
           "matches": np.where(e["nvalid"], e["S"], 0).astype(np.int32)}
    stats = np.zeros((8,), np.int32)
    stats[:6] = [len(ns), int(e["S"][e["nvalid"]].sum()), int((code == 3).sum()), int(ps[ns, ks].sum()), int(attempt.sum()),
                 int((~np.isfinite(x3d[ns, ks]).all(-1)).sum())]
    out.update(stats=stats, created=len(ns), cosr=e.get("cosr"))
    return out


# ---------------------------------------------------------------- cases
def _rot(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose_view(R64, centre, fx, fy, cx, cy, mb):
    R = R64.astype(F32)
    t = (-(R64 @ np.asarray(centre, F64))).astype(F32)
    ow = (-(R.astype(F64).T @ t.astype(F64))).astype(F32)              # the caller's mOw = -Rcw^T tcw
    return view(R, t, ow, fx, fy, cx, cy, mb, F32(mb) * F32(fx))


def _project(v, pts):
    pc = pts @ v["rcw"].astype(F64).T + v["tcw"].astype(F64)
    return np.stack([v["fx"] * pc[:, 0] / pc[:, 2] + v["cx"], v["fy"] * pc[:, 1] / pc[:, 2] + v["cy"]], 1), pc[:, 2]


SCALE, NLEVELS, TH_FAR = 1.2, 8, 30.0


def make_case(seed=0, W=640, H=480, N1=1100, N2=(1100, 900, 1100, 1, 700), S=(1100, 640, 0, 1, 257), Kmax=1100, invalid=4, identity1=True,
              plants=True, noise=0.7):
    """One current keyframe and len(N2) neighbours that look at N1 world points at depths 1.5..40 m.  A third of the points are seen without
    noise (their keypoints are the float32 projections: the CLEAR slots when their parallax is above 2 degrees), the others with `noise` px
    of Gaussian noise, on the quarter-pixel grid.  40 % of the features are stereo, 16 % on either side hold a map point (30 % of the slots
    are dropped for one), 15 % of the matches are outliers (clear when more than 20 px off), octaves follow the distance with some jitter.
    6 % of the inlier matches are 3..12 px off.  Neighbour 1 stands 6 cm from the current keyframe (less than the stereo baseline: its stereo
    features are unprojected, not triangulated).  Neighbour `invalid` fails the baseline gate.  With `plants` (the shapes of the main case): neighbour 3's single slot has w == 0 (a
    sheared matrix for a rotation: with a rotation w == 0 needs parallel rays, which never reach Triangulate), feature N1 - 2 is a stereo
    feature of subnormal depth that neighbour 0 sees (dist1 == 0), three stereo features have depth 0, three points lie between the image planes of
    the current keyframe and neighbour 1 (z2 <= 0), and three slots carry indices out of range.  identity1: the current keyframe is the world frame.  Returns (params without the two switches, case)."""
    rng = np.random.default_rng(seed)
    Nn, N2max = len(N2), max(N2)
    fx, fy, cx, cy = 420.5, 419.25, 318.75, 241.5
    R1 = np.eye(3) if identity1 else _rot((0.3, -1.0, 0.2), 0.3)
    c1 = np.zeros(3) if identity1 else np.array([0.4, -0.2, 0.3])
    v1 = _pose_view(R1, c1, fx, fy, cx, cy, 0.11)
    depth = np.exp(rng.uniform(np.log(1.5), np.log(40.0), N1))
    uv = np.stack([rng.uniform(30, W - 30, N1), rng.uniform(30, H - 30, N1)], 1)
    pc = np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth, depth], 1)
    pw = (pc - v1["tcw"].astype(F64)) @ v1["rcw"].astype(F64)          # R^T (pc - t)
    exact = rng.random(N1) < 0.35

    def observe(v, ids):
        """keypoints (undistorted = raw), uright, depth, octave of the world points ids in view v"""
        p, z = _project(v, pw[ids])
        n = len(ids)
        k = np.where(exact[ids, None], p, np.round((p + noise * rng.standard_normal((n, 2))) * 4) / 4).astype(F32)
        stereo = rng.random(n) < 0.4
        ur = np.where(exact[ids], p[:, 0] - float(v["mbf"]) / z, np.round((k[:, 0] - float(v["mbf"]) / z + 0.3 * rng.standard_normal(n)) * 4) / 4)
        ur = np.where(stereo & (z > 0.2), ur, -1).astype(F32)
        dep = np.where(ur >= 0, np.where(exact[ids], z, float(v["mbf"]) / np.maximum(k[:, 0] - ur, 1e-3)), -1).astype(F32)
        lvl = np.log(np.maximum(np.linalg.norm(pw[ids] - v["ow"].astype(F64), axis=1), 1e-3) / 1.5) / np.log(SCALE)
        jit = rng.choice((-1, 0, 0, 0, 1, 3), n)
        return k, ur, dep, np.clip(np.round(lvl).astype(np.int64) // 2 + jit, 0, NLEVELS - 1).astype(np.int32)
    k1, ur1, d1, o1 = observe(v1, np.arange(N1))
    has1 = (rng.random(N1) < 0.16).astype(np.uint8)
    views2 = []
    kp2 = np.zeros((Nn, N2max, 2), F32); ur2 = np.full((Nn, N2max), -1, F32); d2 = np.full((Nn, N2max), -1, F32)
    o2 = np.zeros((Nn, N2max), np.int32); has2 = np.zeros((Nn, N2max), np.uint8)
    pairs = np.full((Nn, Kmax, 2), -7, np.int32)
    clear = np.zeros((Nn, Kmax), bool)
    centres = [(0.45, 0.05, -0.35), (0.06, 0.01, 0.02), (0.2, -0.5, 0.0), (0.0, 0.0, 0.0), (0.9, 0.3, -0.2), (0.3, 0.6, 0.2), (-0.4, -0.6, -0.1)]
    for n in range(Nn):
        Rn = _rot(rng.standard_normal(3), 0.04 + 0.03 * n) @ R1
        v2 = _pose_view(Rn, c1 + R1.T @ np.array(centres[n % len(centres)]), fx + 3 * n, fy - 2 * n, cx + n, cy - n, 0.11 + 0.01 * n)
        views2.append(v2)
        ids = rng.permutation(N1)[:N2[n]]                              # feature j of neighbour n sees world point ids[j]
        kp2[n, :N2[n]], ur2[n, :N2[n]], d2[n, :N2[n]], o2[n, :N2[n]] = observe(v2, ids)
        has2[n, :N2[n]] = rng.random(N2[n]) < 0.16
        order = np.argsort(ids)
        take = np.sort(rng.permutation(len(ids))[:S[n]])
        i, j = ids[order][take], order[take]                           # i ascending
        out = rng.random(len(i)) < 0.15
        j = j.copy(); j[out] = np.roll(j[out], 1)                      # the outliers trade features among themselves: every j still once
        pairs[n, :len(i), 0], pairs[n, :len(i), 1] = i, j
        off = ~out & (rng.random(len(i)) < 0.06)                       # and some matches are a few pixels off
        kp2[n, j[off]] += (np.round(rng.uniform(3, 12, (int(off.sum()), 1)) * rng.choice((-1, 1), (int(off.sum()), 2)) * 4) / 4).astype(F32)
        p2, z2 = _project(v2, pw[i])
        ray1, ray2 = pw[i] - v1["ow"].astype(F64), pw[i] - v2["ow"].astype(F64)
        par = np.degrees(np.arccos(np.clip((ray1 * ray2).sum(1) / np.linalg.norm(ray1, axis=1) / np.linalg.norm(ray2, axis=1), -1, 1)))
        gross = np.linalg.norm(kp2[n, j].astype(F64) - p2, axis=1) > 20
        clear[n, :len(i)] = np.where(out, gross, exact[i] & (par > 2) & (z2 > 0.5) & ~off)
    S = np.array(S, np.int32)
    if plants:
        # w == 0: the current keyframe's feature at its principal point, neighbour 3 behind a sheared matrix (column 2 of A is zero, exactly)
        i4 = N1 - 1
        k1[i4] = (cx, cy); ur1[i4] = -1; d1[i4] = -1; has1[i4] = 0
        sh = views2[3]
        sh["rcw"] = (np.array([[1, 0, 1], [0, 1, 0], [0, 0, 1]], F64) @ v1["rcw"].astype(F64)).astype(F32)
        sh["tcw"] = _f((0.5, 0.25, 0.0)); sh["ow"] = _f((-0.5, -0.25, 0.0))
        kp2[3, 0] = (float(sh["cx"]) + float(sh["fx"]), float(sh["cy"])); ur2[3, 0] = -1; d2[3, 0] = -1; has2[3, 0] = 0
        pairs[3, 0] = (i4, 0)
        # dist1 == 0: a stereo feature of subnormal depth at the principal point unprojects to the camera centre (identity1 only: the centre is 0)
        i13, n13 = N1 - 2, 0
        k13 = int(np.flatnonzero(pairs[n13, :S[n13], 0] <= i13)[-1])
        j13 = int(pairs[n13, k13, 1])
        pairs[n13, k13, 0] = i13
        k1[i13] = (cx, cy); ur1[i13] = cx - 5; d1[i13] = F32(2.0 ** -130); has1[i13] = 0
        p0, _ = _project(views2[n13], v1["ow"].astype(F64)[None])
        kp2[n13, j13] = np.round(p0[0] * 4) / 4; ur2[n13, j13] = -1; d2[n13, j13] = -1; has2[n13, j13] = 0
        clear[n13, k13] = False
        # UnprojectStereo fails: stereo features without a depth
        for i6 in pairs[0, 5:8, 0]:
            ur1[i6] = 100.0; d1[i6] = 0.0; has1[i6] = 0
        clear[0, 5:8] = False
        # z2 <= 0: points between the image planes of the current keyframe and neighbour 1, which stands 2 cm ahead
        i8 = pairs[1, 20:23, 0]
        for m, (i_, j_) in enumerate(pairs[1, 20:23]):
            X = np.array([[0.001 * m, 0.0, 0.01]])
            k1[i_] = _project(v1, X)[0][0]; ur1[i_] = -1; d1[i_] = -1; has1[i_] = 0
            kp2[1, j_] = _project(views2[1], X)[0][0]; ur2[1, j_] = -1; d2[1, j_] = -1; has2[1, j_] = 0
        # indices out of range: j == n2, j < 0 and (the last slot, so that i still ascends) i == N1
        pairs[1, 3, 1] = N2[1]; pairs[1, 9, 1] = -1; pairs[1, S[1] - 1, 0] = N1
        touched = np.isin(pairs[..., 0], [i4, i13, *pairs[0, 5:8, 0], *i8])      # whatever else matched a planted feature is no clear slot
        clear &= ~touched
        clear[1, [3, 9, S[1] - 1]] = True
    nv = np.ones((Nn,), np.uint8)
    if invalid is not None:
        nv[invalid] = 0
    sf = (F32(SCALE) ** np.arange(NLEVELS)).astype(F32)
    base = {"th_far": TH_FAR, "ratio_factor": F32(1.5) * F32(SCALE), "scale_factors": sf, "level_sigma2": (sf * sf).astype(F32)}
    case = {"view1": v1, "kpts1": k1, "kpts1_raw": None, "octave1": o1, "uright1": ur1, "depth1": d1, "has_mp1": has1, "views2": views2,
            "kpts2": kp2, "kpts2_raw": None, "octave2": o2, "uright2": ur2, "depth2": d2, "has_mp2": has2, "n2": np.array(N2, np.int32),
            "neighbour_valid": nv, "S": S, "pairs": pairs, "clear": clear}
    return base, case


def P(base, far_points=True, inertial=False):
    return params(inertial, far_points, base["th_far"], base["ratio_factor"], base["scale_factors"], base["level_sigma2"])


# ---------------------------------------------------------------- the planted case
# Axis-aligned poses, fx = fy = 256: every figure is exact in fp32 unless a comment says otherwise.  The current keyframe is the world frame
# with cx = 320, cy = 0 (so that an error in y can be any float) and tcw = (0, 0, -0.0); mb = 0.5, mbf = 64.  Scale factors (1, 1.5, 2, 4),
# sigma2 their squares, ratio_factor 2, th_far 16.
def _up(v):
    return np.nextafter(F32(v), F32(np.inf))


def _dn(v):
    return np.nextafter(F32(v), F32(-np.inf))


def _search(fn, start, target, span=200000):
    """the float near `start` at which fn (float32 in, float32 out) gives exactly `target`"""
    x = F32(start)
    cand = (x.view(np.int32) + np.arange(-span, span, dtype=np.int32)).view(F32)
    with np.errstate(all="ignore"):
        hit = np.flatnonzero(fn(cand) == F32(target))
    assert len(hit), (start, target)
    return cand[hit[len(hit) // 2]]


PL_FX, PL_CX1, PL_CY1, PL_CX2, PL_CY2 = 256.0, 320.0, 0.0, 320.0, 240.0
PL_TH_FAR, PL_RATIO = 16.0, 2.0
PL_SF = (1.0, 1.5, 2.0, 4.0)
PLANTED_NEIGHBOURS = ("right", "left", "down", "ahead", "behind", "turned", "sheared")


def planted_case():
    """Returns (base, case, expect): expect maps a slot's name to (n, k, code with inertial off, code with inertial on), far points ON."""
    I = np.eye(3)
    v1 = view(I, (0, 0, -0.0), (0, 0, 0), PL_FX, PL_FX, PL_CX1, PL_CY1, 0.5, 64.0)
    mk = lambda R, t, ow, mb, mbf: view(R, t, ow, PL_FX, PL_FX, PL_CX2, PL_CY2, mb, mbf)   # noqa: E731
    turned = np.array([[1, 0, 0.0], [0, 0, -1], [-0.0, 1, -0.0]])        # a quarter turn about x; the signs of its zeros matter below
    views2 = [mk(I, (0.25, 0, 0), (-0.25, 0, 0), 0.5, 64.0), mk(I, (-0.5, 0, 0), (0.5, 0, 0), 0.5, 64.0), mk(I, (0, 0.5, 0), (0, -0.5, 0), 0.5, 64.0),
              mk(I, (0, 0, -2), (0, 0, 2), 4.0, 128.0),                  # ahead: its own mbf is NOT the current keyframe's
              mk(I, (0, 0, 2), (0, 0, -2), 0.5, 128.0),                  # behind
              mk(turned, (0, 0, 8), (0, -8, -0.0), 8.0, 128.0),
              mk(np.array([[1, 0, 1], [0, 1, 0], [0, 0, 1.0]]), (0.5, 0.25, 0), (-0.5, -0.25, 0), 0.5, 64.0)]
    f1, f2, slots = [], [[] for _ in views2], []                          # features: (kp, raw, octave, uright, depth, has_mp)
    expect, expect_cos = {}, {}

    def feat1(kp, raw=None, octave=0, uright=-1.0, depth=-1.0, has_mp=0):
        f1.append((kp, kp if raw is None else raw, octave, uright, depth, has_mp))
        return len(f1) - 1

    def feat2(n, kp, raw=None, octave=0, uright=-1.0, depth=-1.0, has_mp=0):
        f2[n].append((kp, kp if raw is None else raw, octave, uright, depth, has_mp))
        return len(f2[n]) - 1

    def slot(name, n, i, j, code, code_inertial=None):
        slots.append((n, i, j, name, code, code if code_inertial is None else code_inertial))
    c1, c2 = (PL_CX1, PL_CY1), (PL_CX2, PL_CY2)
    # 1. a feature three neighbours can triangulate (16 px of disparity in each: (0, 0, 4) or (0, 0, 8)); neighbour 0 takes it
    i = feat1(c1)
    slot("claim0", 0, i, feat2(0, (PL_CX2 + 16, PL_CY2)), 0)
    slot("claim1", 1, i, feat2(1, (PL_CX2 - 16, PL_CY2)), CLAIMED)
    slot("claim2", 2, i, feat2(2, (PL_CX2, PL_CY2 + 16)), CLAIMED)
    # 2. cosParallaxRays at the two floats around each literal: xn1 = (a, 0, 1), xn2 = (b, 0, 1), both mono, about 5 px of disparity (a point
    #    12 or 9 m away).  Not every float is the cosine of such a pair: a is stepped until some b gives the target
    def cos_of(a_px, u):
        a, b = (F32(PL_CX1 + a_px) - F32(PL_CX1)) / F32(PL_FX), (u - F32(PL_CX2)) / F32(PL_FX)
        return ((a * b + F32(0)) + F32(1)) / (np.sqrt((a * a + F32(0)) + F32(1)) * np.sqrt((b * b + F32(0)) + F32(1)))
    for name, target, code, code_in in (("cos9998_below", _dn(COS_9998), 0, 5), ("cos9998_at", COS_9998, 5, 5),
                                        ("cos9996_below", _dn(COS_9996), 0, 0), ("cos9996_at", COS_9996, 0, 5)):
        x0 = np.sqrt(1.0 / float(target) ** 2 - 1.0)
        for a_px in range(0, 256, 4):
            try:
                u = _search(lambda uu: cos_of(a_px, uu), PL_CX2 + a_px + PL_FX * x0 * (1 + (a_px / PL_FX) ** 2), target, span=20000)
                break
            except AssertionError:
                continue
        slot(name, 0, feat1((PL_CX1 + a_px, PL_CY1)), feat2(0, (float(u), PL_CY2)), code, code_in)
        expect_cos[name] = target
    # 3. view 1's stereo gate: the point (0, 0, 4) unprojected from the current keyframe (raw keypoint at the principal point, depth 4); its
    #    UNDISTORTED keypoint is off by (2.25, ey) and uright by 1.5, so that the sum is the float below / above 7.8
    lo = F32(CHI2_STEREO) if float(F32(CHI2_STEREO)) <= CHI2_STEREO else _dn(F32(CHI2_STEREO))
    ur_exact = F32(PL_CX1) - F32(64.0) * F32(0.25)
    for name, target, code in (("chi2_stereo_below", lo, 0), ("chi2_stereo_above", _up(lo), 10)):
        ey = _search(lambda e: (F32(2.25) * F32(2.25) + e * e) + F32(1.5) * F32(1.5), np.sqrt(float(target) - 7.3125), target)
        i = feat1((PL_CX1 - 2.25, -float(ey)), raw=c1, uright=float(ur_exact) - 1.5, depth=4.0)
        slot(name, 3, i, feat2(3, c2), code)
    # 4. view 1's mono gate: the same point unprojected from neighbour `behind` (raw keypoint at its principal point, depth 6), the current
    #    keyframe's mono keypoint off by (2.25, ey).  Its uright fits the CURRENT keyframe's mbf (64 / 6), not its own (128 / 6)
    lo = F32(CHI2_MONO) if float(F32(CHI2_MONO)) <= CHI2_MONO else _dn(F32(CHI2_MONO))
    invz6 = (F64(1.0) / F64(6.0)).astype(F32)
    ur6 = F32(PL_CX2) - F32(64.0) * invz6
    for name, target, code in (("chi2_mono_below", lo, 0), ("chi2_mono_above", _up(lo), 9)):
        ey = _search(lambda e: F32(2.25) * F32(2.25) + e * e, np.sqrt(float(target) - 5.0625), target)
        slot(name, 4, feat1((PL_CX1 - 2.25, -float(ey))), feat2(4, c2, uright=float(ur6), depth=6.0), code)
    # 5. z1 == +0: neighbour `behind` unprojects (-1, -1, 2 - 2); z1 == -0: neighbour `turned` unprojects (-1, -4, -0) -- its matrix carries
    #    the zeros' signs -- and 0 * (-1) + 0 * (-4) + 1 * (-0) + (-0) is -0
    slot("z1_zero", 4, feat1((PL_CX1 - 128, PL_CY1 - 128)), feat2(4, (PL_CX2 - 128, PL_CY2 - 128), depth=2.0, uright=100.0), 7)
    slot("z1_minus_zero", 5, feat1((PL_CX1, PL_CY1 + 256)), feat2(5, (PL_CX2 - 64, PL_CY2), depth=4.0, uright=100.0), 7)
    # 6. the far gate: dist1 == th_far and the float below (neighbour `ahead`, dist2 = 14)
    slot("far_at", 3, feat1(c1, uright=float(F32(PL_CX1) - F32(64.0) * (F64(1.0) / F64(16.0)).astype(F32)), depth=16.0), feat2(3, c2), 14)
    zb = _dn(16.0)
    slot("far_below", 3, feat1(c1, uright=float(F32(PL_CX1) - F32(64.0) * (F64(1.0) / F64(zb)).astype(F32)), depth=float(zb)), feat2(3, c2), 0)
    # 7. ratioDist * ratioFactor == ratioOctave: (6 / 8) * 2 == 1.5 / 1 passes
    slot("ratio_equal", 3, feat1(c1, octave=1, uright=float(F32(PL_CX1) - F32(64.0) * F32(0.125)), depth=8.0), feat2(3, c2), 0)
    slot("ratio_fails", 3, feat1(c1, octave=2, uright=float(F32(PL_CX1) - F32(64.0) * F32(0.125)), depth=8.0), feat2(3, c2), 15)
    # 8. w == 0 behind the sheared matrix
    slot("w_zero", 6, feat1(c1), feat2(6, (PL_CX2 + PL_FX, PL_CY2)), 4)
    # 9. a NaN raw keypoint unprojects to a NaN point that no comparison stops
    slot("nan_point", 3, feat1(c1, raw=(float("nan"), 0.0), uright=float(F32(PL_CX1) - F32(64.0) * F32(0.125)), depth=8.0), feat2(3, c2), 0)
    # 10. both views stereo: view 2's parallax (mb 4 at depth 5: 0.72) is far below view 1's, and is never computed -- the point comes from
    #     the current keyframe (0, 0, 8), not from neighbour `ahead` (0, 0, 7)
    invz = (F64(1.0) / F64(6.0)).astype(F32)
    slot("both_stereo", 3, feat1(c1, uright=float(F32(PL_CX1) - F32(64.0) * F32(0.125)), depth=8.0),
         feat2(3, c2, uright=float(F32(PL_CX2) - F32(64.0) * invz), depth=5.0), 0)
    # 11. an index out of range on either side, an existing map point on either side
    slot("i_out_of_range", 3, 4000, feat2(3, c2), 2)
    slot("mp1", 0, feat1(c1, has_mp=1), feat2(0, (PL_CX2 + 16, PL_CY2)), 3)
    slot("mp2", 0, feat1(c1), feat2(0, (PL_CX2 + 16, PL_CY2), has_mp=1), 3)
    slot("j_out_of_range", 0, feat1(c1), 4000, 2)                       # i ascends: after every feature of neighbour 0
    Nn, N1, N2max = len(views2), len(f1), max(len(f) for f in f2)
    per = [sorted((s for s in slots if s[0] == n), key=lambda s: s[1]) for n in range(Nn)]
    Kmax = max(len(p) for p in per) + 1
    pairs = np.full((Nn, Kmax, 2), -7, np.int32)
    for n, p in enumerate(per):
        for k, (_, i, j, name, code, code_in) in enumerate(p):
            pairs[n, k] = (i, j)
            expect[name] = (n, k, code, code_in)

    def cols(fs, n):
        a = {"kp": np.zeros((n, 2), F32), "raw": np.zeros((n, 2), F32), "oct": np.zeros((n,), np.int32), "ur": np.full((n,), -1, F32),
             "dep": np.full((n,), -1, F32), "mp": np.zeros((n,), np.uint8)}
        for r, (kp, raw, o, ur, dep, mp) in enumerate(fs):
            a["kp"][r], a["raw"][r], a["oct"][r], a["ur"][r], a["dep"][r], a["mp"][r] = kp, raw, o, ur, dep, mp
        return a
    a1 = cols(f1, N1)
    a2 = [cols(f, N2max) for f in f2]
    st = lambda k: np.stack([a[k] for a in a2])                          # noqa: E731
    sf = _f(PL_SF)
    base = {"th_far": PL_TH_FAR, "ratio_factor": F32(PL_RATIO), "scale_factors": sf, "level_sigma2": (sf * sf).astype(F32)}
    case = {"view1": v1, "kpts1": a1["kp"], "kpts1_raw": a1["raw"], "octave1": a1["oct"], "uright1": a1["ur"], "depth1": a1["dep"], "has_mp1": a1["mp"],
            "views2": views2, "kpts2": st("kp"), "kpts2_raw": st("raw"), "octave2": st("oct"), "uright2": st("ur"), "depth2": st("dep"),
            "has_mp2": st("mp"), "n2": np.array([len(f) for f in f2], np.int32), "neighbour_valid": None,
            "S": np.array([len(p) for p in per], np.int32), "pairs": pairs}
    case["expect_cos"] = {k: expect[k][:2] + (v,) for k, v in expect_cos.items()}
    return base, case, expect


# ---------------------------------------------------------------- what the test files share
_cases, _cache = {}, {}


def case_of(name):
    """(base, case) of "main" (the shapes of the issue: 640 x 480, Nn = 5, N1 = 1100, Kmax = 1100), "posed" (three neighbours of a current
    keyframe that is NOT the world frame, 300 slots each) or "planted" """
    if name not in _cases:
        if name == "planted":
            _cases[name] = planted_case()[:2]
        elif name == "posed":
            _cases[name] = make_case(3, N1=500, N2=(500, 400, 300), S=(300, 300, 300), Kmax=320, invalid=None, identity1=False, plants=False)
        else:
            _cases[name] = make_case(0)
    return _cases[name]


def solved(name, far_points=True, inertial=False):
    """(P, case, restatement result), computed once per session"""
    key = (name, far_points, inertial)
    if key not in _cache:
        base, c = case_of(name)
        p = P(base, far_points, inertial)
        _cache[key] = (p, c, triangulate(p, c))
    return _cache[key]


def to_capi(p, **kw):
    from rover_slam_amd import capi
    a = dict(inertial=p["inertial"], far_points=p["far_points"], th_far=p["th_far"], ratio_factor=p["ratio_factor"],
             scale_factors=p["scale_factors"], level_sigma2=p["level_sigma2"])
    a.update(kw)
    return capi.tri_params(**a)


def view_to_capi(v):
    from rover_slam_amd import capi
    return capi.tri_view(**{k: v[k] for k in VIEW_KEYS})
