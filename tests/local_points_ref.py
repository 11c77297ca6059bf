"""numpy restatement of steps 2 and 3 of Tracking::SearchLocalPoints (reference src/Tracking.cc:4124-4180), the contract of DESIGN.md 6f:
Frame::isInFrustum (src/Frame.cc:711-794, one pinhole camera) and the head of SPmatcher::SearchByProjection1 (src/Matchers/SPmatcher.cc:
1178-1206) for every local map point as single np.float32 operations in the order the contract writes them, then GetFeaturesInArea, the scan
and the loop's sequential assignment from projection_search_ref (6d).  Shared by test_local_points_ref.py (CPU) and
test_gpu_local_points.py; holds the case generators."""
import numpy as np

import projection_search_ref as PS
import sim3_search_ref as S3

F32 = np.float32
TH_HIGH = PS.TH_HIGH
LEVEL_ZERO, LEVEL_PREDICTED = 0, 1     # RFE_LEVEL_*: SPmatcher.cc:1193 as written / ORB-SLAM3's predicted level
MAX_LEVELS = 16
REJECT = ("searched", "invalid", "z < 0", "outside the image", "distance", "viewing angle", "far point")
# RadiusByViewingCos (SPmatcher.cc:1357-1364) compares the float with the double literal 0.998; fl32(0.998) lies above it
VIEWCOS_NEAR = F32(0.998)
assert float(VIEWCOS_NEAR) > 0.998 > float(np.nextafter(VIEWCOS_NEAR, F32(0))) and VIEWCOS_NEAR.view(np.uint32) == 0x3F7F7CEE


def _f(a):
    return np.asarray(a, F32)


def params(rcw, tcw, ow, intrinsics, mbf, bounds, th, far_points=False, th_far=0.0, scale_factors=(1.0,), log_scale_factor=0.0,
           level_mode=LEVEL_ZERO, view_cos_limit=0.5):
    return {"rcw": _f(rcw).reshape(3, 3), "tcw": _f(tcw), "ow": _f(ow), "intrinsics": tuple(F32(v) for v in intrinsics), "mbf": F32(mbf),
            "bounds": tuple(float(b) for b in bounds), "th": F32(th), "far_points": bool(far_points), "th_far": F32(th_far),
            "scale_factors": _f(scale_factors), "nlevels": len(scale_factors), "log_scale_factor": F32(log_scale_factor),
            "level_mode": level_mode, "view_cos_limit": F32(view_cos_limit)}


def front(P, pw, normal, min_dist, max_dist, scale_dist, valid=None):
    """isInFrustum and the head of SearchByProjection1 for every map point at once.  Returns what one call reports per point -- proj [Np,2],
    proj_xr, depth, view_cos, level (the PREDICTED level in both modes), reject -- and what the search runs on: radius [Np] and search_level
    (None in LEVEL_ZERO, else level)."""
    pw, normal, min_dist, max_dist = _f(pw).reshape(-1, 3), _f(normal).reshape(-1, 3), _f(min_dist).reshape(-1), _f(max_dist).reshape(-1)
    scale_dist = _f(scale_dist).reshape(-1)
    Np = pw.shape[0]
    R, t, ow = P["rcw"], P["tcw"], P["ow"]
    fx, fy, cx, cy = P["intrinsics"]
    min_x, min_y, max_x, max_y = (F32(b) for b in P["bounds"])
    px, py, pz = pw[:, 0], pw[:, 1], pw[:, 2]
    with np.errstate(all="ignore"):
        x = ((R[0, 0] * px + R[0, 1] * py) + R[0, 2] * pz) + t[0]
        y = ((R[1, 0] * px + R[1, 1] * py) + R[1, 2] * pz) + t[1]
        z = ((R[2, 0] * px + R[2, 1] * py) + R[2, 2] * pz) + t[2]
        pc_dist = np.sqrt((x * x + y * y) + z * z)
        invz = F32(1) / z
        u, v = (fx * x) / z + cx, (fy * y) / z + cy
        ox, oy, oz = px - ow[0], py - ow[1], pz - ow[2]
        dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
        cosv = ((ox * normal[:, 0] + oy * normal[:, 1]) + oz * normal[:, 2]) / dist
        c = np.ceil(np.log(scale_dist / dist) / P["log_scale_factor"])
        xr = u - P["mbf"] * invz
        for a in (x, pc_dist, invz, u, dist, cosv, c, xr):
            assert a.dtype == np.float32
        gates = [np.zeros((Np,), bool) if valid is None else np.asarray(valid).reshape(-1) == 0,
                 z < 0,
                 (u < min_x) | (u > max_x) | (v < min_y) | (v > max_y),
                 (dist < min_dist) | (dist > max_dist),
                 cosv < P["view_cos_limit"],
                 (pc_dist > P["th_far"]) if P["far_points"] else np.zeros((Np,), bool)]
    reject = np.zeros((Np,), np.int32)
    for code in (6, 5, 4, 3, 2, 1):                               # the first failure stays
        reject[gates[code - 1]] = code
    seen, ok = (reject == 0) | (reject == 6), reject == 0
    pred = np.where(~(c > 0), 0, np.where(c >= P["nlevels"], P["nlevels"] - 1, np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0))).astype(np.int32)
    level = np.where(seen, pred, -1).astype(np.int32)
    L = level if P["level_mode"] == LEVEL_PREDICTED else np.zeros((Np,), np.int32)
    r0 = np.where(cosv >= VIEWCOS_NEAR, F32(2.5), F32(4.0)).astype(F32)
    radius = np.where(ok, (r0 * P["th"]) * P["scale_factors"][np.maximum(L, 0)], F32(0)).astype(F32)
    proj = np.stack([u, v], 1).astype(F32)
    proj[(reject == 2) | (reject == 3)] = -1
    proj[reject == 1] = 0
    zero = lambda a: np.where(seen, a, F32(0)).astype(F32)   # noqa: E731
    return {"proj": np.ascontiguousarray(proj), "proj_xr": zero(xr), "depth": zero(pc_dist), "view_cos": zero(cosv), "level": level,
            "reject": reject, "radius": radius, "search_level": level if P["level_mode"] == LEVEL_PREDICTED else None}


KEYS = ("assign", "best_idx", "best_dist", "second_dist", "proj", "proj_xr", "depth", "view_cos", "level", "reject")


def search(oracle, P, c, sequential=True, valid="case", nf=None, kxy=False):
    """Everything one call returns (KEYS), nmatches, in_frustum, searched, candidates, lists, radius.  sequential=False: every map point
    scans against the static skip alone.  nf: only the first nf features exist (*nf_dev); kxy: the positions are c["kxy"] read as float."""
    fr = front(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c.get("valid") if isinstance(valid, str) else valid)
    Nf = len(c["desc"])
    n = Nf if nf is None else nf
    kpts = (c["kxy"].astype(F32) if kxy else c["kpts"])[:n]
    octave = None if c.get("octave") is None else c["octave"][:n]
    skip = None if c.get("skip") is None else c["skip"][:n]
    lists = PS.candidate_lists(kpts, octave, P["bounds"], fr["proj"], fr["radius"], fr["search_level"])
    assert all(not l for l, r in zip(lists, fr["reject"]) if r)            # radius 0 keeps nothing
    if sequential:
        r = PS.search_by_projection_seq(oracle, c["q"], c["desc"][:n], lists, skip, c.get("observed"), TH_HIGH)
    else:
        bi, bd, sd = PS.static_scan(oracle, c["q"], c["desc"][:n], lists, skip)
        r = {"assign": np.full((n,), -1, np.int32), "best_idx": bi, "best_dist": bd, "second_dist": sd, "nmatches": -1}
    assign = np.full((Nf,), -1, np.int32)
    assign[:n] = r["assign"]
    out = {k: fr[k] for k in ("proj", "proj_xr", "depth", "view_cos", "level", "reject", "radius")}
    out.update(assign=assign, best_idx=r["best_idx"], best_dist=r["best_dist"], second_dist=r["second_dist"], nmatches=r["nmatches"],
               in_frustum=int(((fr["reject"] == 0) | (fr["reject"] == 6)).sum()), searched=int((fr["reject"] == 0).sum()),
               candidates=sum(len(l) for l in lists), lists=lists)
    return out


# ---------------------------------------------------------------- cases
STEP_MARGIN = S3.STEP_MARGIN
TH_FAR = 8.5


def make_case(seed, W=640, H=480, Nf=1100, Np=2600, nlevels=1, scale_factor=1.2, ncent=40):
    """The tracking case: a frame of Nf quarter-pixel features in groups of four around Nf / 4 sites (clustered descriptors as
    PS.make_case), 15 % of them owned by an observed map point before the call (skip), and Np local map points aimed at the first half of
    the features from depths 2..10 through the inverse of a pose of 0.3 rad and a non-zero translation; 10 % of them have no observation.
    About 5 / 10 / 10 / 19 / 14 % of the points are built to fail gates 1..5; of the rest those deeper than TH_FAR are far points, and
    about half look along their normal (viewCos > 0.998, radius 2.5) while the others do not (radius 4).  With nlevels > 1 the features
    carry random octaves.  Returns (base, case): base holds everything of the params but th, far_points and level_mode (see P());
    case["moved"] counts the points whose mfMaxDistance was scaled by 1.01 to get away from an integer level step."""
    rng = np.random.default_rng(seed)
    quat, t = S3.pose()
    R64 = S3._rot64(quat)
    R = R64.astype(F32)
    ow = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(F32)          # mOw = -Rcw^T tcw, the caller's value
    fx, fy, cx, cy = 420.5, 419.25, 318.75, 241.5
    sf = (F32(scale_factor) ** np.arange(nlevels)).astype(F32)
    base = {"rcw": R, "tcw": t, "ow": ow, "intrinsics": (fx, fy, cx, cy), "mbf": 42.0625, "bounds": (0.0, 0.0, float(W), float(H)),
            "scale_factors": sf, "log_scale_factor": np.log(F32(scale_factor)).astype(F32), "th_far": TH_FAR}
    nsite = max(Nf // 4, 1)
    site = np.stack([rng.uniform(20, W - 20, nsite), rng.uniform(20, H - 20, nsite)], 1)
    kpts = site[np.arange(Nf) % nsite] + rng.uniform(-8, 8, (Nf, 2))
    kpts = (np.round(kpts * 4) / 4).astype(F32)                                  # quarter pixels: exact in fp32
    centre = rng.standard_normal((ncent, 256)).astype(F32)
    cluster = (kpts[:, 0].astype(np.int64) // 32 + 5 * (kpts[:, 1].astype(np.int64) // 30)) % ncent
    desc = centre[cluster] + F32(0.03) * rng.standard_normal((Nf, 256)).astype(F32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    skip = (rng.random(Nf) < 0.15).astype(np.uint8)
    octave = rng.integers(0, nlevels, Nf).astype(np.int32) if nlevels > 1 else None
    src = rng.integers(0, max(Nf // 2, 1), Np)
    q = (desc[src] + F32(0.02) * rng.standard_normal((Np, 256)).astype(F32)).astype(F32)
    observed = (rng.random(Np) < 0.9).astype(np.uint8)
    kind = rng.choice(6, Np, p=(0.42, 0.05, 0.10, 0.10, 0.19, 0.14))            # the gate the point is built to stop at (0: none)
    uv = kpts[src].astype(np.float64) + rng.uniform(-3, 3, (Np, 2))
    out = kind == 3                                                              # aimed past one of the four borders
    side = rng.integers(0, 4, Np); far = rng.uniform(1, 200, Np)
    uv[out & (side == 0), 0] = -far[out & (side == 0)]; uv[out & (side == 1), 0] = W + far[out & (side == 1)]
    uv[out & (side == 2), 1] = -far[out & (side == 2)]; uv[out & (side == 3), 1] = H + far[out & (side == 3)]
    depth = rng.uniform(2, 10, Np) * np.where(kind == 2, -1.0, 1.0)
    pc = np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth, depth], 1)
    pw = ((pc - t.astype(np.float64)) @ R64).astype(F32)                         # R^T (pc - t), row by row
    po = pw.astype(np.float64) - ow.astype(np.float64)
    dist = np.sqrt((po * po).sum(1))
    away = np.where(kind == 5, -1.0, 1.0)[:, None]                               # 5: the normal looks the other way
    spread = np.where(rng.random(Np) < 0.5, 0.02, 0.3)[:, None]                  # along the normal (viewCos > 0.998) or not
    nrm = away * po / dist[:, None] + spread * rng.standard_normal((Np, 3))
    normal = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    min_dist = (dist * 0.5).astype(F32)
    # mfMaxDistance: from 0.91 of the distance (inside the gate's 1.2f, and level 0) up to past the last level's step
    scale_dist = (dist * float(scale_factor) ** rng.uniform(-0.5, max(nlevels, 2) - 0.5, Np)).astype(F32)
    near = (kind == 4) & (rng.random(Np) < 0.5)
    min_dist[near] = (dist[near] * 1.1).astype(F32)                              # 4: closer than the invariance region ...
    scale_dist[(kind == 4) & ~near] = (dist[(kind == 4) & ~near] * 0.75).astype(F32)   # ... or farther: 1.2f * 0.75 = 0.9 of the distance
    valid = (kind != 1).astype(np.uint8)
    steps = S3.level_steps(base, pw, scale_dist)
    close = np.abs(steps - np.round(steps)) < STEP_MARGIN
    scale_dist[close] = (scale_dist[close] * F32(1.01)).astype(F32)
    steps = S3.level_steps(base, pw, scale_dist)
    assert not (np.abs(steps - np.round(steps)) < STEP_MARGIN).any()
    max_dist = (F32(1.2) * scale_dist).astype(F32)                               # GetMaxDistanceInvariance(), src/MapPoint.cc:668-672
    case = {"kpts": np.ascontiguousarray(kpts), "kxy": np.ascontiguousarray(np.round(kpts).astype(np.int32)), "desc": np.ascontiguousarray(desc),
            "skip": skip, "octave": octave, "q": np.ascontiguousarray(q), "observed": observed, "pw": np.ascontiguousarray(pw),
            "normal": np.ascontiguousarray(normal), "min_dist": min_dist, "max_dist": max_dist, "scale_dist": scale_dist, "valid": valid,
            "src": src, "kind": kind, "moved": int(close.sum())}
    return base, case


def P(base, th, far_points=True, level_mode=LEVEL_ZERO):
    return params(base["rcw"], base["tcw"], base["ow"], base["intrinsics"], base["mbf"], base["bounds"], th, far_points, base["th_far"],
                  base["scale_factors"], base["log_scale_factor"], level_mode)


# the planted case: identity pose, power-of-two intrinsics and distances -- every figure below is exact in fp32.  With z = 4 a point
# (x, y, 4) projects to (64 x + 320, 64 y + 240); th = 1, so the radius is 2.5 or 4
_UP = lambda v: float(np.nextafter(F32(v), F32(np.inf)))   # noqa: E731
_DN = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))  # noqa: E731
_C = float(VIEWCOS_NEAR)
_S = 0.0625                                  # the x component of the two normals around the threshold: PO . n does not see it
NAN = float("nan")
PLANTED_BOUNDS = (0.0, 0.0, 640.0, 480.0)
PLANTED_TH_FAR = 8.0
# ((world point, normal, min_dist, max_dist, valid, observed), expected reject code)
PLANTED_POINTS = (
    (((5.0, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),             # 0: u = 640 = max_x: the gate is closed, inside
    (((5.0 + 2.0 ** -20, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 3),  # 1: u = 640 + 2^-14, one ulp above max_x
    (((-5.0, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),            # 2: u = 0 = min_x: inside; takes feature 1
    (((1.0, 1.0, 0.0), (0, 0, 1), 0.0, 99.0, 1, 1), 3),             # 3: z == 0 passes the depth gate, u = +inf
    (((1.0, 1.0, -0.0), (0, 0, 1), 0.0, 99.0, 1, 1), 3),            # 4: z == -0 is not < 0, u = -inf
    (((0.0, 0.0, -2.0), (0, 0, -1), 0.0, 99.0, 1, 1), 2),           # 5: z < 0
    (((NAN, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),             # 6: a NaN coordinate (0 * NaN: all of Pc) fails no comparison: searched, no candidates
    (((0.0, 0.0, 4.0), (0, 0, 1), 4.0, 99.0, 1, 1), 0),             # 7: dist == min_dist
    (((0.0, 0.0, 4.0), (0, 0, 1), _UP(4.0), 99.0, 1, 1), 4),        # 8: dist one ulp below min_dist
    (((3.0, 0.0, 4.0), (0, 0, 1), 1.0, 5.0, 1, 1), 0),              # 9: dist == max_dist (3, 4, 5)
    (((3.0, 0.0, 4.0), (0, 0, 1), 1.0, _DN(5.0), 1, 1), 4),         # 10: dist one ulp above max_dist
    (((0.0, 0.0, 4.0), (0, 0, 0.5), 0.0, 99.0, 1, 1), 0),           # 11: viewCos == 0.5f
    (((0.0, 0.0, 4.0), (0, 0, _DN(0.5)), 0.0, 99.0, 1, 1), 5),      # 12: viewCos one ulp below 0.5
    (((0.0, 0.0, 4.0), (_S, 0, _C), 0.0, 99.0, 1, 1), 0),           # 13: viewCos == fl32(0.998) > 0.998: radius 2.5, feature 0 out of reach
    (((0.0, 0.0, 4.0), (_S, 0, _DN(_C)), 0.0, 99.0, 1, 1), 0),      # 14: its lower neighbour: radius 4, takes feature 0
    (((0.0, 0.0, 8.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),             # 15: depth == th_far
    (((0.0, 0.0, _UP(8.0)), (0, 0, 1), 0.0, 99.0, 1, 1), 6),        # 16: depth one ulp above th_far: in the frustum, not searched
    (((1.0, 1.0, 4.0), (0, 0, 1), 0.0, 99.0, 0, 1), 1),             # 17: invalid; it would take feature 2 before point 18
    (((1.0, 1.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),             # 18: takes feature 2
    (((-1.0, 1.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 0), 0),            # 19: no observations: takes feature 4 and does not block it
    (((-1.0, 1.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),            # 20: takes feature 4 over point 19
    (((-1.0, 1.0, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),            # 21: feature 4 is blocked now: the near copy, feature 5
    (((0.0, 3.75, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),            # 22: v = 480 = max_y: inside
    (((0.0, -3.75, 4.0), (0, 0, 1), 0.0, 99.0, 1, 1), 0),           # 23: v = 0 = min_y: inside; feature 6 there is skipped
)
# feature 0 lies 3 pixels from the centre: inside radius 4, outside 2.5
PLANTED_FEATURES = ((323.0, 240.0), (1.0, 240.0), (385.0, 305.0), (386.0, 303.0), (257.0, 305.0), (255.0, 303.0), (321.0, 1.0), (600.0, 20.0))
PLANTED_SKIP = (0, 0, 0, 0, 0, 0, 1, 0)
PLANTED_CARRIES = {13: 0, 14: 0, 2: 1, 17: 2, 18: 2, 19: 4, 20: 4, 21: 4, 23: 6}       # map point -> the feature whose descriptor it carries
PLANTED_ASSIGN = (14, 2, 18, -1, 20, 21, -1, -1)
PLANTED_NMATCHES = 6                                                                   # points 2, 14, 18, 19 (overwritten), 20, 21


def planted_case():
    base = {"rcw": np.eye(3, dtype=F32), "tcw": np.zeros(3, F32), "ow": np.zeros(3, F32), "intrinsics": (256.0, 256.0, 320.0, 240.0), "mbf": 64.0,
            "bounds": PLANTED_BOUNDS, "scale_factors": np.ones(1, F32), "log_scale_factor": F32(0), "th_far": PLANTED_TH_FAR}
    rng = np.random.default_rng(77)
    desc = rng.standard_normal((len(PLANTED_FEATURES), 256)).astype(F32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    for a, b in ((3, 2), (5, 4)):                                   # near copies
        desc[a] = desc[b] + F32(0.005) * rng.standard_normal(256).astype(F32)
        desc[a] = desc[a] / np.linalg.norm(desc[a])
    q = rng.standard_normal((len(PLANTED_POINTS), 256)).astype(F32)
    q = (F32(3) * q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)    # length 3: at least 2 from every feature, never accepted
    for i, j in PLANTED_CARRIES.items():
        q[i] = desc[j]
    pts = [p for p, _ in PLANTED_POINTS]
    kpts = np.array(PLANTED_FEATURES, F32)
    case = {"kpts": kpts, "kxy": kpts.astype(np.int32), "desc": np.ascontiguousarray(desc), "q": np.ascontiguousarray(q),
            "skip": np.array(PLANTED_SKIP, np.uint8), "octave": None, "observed": np.array([p[5] for p in pts], np.uint8),
            "pw": np.array([p[0] for p in pts], F32), "normal": np.array([p[1] for p in pts], F32), "min_dist": np.array([p[2] for p in pts], F32),
            "max_dist": np.array([p[3] for p in pts], F32), "scale_dist": np.array([p[3] for p in pts], F32),
            "valid": np.array([p[4] for p in pts], np.uint8)}
    return base, case


# ---------------------------------------------------------------- what both test files share: solved cases, the binding, the C++ driver
_cases, _cache = {}, {}


def case_of(name):
    """(base, case) of "main" (640 x 480, Nf = 1100, Np = 2600, one level), "main8" (eight levels, scale factor 1.2, octaves) or "planted" """
    if name not in _cases:
        _cases[name] = planted_case() if name == "planted" else make_case(0, nlevels=8 if name == "main8" else 1)
    return _cases[name]


def solved(oracle, name, th=1, far_points=True, level_mode=LEVEL_ZERO, sequential=True):
    """(P, case, restatement result), computed once per session"""
    key = (name, th, far_points, level_mode, sequential)
    if key not in _cache:
        base, c = case_of(name)
        p = P(base, th, far_points, level_mode)
        _cache[key] = (p, c, search(oracle, p, c, sequential))
    return _cache[key]


def to_capi(p, **kw):
    from rover_slam_amd import capi
    return capi.frustum_params(p["rcw"], p["tcw"], p["ow"], p["intrinsics"], p["mbf"], p["bounds"], p["th"], p["far_points"], p["th_far"],
                               p["scale_factors"], p["log_scale_factor"], p["level_mode"], p["view_cos_limit"], **kw)


FIELDS = ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "level", "view_cos", "visible")


def map_point_fields(ref, before):
    """What SearchLocalPoints_rfe leaves in every map point, from one call's outputs and the fields' values before it (a dict of arrays named
    FIELDS): an invalid point is not touched; isInFrustum resets mbTrackInView / mTrackProjX / mTrackProjY first (Frame.cc:711-713), stores
    the projection behind the image gate (:740-741) and the rest behind the last gate (:778-791)."""
    rej = ref["reject"]
    touched, past_image, seen = rej != 1, (rej != 1) & (rej != 2) & (rej != 3), (rej == 0) | (rej == 6)
    out = {k: np.array(before[k]) for k in FIELDS}
    out["in_view"][touched] = seen[touched]
    out["proj_x"][touched] = -1; out["proj_y"][touched] = -1
    out["proj_x"][past_image] = ref["proj"][past_image, 0]; out["proj_y"][past_image] = ref["proj"][past_image, 1]
    for k in ("proj_xr", "depth", "view_cos", "level"):
        out[k][seen] = ref[k][seen]
    out["visible"][seen] += 1
    return out


def write_driver_case(path, p, c, nleft=-1, frame_id=7):
    """a case as tests/cpp/local_points_driver.cpp reads it.  An invalid map point is bad (even index) or was seen in this frame already
    (odd index); a skipped feature holds an observed map point that is not in the list, every fourth other feature an unobserved one.
    Returns the fields of every map point before the call (stale values that the call must leave or replace as the reference does) and
    what F.mvpMapPoints holds before it (-1 NULL, -2 the observed other, -3 the unobserved other)."""
    Np, Nf = len(c["pw"]), len(c["kpts"])
    invalid = c["valid"] == 0
    bad = (invalid & (np.arange(Np) % 2 == 0)).astype(np.uint8)
    last_seen = np.where(invalid & (np.arange(Np) % 2 == 1), frame_id, frame_id - 1).astype(np.int32)
    prior = np.where(c["skip"] != 0, -2, np.where(np.arange(Nf) % 4 == 0, -3, -1)).astype(np.int32)
    rng = np.random.default_rng(5)
    before = {"in_view": (rng.random(Np) < 0.5), "proj_x": rng.uniform(0, 600, Np).astype(F32), "proj_y": rng.uniform(0, 400, Np).astype(F32),
              "proj_xr": rng.uniform(0, 600, Np).astype(F32), "depth": rng.uniform(1, 9, Np).astype(F32), "level": rng.integers(0, 8, Np).astype(np.int32),
              "view_cos": rng.uniform(0.5, 1, Np).astype(F32), "visible": rng.integers(1, 50, Np).astype(np.int32)}
    octave = np.zeros((Nf,), np.int32) if c.get("octave") is None else c["octave"]
    with open(path, "wb") as f:
        np.array([Np, Nf, nleft, p["nlevels"], int(p["far_points"]), frame_id], np.int32).tofile(f)
        np.array([*p["rcw"].reshape(-1), *p["tcw"], *p["ow"], *p["intrinsics"], p["mbf"], *p["bounds"], p["log_scale_factor"], p["th"], p["th_far"]],
                 np.float32).tofile(f)
        p["scale_factors"].astype(np.float32).tofile(f); bad.tofile(f); last_seen.tofile(f); c["observed"].astype(np.uint8).tofile(f)
        before["in_view"].astype(np.uint8).tofile(f)
        for k in ("proj_x", "proj_y", "proj_xr", "depth", "level", "view_cos", "visible"):
            before[k].tofile(f)
        prior.tofile(f); octave.astype(np.int32).tofile(f)
        for k in ("pw", "normal", "min_dist", "max_dist", "scale_dist", "q", "kpts", "desc"):
            c[k].astype(np.float32).tofile(f)
    return before, prior


def read_driver_out(path, Np, Nf):
    """the driver's dump: the return value, nToMatch, F.mvpMapPoints, then the fields of every map point"""
    raw = np.fromfile(path, np.uint8)
    hd = raw[:8].view(np.int32)
    o = 8
    who = raw[o:o + 4 * Nf].view(np.int32); o += 4 * Nf
    got = {"in_view": raw[o:o + Np].astype(bool)}; o += Np
    for k, dt in (("proj_x", F32), ("proj_y", F32), ("proj_xr", F32), ("depth", F32), ("level", np.int32), ("view_cos", F32), ("visible", np.int32)):
        got[k] = raw[o:o + 4 * Np].view(dt); o += 4 * Np
    assert o == len(raw)
    return int(hd[0]), int(hd[1]), who, got
