"""numpy restatement of the two Sim3 SearchByProjection overloads of loop closing (reference src/Matchers/SPmatcher.cc:1558-1669 and
:2076-2182), the contract of DESIGN.md 6e: the front of the loop (Sophus' SE3f * p, the projection, the gates, MapPoint::PredictScale, the
radius) as single np.float32 operations in the order the reference writes them, then KeyFrame::GetFeaturesInArea, the scan and the loop's
sequential assignment from projection_search_ref (6d) with every map point observed.  Shared by test_sim3_search_ref.py (CPU) and
test_gpu_sim3_search.py."""
import numpy as np

import projection_search_ref as PS

F32 = np.float32
TH_LOW = F32(1.2)                      # SPmatcher::TH_LOW
PROJ_INVZ, PROJ_DIV = 0, 1             # RFE_PROJ_*: SPmatcher.cc:1596-1601 / Pinhole::project
DIST_FLOAT, DIST_TRUNC = 0, 1          # RFE_DIST_*: `float dist` (:1650) / `int dist` (:2164)
MAX_LEVELS = 16
REJECT = ("searched", "invalid", "z < 0", "outside the image", "distance", "viewing angle")


def _f(a):
    return np.asarray(a, F32)


def cross(a, b):
    """Eigen's cross product, component by component: a [3] (or [N,3]) x b [N,3]"""
    a, b = _f(a), _f(b)
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], -1).astype(F32)


def rotate(quat, p):
    """Sophus::SO3f * p (so3.hpp:358-367): uv = qv x p; uv += uv; p + qw * uv + qv x uv, every operation one fp32 rounding"""
    quat, p = _f(quat), _f(p).reshape(-1, 3)
    qv, qw = quat[:3], quat[3]
    uv = cross(qv, p)
    uv = uv + uv
    return ((p + qw * uv) + cross(qv, uv)).astype(F32)


def inverse_translation(quat, t):
    """Tcw.inverse().translation() = -(R^T t), with R^T applied as the conjugate quaternion through rotate()"""
    quat = _f(quat)
    conj = np.array([-quat[0], -quat[1], -quat[2], quat[3]], F32)
    return (-rotate(conj, _f(t).reshape(1, 3))[0]).astype(F32)


def params(quat, t, intrinsics, bounds, th, scale_factors=(1.0,), log_scale_factor=0.0, proj_mode=PROJ_INVZ, ow=None):
    quat, t = _f(quat), _f(t)
    return {"quat": quat, "t": t, "ow": inverse_translation(quat, t) if ow is None else _f(ow), "intrinsics": tuple(F32(v) for v in intrinsics),
            "bounds": tuple(float(b) for b in bounds), "th": int(th), "scale_factors": _f(scale_factors), "nlevels": len(scale_factors),
            "log_scale_factor": F32(log_scale_factor), "proj_mode": proj_mode}


def project(P, pw, normal, min_dist, max_dist, scale_dist, valid=None):
    """The front of the loop for every map point at once.  Returns proj [Np,2], radius [Np], level [Np] and reject [Np] (0 = searched, else
    the first gate that failed); a rejected point has proj (0, 0), radius 0, level -1.  max_dist is GetMaxDistanceInvariance() = 1.2f *
    mfMaxDistance, which the distance gate compares with; scale_dist is the bare mfMaxDistance, which PredictScale divides by the distance."""
    pw, normal, min_dist, max_dist = _f(pw).reshape(-1, 3), _f(normal).reshape(-1, 3), _f(min_dist).reshape(-1), _f(max_dist).reshape(-1)
    scale_dist = _f(scale_dist).reshape(-1)
    Np = pw.shape[0]
    fx, fy, cx, cy = P["intrinsics"]
    min_x, min_y, max_x, max_y = (F32(b) for b in P["bounds"])
    with np.errstate(all="ignore"):
        pc = (rotate(P["quat"], pw) + P["t"]).astype(F32)
        x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
        if P["proj_mode"] == PROJ_INVZ:
            invz = F32(1) / z
            u, v = fx * (x * invz) + cx, fy * (y * invz) + cy
        else:
            u, v = (fx * x) / z + cx, (fy * y) / z + cy
        po = (pw - P["ow"]).astype(F32)
        dist = np.sqrt((po[:, 0] * po[:, 0] + po[:, 1] * po[:, 1]) + po[:, 2] * po[:, 2]).astype(F32)
        dot = ((po[:, 0] * normal[:, 0] + po[:, 1] * normal[:, 1]) + po[:, 2] * normal[:, 2]).astype(F32)
        c = np.ceil(np.log(scale_dist / dist).astype(F32) / P["log_scale_factor"]).astype(F32)
        gates = [np.zeros((Np,), bool) if valid is None else np.asarray(valid).reshape(-1) == 0,
                 z < 0,
                 ~((u >= min_x) & (u < max_x) & (v >= min_y) & (v < max_y)),
                 (dist < min_dist) | (dist > max_dist),
                 dot < F32(0.5) * dist]
    reject = np.zeros((Np,), np.int32)
    for code in (5, 4, 3, 2, 1):                                  # the first failure stays
        reject[gates[code - 1]] = code
    ok = reject == 0
    level = np.where(~(c > 0), 0, np.where(c >= P["nlevels"], P["nlevels"] - 1, np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0))).astype(np.int32)
    level = np.where(ok, level, -1).astype(np.int32)
    radius = np.where(ok, F32(P["th"]) * P["scale_factors"][np.maximum(level, 0)], F32(0)).astype(F32)
    proj = np.where(ok[:, None], np.stack([u, v], 1), F32(0)).astype(F32)
    return {"proj": np.ascontiguousarray(proj), "radius": radius, "level": level, "reject": reject}


def level_steps(P, pw, scale_dist):
    """log(ratio) / log_scale_factor of every map point in float64: logf is not correctly rounded on either side, so a case keeps its
    searched points away from the integers, where ceil() would turn one ulp into a level"""
    po = np.asarray(pw, np.float64).reshape(-1, 3) - np.asarray(P["ow"], np.float64)
    with np.errstate(all="ignore"):
        return np.log(np.asarray(scale_dist, np.float64) / np.sqrt((po * po).sum(1))) / float(P["log_scale_factor"])


def _sequence(lists, dist, blocked0, th_accept, Nf, sequential=True):
    """the reference's loop on stored distances (PS._scan is the scan of 6d: strict <, so the FIRST least distance wins)"""
    out = PS._out(len(lists), Nf)
    blocked = np.zeros((max(Nf, 1),), bool) if blocked0 is None else np.asarray(blocked0).astype(bool).copy()
    for i, (cl, dl) in enumerate(zip(lists, dist)):
        bi, bd, sd = PS._scan(cl, dl, lambda j: blocked[j])
        out["best_idx"][i], out["best_dist"][i], out["second_dist"][i] = bi, bd, sd
        if bd <= F32(th_accept):
            out["assign"][bi] = i
            out["nmatches"] += 1
            if sequential:
                blocked[bi] = True                                 # vpMatched[bestIdx] = pMP: `if(vpMatched[idx]) continue;` from now on
    return out


def search(oracle, P, c, dist_mode=DIST_FLOAT, th_accept=TH_LOW, sequential=True, valid="case"):
    """Everything one call returns: proj / radius / level / reject, matched [Nf], best_idx / best_dist / second_dist [Np], nmatches,
    searched, candidates, lists.  sequential=False: every map point scans against matched_in alone (what the sequence is compared with)."""
    front = project(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c.get("valid") if isinstance(valid, str) else valid)
    lists = PS.candidate_lists(c["kpts"], None, P["bounds"], front["proj"], front["radius"])
    Nf = len(c["kpts"])
    assert all(not l for l, r in zip(lists, front["reject"]) if r)         # radius 0 keeps nothing
    if dist_mode == DIST_FLOAT and sequential:
        r = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists, c.get("matched_in"), None, th_accept)
    else:
        dist = PS.candidate_distances(oracle, c["q"], c["desc"], lists)
        if dist_mode == DIST_TRUNC:
            dist = [np.trunc(d).astype(F32) for d in dist]            # int dist = DescriptorDistance_sp(...): toward zero
        r = _sequence(lists, dist, c.get("matched_in"), th_accept, Nf, sequential)
    out = dict(front, matched=r["assign"], best_idx=r["best_idx"], best_dist=r["best_dist"], second_dist=r["second_dist"], nmatches=r["nmatches"],
               searched=int((front["reject"] == 0).sum()), candidates=sum(len(l) for l in lists), lists=lists)
    return out


KEYS = ("matched", "best_idx", "best_dist", "second_dist", "proj", "radius", "level", "reject")


# ---------------------------------------------------------------- cases
def pose(angle=0.3, axis=(0.2, 1.0, 0.1), t=(0.3, -0.2, 0.5)):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    quat = np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]]).astype(F32)
    quat = (quat / np.sqrt((quat.astype(np.float64) ** 2).sum())).astype(F32)
    return quat, np.asarray(t, F32)


def _rot64(quat):
    x, y, z, w = (float(v) for v in quat)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


STEP_MARGIN = 1e-3          # a few ulp of logf are about 1e-7 of a level step here: three orders of magnitude inside the margin


def make_case(seed, W=640, H=480, Nf=1100, Np=2600, th=10, nlevels=1, scale_factor=1.2, proj_mode=PROJ_INVZ, ncent=40):
    """The loop-closing case: a keyframe of Nf quarter-pixel features in groups of four around Nf / 4 sites (clustered descriptors as
    PS.make_case: a block of 32 x 30 pixels shares a centre), 15 % of them matched before the call, and Np map points aimed at the first
    half of the features from random depths through the inverse of a pose of 0.3 rad and a non-zero translation.  About 5 / 10 / 10 / 19 /
    14 % of the points are built to fail gates 1..5, the rest reach the search.  Returns (P, case); case["moved"] counts the points whose
    mfMaxDistance was scaled by 1.01 to get away from an integer level step."""
    rng = np.random.default_rng(seed)
    quat, t = pose()
    fx, fy, cx, cy = 420.5, 419.25, 318.75, 241.5
    sf = (F32(scale_factor) ** np.arange(nlevels)).astype(F32)
    P = params(quat, t, (fx, fy, cx, cy), (0.0, 0.0, float(W), float(H)), th, sf, np.log(F32(scale_factor)).astype(F32), proj_mode)
    nsite = max(Nf // 4, 1)
    site = np.stack([rng.uniform(20, W - 20, nsite), rng.uniform(20, H - 20, nsite)], 1)
    kpts = site[np.arange(Nf) % nsite] + rng.uniform(-8, 8, (Nf, 2))
    kpts = (np.round(kpts * 4) / 4).astype(F32)                                  # quarter pixels: exact in fp32
    centre = rng.standard_normal((ncent, 256)).astype(F32)
    cluster = (kpts[:, 0].astype(np.int64) // 32 + 5 * (kpts[:, 1].astype(np.int64) // 30)) % ncent
    desc = centre[cluster] + F32(0.03) * rng.standard_normal((Nf, 256)).astype(F32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    matched_in = (rng.random(Nf) < 0.15).astype(np.uint8)
    src = rng.integers(0, max(Nf // 2, 1), Np)
    q = (desc[src] + F32(0.02) * rng.standard_normal((Np, 256)).astype(F32)).astype(F32)
    kind = rng.choice(6, Np, p=(0.42, 0.05, 0.10, 0.10, 0.19, 0.14))            # the gate the point is built to stop at (0: none)
    uv = kpts[src].astype(np.float64) + rng.uniform(-3, 3, (Np, 2))
    out = kind == 3                                                              # aimed past one of the four borders
    side = rng.integers(0, 4, Np); far = rng.uniform(1, 200, Np)
    uv[out & (side == 0), 0] = -far[out & (side == 0)]; uv[out & (side == 1), 0] = W + far[out & (side == 1)]
    uv[out & (side == 2), 1] = -far[out & (side == 2)]; uv[out & (side == 3), 1] = H + far[out & (side == 3)]
    depth = rng.uniform(2, 10, Np) * np.where(kind == 2, -1.0, 1.0)
    pc = np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth, depth], 1)
    R = _rot64(quat)
    pw = ((pc - t.astype(np.float64)) @ R).astype(F32)                           # R^T (pc - t), row by row
    po = pw.astype(np.float64) - P["ow"].astype(np.float64)
    dist = np.sqrt((po * po).sum(1))
    away = np.where(kind == 5, -1.0, 1.0)[:, None]                               # 5: the normal looks the other way
    nrm = away * po / dist[:, None] + 0.3 * rng.standard_normal((Np, 3))
    normal = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    min_dist = (dist * 0.5).astype(F32)
    # mfMaxDistance: from 0.91 of the distance (inside the gate's 1.2f, and level 0) up to past the last level's step
    scale_dist = (dist * float(scale_factor) ** rng.uniform(-0.5, max(nlevels, 2) - 0.5, Np)).astype(F32)
    near = (kind == 4) & (rng.random(Np) < 0.5)
    min_dist[near] = (dist[near] * 1.1).astype(F32)                              # 4: closer than the invariance region ...
    scale_dist[(kind == 4) & ~near] = (dist[(kind == 4) & ~near] * 0.75).astype(F32)   # ... or farther: 1.2f * 0.75 = 0.9 of the distance
    valid = (kind != 1).astype(np.uint8)
    steps = level_steps(P, pw, scale_dist)
    close = np.abs(steps - np.round(steps)) < STEP_MARGIN
    scale_dist[close] = (scale_dist[close] * F32(1.01)).astype(F32)
    steps = level_steps(P, pw, scale_dist)
    assert not (np.abs(steps - np.round(steps)) < STEP_MARGIN).any()
    max_dist = (F32(1.2) * scale_dist).astype(F32)                               # GetMaxDistanceInvariance(), src/MapPoint.cc:668-672
    case = {"kpts": np.ascontiguousarray(kpts), "desc": np.ascontiguousarray(desc), "matched_in": matched_in, "q": np.ascontiguousarray(q),
            "pw": np.ascontiguousarray(pw), "normal": np.ascontiguousarray(normal), "min_dist": min_dist, "max_dist": max_dist, "scale_dist": scale_dist,
            "valid": valid, "src": src, "kind": kind, "moved": int(close.sum())}
    return P, case


# the planted case: identity rotation, t = 0, power-of-two intrinsics -- every projection below is exact in fp32 in both forms
PLANTED_BOUNDS = (0.0, 0.0, 640.0, 480.0)
PLANTED_POINTS = (                       # (world point, normal, min_dist, max_dist, valid), expected reject code
    (((5.0, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1), 3),        # 0: u = 256 * 1.25 + 320 = 640 = max_x: half open, outside
    (((-5.0, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1), 0),       # 1: u = 0 = min_x: inside
    (((1.0, 1.0, 0.0), (0, 0, 1), 0.0, 99.0, 1), 3),        # 2: z == 0 passes the depth gate and fails IsInImage through inf
    (((0.0, 0.0, -2.0), (0, 0, -1), 0.0, 99.0, 1), 2),      # 3: z < 0
    (((0.0, 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 0), 1),        # 4: invalid; it would take feature 1 (its own descriptor) before point 5
    (((0.0, 0.0, 4.0), (0, 0, 1), 4.0, 99.0, 1), 0),        # 5: dist == min_dist
    (((3.0, 0.0, 4.0), (0, 0, 1), 1.0, 5.0, 1), 0),         # 6: dist == max_dist (3, 4, 5)
    (((0.0, 3.0, 4.0), (0, 0, 0.625), 0.0, 99.0, 1), 0),    # 7: PO . n = 2.5 = 0.5 * dist
    (((0.0, 3.0, 4.0), (0, 0, 0.5), 0.0, 99.0, 1), 5),      # 8: PO . n = 2.0 < 2.5
    (((0.0, 3.75, 4.0), (0, 0, 1), 0.0, 99.0, 1), 3),       # 9: v = 256 * 0.9375 + 240 = 480 = max_y
    (((0.0, -3.75, 4.0), (0, 0, 1), 0.0, 99.0, 1), 0),      # 10: v = 0 = min_y
    (((0.0, 0.0, 4.0), (0, 0, 1), 4.5, 99.0, 1), 4),        # 11: dist < min_dist
    (((0.0, 0.0, 4.0), (0, 0, 1), 0.0, 3.5, 1), 4),         # 12: dist > max_dist
    (((0.0, 0.0, -0.0), (0, 0, 1), 0.0, 99.0, 1), 3),       # 13: z == -0: not < 0, then NaN
    (((float("nan"), 0.0, 4.0), (0, 0, 1), 0.0, 99.0, 1), 3),   # 14: a NaN coordinate fails IsInImage
    (((1.0, 1.0, 4.0), (0, 0, 1), 0.0, 99.0, 1), 0),        # 15: an ordinary point on feature 6
)
PLANTED_FEATURES = ((0.0, 240.0), (320.0, 240.0), (512.0, 240.0), (320.0, 432.0), (320.0, 0.0), (325.0, 243.0), (384.0, 304.0), (600.0, 20.0))
PLANTED_WANT = {1: 0, 5: 5, 6: 2, 7: 3, 10: 4, 15: 6}       # searched point -> the feature whose descriptor it carries
# feature 5 (325, 243) was matched before the call: point 5, which carries its descriptor, takes feature 1 (a near copy) instead -- and the
# invalid point 4, which carries feature 1's descriptor exactly, would have taken it first
PLANTED_MATCHED = (1, 5, 6, 7, 10, -1, 15, -1)


def planted_case(proj_mode=PROJ_INVZ):
    P = params((0, 0, 0, 1), (0, 0, 0), (256.0, 256.0, 320.0, 240.0), PLANTED_BOUNDS, 10, (1.0,), 0.0, proj_mode, ow=(0, 0, 0))
    rng = np.random.default_rng(77)
    desc = rng.standard_normal((len(PLANTED_FEATURES), 256)).astype(F32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    q = rng.standard_normal((len(PLANTED_POINTS), 256)).astype(F32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    desc[1] = desc[5] + F32(0.005) * rng.standard_normal(256).astype(F32)
    desc[1] = desc[1] / np.linalg.norm(desc[1])
    for i, j in PLANTED_WANT.items():
        q[i] = desc[j]
    q[4] = desc[1]
    pts = [p for p, _ in PLANTED_POINTS]
    case = {"kpts": np.array(PLANTED_FEATURES, F32), "desc": np.ascontiguousarray(desc), "q": np.ascontiguousarray(q),
            "matched_in": np.array([0, 0, 0, 0, 0, 1, 0, 0], np.uint8),
            "pw": np.array([p[0] for p in pts], F32), "normal": np.array([p[1] for p in pts], F32), "min_dist": np.array([p[2] for p in pts], F32),
            "max_dist": np.array([p[3] for p in pts], F32), "scale_dist": np.array([p[3] for p in pts], F32), "valid": np.array([p[4] for p in pts], np.uint8)}
    return P, case


# ---------------------------------------------------------------- what both test files share: solved cases, the binding, the C++ driver
MODES = ((PROJ_INVZ, DIST_FLOAT), (PROJ_INVZ, DIST_TRUNC), (PROJ_DIV, DIST_FLOAT), (PROJ_DIV, DIST_TRUNC))
_cases, _cache = {}, {}


def main_case(nlevels=1):
    if nlevels not in _cases:
        _cases[nlevels] = make_case(0, nlevels=nlevels)
    return _cases[nlevels]


def solved(oracle, name, proj_mode=PROJ_INVZ, dist_mode=DIST_FLOAT, sequential=True):
    """(P, case, restatement result) of "main" (640 x 480, Nf = 1100, Np = 2600), "main8" (the same with nlevels = 8, scale factor 1.2) or
    "planted", computed once per session"""
    key = (name, proj_mode, dist_mode, sequential)
    if key not in _cache:
        P, c = planted_case() if name == "planted" else main_case(8 if name == "main8" else 1)
        P = dict(P, proj_mode=proj_mode)
        _cache[key] = (P, c, search(oracle, P, c, dist_mode, TH_LOW, sequential))
    return _cache[key]


def to_capi(P, dist_mode):
    from rover_slam_amd import capi
    return capi.sim3_params(P["quat"], P["t"], P["ow"], P["intrinsics"], P["bounds"], P["th"], P["scale_factors"], P["log_scale_factor"],
                            P["proj_mode"], dist_mode)


DRIVER_SCALE = F32(1.5)
RATIO_HAMMING = F32(0.75)          # TH_LOW * 0.75 = 0.9: the second overload accepts a truncated distance of 0 only


def write_driver_case(path, P, c, nleft=-1):
    """the main case as tests/cpp/sim3_search_driver.cpp reads it.  The Sim3 carries translation t * s and scale s, and the shim divides
    them again: the P returned holds that quotient and the camera centre the driver's SE3 stand-in derives from it.  An invalid map point
    is bad (even index) or already in vpMatched (odd index: it owns one of the pre-matched features); the other pre-matched features hold
    a map point that is not in vpPoints."""
    Np, Nf = len(c["pw"]), len(c["kpts"])
    big = (P["t"] * DRIVER_SCALE).astype(F32)
    t = (big / DRIVER_SCALE).astype(F32)
    Pd = dict(P, t=t, ow=inverse_translation(P["quat"], t))
    invalid = np.flatnonzero(c["valid"] == 0)
    pre = np.flatnonzero(c["matched_in"] != 0)
    found = invalid[invalid % 2 == 1][:len(pre)]
    bad = np.zeros((Np,), np.uint8); bad[invalid] = 1; bad[found] = 0
    prior = np.where(c["matched_in"] != 0, -2, -1).astype(np.int32)
    prior[pre[:len(found)]] = found
    assert len(found) > 10 and bad.sum() > 10 and (prior == -2).sum() > 10
    with open(path, "wb") as f:
        np.array([Np, Nf, nleft, P["th"], P["nlevels"]], np.int32).tofile(f)
        np.array([*P["quat"], *big, DRIVER_SCALE, *P["intrinsics"], *P["bounds"], P["log_scale_factor"], RATIO_HAMMING], np.float32).tofile(f)
        P["scale_factors"].astype(np.float32).tofile(f); bad.tofile(f); prior.tofile(f)
        for k in ("pw", "normal", "min_dist", "max_dist", "scale_dist", "q", "kpts", "desc"):
            c[k].astype(np.float32).tofile(f)
    return Pd, prior
