"""numpy restatement of the left-camera branch of SPmatcher::SearchByProjection1 (reference src/Matchers/SPmatcher.cc:1190-1283) with
Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (src/Frame.cc:488-523, 998-1014, 895-987), the contract of DESIGN.md 6d.
fp32 throughout, in the order the reference writes it; the descriptor distances are the oracle's (oracle.search_candidates, pinned bit
for bit to the reference recording by tests/golden/ref_distance.npz).  Shared by test_projection_search_ref.py (CPU) and
test_gpu_projection_search.py."""
import numpy as np

COLS, ROWS = 32, 24            # FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:49-50
TH_HIGH = np.float32(1.4)      # SPmatcher::TH_HIGH
F32 = np.float32


def round_half_away(v):
    """C's roundf on an fp32 value (NOT numpy's half-to-even round)."""
    v = F32(v)
    t = np.trunc(v)
    return F32(t + np.sign(v)) if abs(F32(v - t)) >= F32(0.5) else F32(t)      # v - trunc(v) is exact in fp32


def _inv(bounds):
    min_x, min_y, max_x, max_y = (F32(b) for b in bounds)
    return min_x, min_y, F32(COLS) / F32(max_x - min_x), F32(ROWS) / F32(max_y - min_y)


def cells(kpts, bounds):
    """PosInGrid of every feature: [Nf,2] int (cell x, cell y), (-1, -1) for a feature outside the grid."""
    min_x, min_y, inv_w, inv_h = _inv(bounds)
    k = np.asarray(kpts, F32).reshape(-1, 2)
    out = np.full((k.shape[0], 2), -1, np.int64)
    for i in range(k.shape[0]):
        gx = round_half_away(F32(k[i, 0] - min_x) * inv_w)
        gy = round_half_away(F32(k[i, 1] - min_y) * inv_h)
        if 0 <= gx < COLS and 0 <= gy < ROWS:
            out[i] = (int(gx), int(gy))
    return out


def build_grid(kpts, bounds):
    """mGrid[ix][iy]: feature indices in ascending order (AssignFeaturesToGrid pushes them in index order)."""
    grid = [[[] for _ in range(ROWS)] for _ in range(COLS)]
    for i, (cx, cy) in enumerate(cells(kpts, bounds)):
        if cx >= 0:
            grid[cx][cy].append(i)
    return grid


def features_in_area(grid, kpts, octave, bounds, px, py, r, level):
    """GetFeaturesInArea(px, py, r, level - 1, level) -> feature indices in the reference's visiting order."""
    min_x, min_y, inv_w, inv_h = _inv(bounds)
    px, py, r = F32(px), F32(py), F32(r)
    if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(r)):
        return []
    with np.errstate(over="ignore", invalid="ignore"):
        lo_x = np.floor(F32(F32(px - min_x) - r) * inv_w); hi_x = np.ceil(F32(F32(px - min_x) + r) * inv_w)
        lo_y = np.floor(F32(F32(py - min_y) - r) * inv_h); hi_y = np.ceil(F32(F32(py - min_y) + r) * inv_h)
    if not (lo_x < COLS) or not (hi_x >= 0) or not (lo_y < ROWS) or not (hi_y >= 0):
        return []
    x0, x1 = int(lo_x) if lo_x > 0 else 0, int(hi_x) if hi_x < COLS - 1 else COLS - 1        # max(0, .), min(31, .): clamped as floats
    y0, y1 = int(lo_y) if lo_y > 0 else 0, int(hi_y) if hi_y < ROWS - 1 else ROWS - 1
    k = np.asarray(kpts, F32).reshape(-1, 2)
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for j in grid[ix][iy]:
                o = 0 if octave is None else int(octave[j])
                if o < level - 1 or o > level:
                    continue
                if abs(F32(k[j, 0] - px)) < r and abs(F32(k[j, 1] - py)) < r:
                    out.append(j)
    return out


def candidate_lists(kpts, octave, bounds, proj, radius, pred_level=None):
    grid = build_grid(kpts, bounds)
    proj = np.asarray(proj, F32).reshape(-1, 2)
    return [features_in_area(grid, kpts, octave, bounds, proj[i, 0], proj[i, 1], radius[i], 0 if pred_level is None else int(pred_level[i]))
            for i in range(proj.shape[0])]


def to_csr(lists):
    off = np.zeros((len(lists) + 1,), np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    cand = np.array([j for l in lists for j in l], np.int32)
    return off, cand


def _out(Nq, Nf):
    return {"assign": np.full((Nf,), -1, np.int32), "best_idx": np.full((Nq,), -1, np.int32),
            "best_dist": np.full((Nq,), 256, np.float32), "second_dist": np.full((Nq,), 256, np.float32), "nmatches": 0}


def search_by_projection_seq(oracle, q, f, lists, skip=None, observed=None, th_high=TH_HIGH):
    """the reference's loop, map point by map point: each one is scanned by the oracle with the blocked array as it stands at its turn"""
    q = np.ascontiguousarray(q, F32).reshape(-1, 256); f = np.ascontiguousarray(f, F32).reshape(-1, 256)
    Nq, Nf = q.shape[0], f.shape[0]
    out = _out(Nq, Nf)
    blocked = np.zeros((max(Nf, 1),), np.uint8) if skip is None else np.array(skip, np.uint8).copy()
    for i in range(Nq):
        if not lists[i]:
            continue
        bi, bd, sd = oracle.search_candidates(q[i:i + 1], f, np.array([0, len(lists[i])], np.int32), np.array(lists[i], np.int32), blocked)
        out["best_idx"][i], out["best_dist"][i], out["second_dist"][i] = bi[0], bd[0], sd[0]
        if bd[0] <= F32(th_high):
            out["assign"][bi[0]] = i                       # F.mvpMapPoints[bestIdx] = pMP: a later writer overwrites
            out["nmatches"] += 1
            if observed is None or observed[i]:
                blocked[bi[0]] = 1                          # :1227-1229 for every later map point
    return out


def candidate_distances(oracle, q, f, lists):
    """DescriptorDistance_sp of every (map point, candidate), per list: the oracle scan of one-candidate lists returns the distance itself"""
    q = np.ascontiguousarray(q, F32).reshape(-1, 256); f = np.ascontiguousarray(f, F32).reshape(-1, 256)
    off, cand = to_csr(lists)
    if cand.size == 0:
        return [np.zeros((0,), F32) for _ in lists]
    rows = np.repeat(np.arange(len(lists)), np.diff(off))
    _, bd, _ = oracle.search_candidates(q[rows], f, np.arange(cand.size + 1, dtype=np.int32), cand)
    assert (bd < 256).all()
    return [bd[off[i]:off[i + 1]] for i in range(len(lists))]


def _scan(cl, dl, blocked_for):
    bi, bd, sd = -1, F32(256), F32(256)
    for j, d in zip(cl, dl):
        if blocked_for(j):
            continue
        if d < bd:
            sd, bd, bi = bd, d, j
        elif d < sd:
            sd = d
    return bi, bd, sd


def search_by_projection_jacobi(oracle, q, f, lists, skip=None, observed=None, th_high=TH_HIGH):
    """The parallel form: in every round EVERY map point rescans its list against the accepted picks of the round before (feature j is
    blocked for map point i when skip[j], or when the least observed map point accepted on j is < i); the first round that changes no
    accepted pick ends it.  Map point 0 is right after round 1, map point i after round i + 1.  Returns (outputs, rounds)."""
    Nq, Nf = len(lists), np.asarray(f).reshape(-1, 256).shape[0]
    dist = candidate_distances(oracle, q, f, lists)
    sk = np.zeros((max(Nf, 1),), bool) if skip is None else np.asarray(skip).astype(bool)
    ob = np.ones((Nq,), bool) if observed is None else np.asarray(observed).astype(bool)
    big = np.iinfo(np.int64).max
    minw = np.full((max(Nf, 1),), big, np.int64)
    pick = np.full((Nq,), -1, np.int64)
    res = [None] * Nq
    rounds = 0
    while True:
        new = np.full((Nq,), -1, np.int64)
        for i in range(Nq):
            res[i] = _scan(lists[i], dist[i], lambda j: sk[j] or minw[j] < i)
            if res[i][1] <= F32(th_high):
                new[i] = res[i][0]
        rounds += 1
        same = np.array_equal(new, pick)
        pick = new
        if same:
            break
        minw[:] = big
        for i in range(Nq):
            if pick[i] >= 0 and ob[i]:
                minw[pick[i]] = min(minw[pick[i]], i)
    out = _out(Nq, Nf)
    for i in range(Nq):
        out["best_idx"][i], out["best_dist"][i], out["second_dist"][i] = res[i]
        if pick[i] >= 0:
            out["assign"][pick[i]] = i                     # ascending i: the last accepted writer stays
            out["nmatches"] += 1
    return out, rounds


def static_scan(oracle, q, f, lists, skip=None):
    """what one bulk rfe_search_candidates call with the static skip array gives every map point"""
    off, cand = to_csr(lists)
    return oracle.search_candidates(np.ascontiguousarray(q, F32), np.ascontiguousarray(f, F32), off, cand, skip)


def make_case(seed, W=160, H=120, Nf=300, Nq=400, ncent=40, th=3, src_hi=None):
    """The contention case: clustered descriptors, about 2.7 map points per source feature (src_hi=None: the sources are the first half of
    the features), an exact-tie pair (features 3 and 7)."""
    rng = np.random.default_rng(seed)
    kxy = np.stack([rng.integers(0, W, Nf), rng.integers(0, H, Nf)], 1).astype(np.int32)
    kxy[3] = (min(int(kxy[3, 0]), W - 12), min(int(kxy[3, 1]), H - 12))   # the tie pair stays inside the grid (x >= W - 2.5 is column 32)
    kxy[7] = (kxy[3, 0] + 1, kxy[3, 1])
    centre = rng.standard_normal((ncent, 256)).astype(F32)
    cluster = (kxy[:, 0] // 32 + 5 * (kxy[:, 1] // 30)) % ncent
    desc = centre[cluster] + F32(0.03) * rng.standard_normal((Nf, 256)).astype(F32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    desc[7] = desc[3]
    src = rng.integers(0, Nf // 2 if src_hi is None else src_hi, Nq)
    src[Nq // 2] = 3                                             # somebody wants the tie pair, whatever the draw
    q = (desc[src] + F32(0.02) * rng.standard_normal((Nq, 256)).astype(F32)).astype(F32)
    proj = (kxy[src].astype(F32) + rng.uniform(-3, 3, (Nq, 2)).astype(F32)).astype(F32)
    radius = np.where(rng.random(Nq) < 0.5, F32(2.5), F32(4.0)).astype(F32) * F32(th)
    skip = (rng.random(Nf) < 0.2).astype(np.uint8)
    observed = (rng.random(Nq) < 0.9).astype(np.uint8)
    return {"W": W, "H": H, "bounds": (0.0, 0.0, float(W), float(H)), "kxy": kxy, "kpts": kxy.astype(F32), "desc": np.ascontiguousarray(desc),
            "q": np.ascontiguousarray(q), "proj": np.ascontiguousarray(proj), "radius": radius, "skip": skip, "observed": observed, "src": src}


PLANTED_OUT = ((-20.0, 100.0), (100.0, -15.0))                              # scaled coordinate -0.5: roundf gives -1, outside the grid
PLANTED_IN = ((-19.75, 100.0), (100.0, -14.75), (-19.75, -14.75))           # scaled coordinate -0.4875: cell 0
PLANTED = (PLANTED_OUT[0], PLANTED_IN[0], PLANTED_OUT[1], PLANTED_IN[1], PLANTED_IN[2])      # the last five features, in this order
PLANTED_PROJ = ((-12.0, 100.0), (100.0, -8.0), (-12.0, -8.0))               # the last three map points, radius 12


def off_origin(c, seed):
    """A 640 x 480 case of make_case moved to the bounds (-10, -5, 630, 475) of an undistorted image, with sub-pixel positions.  The cells
    are 20 pixels wide and high and fl32(0.05) * 10 k is an exact half for odd k, so a feature at a whole pixel 10 k from the origin sits
    on a rounding tie, where roundf (half away from zero) and round-half-to-even part.  Every position gets a fraction from {0, .25, .5,
    .75} (exact in fp32; the tie pair keeps 0), the last five features are PLANTED on the negative side, and the last three map points
    look at them.  Float positions only: no kxy."""
    assert c["bounds"] == (0.0, 0.0, 640.0, 480.0)
    rng = np.random.default_rng(seed)
    shift = np.array([-10.0, -5.0], F32)
    frac = (rng.integers(0, 4, c["kxy"].shape) * 0.25).astype(F32)
    frac[3] = frac[7] = 0
    kpts = (c["kxy"].astype(F32) + shift + frac).astype(F32)
    kpts[-5:] = np.array(PLANTED, F32)
    proj = (c["proj"] + shift).astype(F32)
    proj[-3:] = np.array(PLANTED_PROJ, F32)
    radius = c["radius"].copy()
    radius[-3:] = F32(12.0)
    out = {k: v for k, v in c.items() if k != "kxy"}
    out.update(bounds=(-10.0, -5.0, 630.0, 475.0), kpts=np.ascontiguousarray(kpts), proj=np.ascontiguousarray(proj), radius=radius)
    return out


def on_half(kpts, bounds):
    """[Nf] bool: the scaled x or y coordinate of the feature is exactly k + 0.5 (a rounding tie in PosInGrid)"""
    min_x, min_y, inv_w, inv_h = _inv(bounds)
    k = np.asarray(kpts, F32).reshape(-1, 2)
    sx = ((k[:, 0] - min_x).astype(F32) * inv_w).astype(F32); sy = ((k[:, 1] - min_y).astype(F32) * inv_h).astype(F32)
    return (np.abs(sx - np.trunc(sx)) == F32(0.5)) | (np.abs(sy - np.trunc(sy)) == F32(0.5))


def case_lists(c, octave=None, pred_level=None):
    return candidate_lists(c["kpts"], octave, c["bounds"], c["proj"], c["radius"], pred_level)


def vacuity(oracle, c, lists, seq, rounds):
    """the figures that show the case exercises the sequence (asserted by both test files)"""
    sbi, _, _ = static_scan(oracle, c["q"], c["desc"], lists, c["skip"])
    accepted = seq["best_dist"] <= TH_HIGH
    writers = np.bincount(seq["best_idx"][accepted], minlength=len(c["kpts"]))
    cell = cells(c["kpts"], c["bounds"])
    return {"differ": int((sbi != seq["best_idx"]).sum()), "outside": int((cell[:, 0] < 0).sum()), "multi": int((writers > 1).sum()),
            "rounds": rounds, "tie": any(3 in l and 7 in l for l in lists), "mean_cand": float(np.mean([len(l) for l in lists])),
            "max_cand": max(len(l) for l in lists)}


def check_vacuity(v, Nq):
    assert v["differ"] >= Nq // 4, v
    assert v["outside"] >= 1 and v["multi"] >= 1 and v["rounds"] >= 3 and v["tie"], v
