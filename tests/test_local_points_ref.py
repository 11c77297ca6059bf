"""CPU: the restatement of Tracking::SearchLocalPoints' steps 2 and 3 that the GPU tests compare against (tests/local_points_ref.py,
DESIGN.md 6f) is held to a scalar, per-point transcription of the reference text (src/Frame.cc:711-794, src/Matchers/SPmatcher.cc:1178-1283)
on np.float32 scalars and to a float64 evaluation of the projection; the generated cases meet the conditions that make them worth running;
the planted points land on the gates' edges; the binding refuses what it can refuse without a device."""
import ctypes

import numpy as np
import pytest

import local_points_ref as LP
import projection_search_ref as PS
import sim3_search_ref as S3
from local_points_ref import LEVEL_PREDICTED, LEVEL_ZERO, case_of, solved, to_capi

F32 = np.float32
CONFIGS = [("main", 1, True, LEVEL_ZERO), ("main", 6, False, LEVEL_ZERO), ("main", 6, True, LEVEL_PREDICTED), ("main8", 1, True, LEVEL_PREDICTED),
           ("main8", 6, True, LEVEL_ZERO), ("main8", 6, False, LEVEL_PREDICTED), ("planted", 1, True, LEVEL_ZERO), ("planted", 1, True, LEVEL_PREDICTED)]


# ---------------------------------------------------------------- the reference text, one map point at a time
class MP:
    """the tracking fields of a map point; None = never written"""
    def __init__(self):
        self.mbTrackInView = None
        self.mTrackProjX = self.mTrackProjY = self.mTrackProjXR = self.mTrackDepth = self.mnTrackScaleLevel = self.mTrackViewCos = None


def is_in_frustum(P, c, i, pMP):
    """Frame.cc:711-794 for map point i, statement by statement on np.float32 scalars; returns (true / false, the gate that said false)"""
    R, t, ow = P["rcw"], P["tcw"], P["ow"]
    fx, fy, cx, cy = P["intrinsics"]
    mnMinX, mnMinY, mnMaxX, mnMaxY = (F32(b) for b in P["bounds"])
    pMP.mbTrackInView = False                                                         # :711
    pMP.mTrackProjX = F32(-1)
    pMP.mTrackProjY = F32(-1)
    px, py, pz = c["pw"][i]                                                           # :717
    x = ((R[0, 0] * px + R[0, 1] * py) + R[0, 2] * pz) + t[0]                         # :721, in the contract's order
    y = ((R[1, 0] * px + R[1, 1] * py) + R[1, 2] * pz) + t[1]
    z = ((R[2, 0] * px + R[2, 1] * py) + R[2, 2] * pz) + t[2]
    Pc_dist = np.sqrt((x * x + y * y) + z * z)                                        # :722
    invz = F32(1.0) / z                                                               # :726
    if z < F32(0.0):                                                                  # :728
        return False, 2
    u, v = (fx * x) / z + cx, (fy * y) / z + cy                                       # :731, Pinhole::project
    if u < mnMinX or u > mnMaxX:                                                      # :735
        return False, 3
    if v < mnMinY or v > mnMaxY:                                                      # :737
        return False, 3
    pMP.mTrackProjX = u                                                               # :740
    pMP.mTrackProjY = v
    maxDistance = c["max_dist"][i]                                                    # :746
    minDistance = c["min_dist"][i]
    ox, oy, oz = px - ow[0], py - ow[1], pz - ow[2]                                   # :750
    dist = np.sqrt((ox * ox + oy * oy) + oz * oz)                                     # :752
    if dist < minDistance or dist > maxDistance:                                      # :755
        return False, 4
    nx, ny, nz = c["normal"][i]                                                       # :762
    viewCos = ((ox * nx + oy * ny) + oz * nz) / dist                                  # :765
    if viewCos < P["view_cos_limit"]:                                                 # :768
        return False, 5
    ratio = c["scale_dist"][i] / dist                                                 # :773, MapPoint.cc:721: the bare mfMaxDistance
    nScale = np.ceil(np.log(ratio) / P["log_scale_factor"])                           # MapPoint.cc:725
    nScale = 0 if not nScale > 0 else (P["nlevels"] - 1 if nScale >= P["nlevels"] else int(nScale))
    for s in (x, Pc_dist, invz, u, dist, viewCos, ratio):
        assert s.dtype == np.float32
    pMP.mbTrackInView = True                                                          # :778
    pMP.mTrackProjX = u
    pMP.mTrackProjXR = u - P["mbf"] * invz                                            # :782
    pMP.mTrackDepth = Pc_dist
    pMP.mTrackProjY = v
    pMP.mnTrackScaleLevel = nScale
    pMP.mTrackViewCos = viewCos
    return True, 0


def search_local_points(oracle, P, c):
    """Tracking.cc:4124-4147 and SPmatcher.cc:1178-1283 on the case: returns the map points, the reject code of each, nToMatch, the candidate
    lists, what every point saw at its turn, F.mvpMapPoints (index into the list, -1 NULL, -2 the map point a skipped feature held) and
    nmatches"""
    Np, Nf = len(c["pw"]), len(c["kpts"])
    mps = [MP() for _ in range(Np)]
    reject = np.zeros((Np,), np.int32)
    nToMatch = 0
    with np.errstate(all="ignore"):
        for i in range(Np):
            if not c["valid"][i]:                                                     # Tracking.cc:4129-4133
                reject[i] = 1
                continue
            inside, reject[i] = is_in_frustum(P, c, i, mps[i])
            if inside:
                nToMatch += 1                                                         # :4141
        # SearchByProjection1
        th = P["th"]
        bFactor = th != F32(1.0)                                                      # :1175
        grid = PS.build_grid(c["kpts"], P["bounds"])
        lists = []
        for i in range(Np):
            pMP = mps[i]
            lists.append([])
            if not pMP.mbTrackInView:                                                 # :1181 (an invalid point: Tracking.cc:4113 / :1187)
                continue
            if P["far_points"] and pMP.mTrackDepth > P["th_far"]:                     # :1184
                reject[i] = 6
                continue
            nPredictedLevel = pMP.mnTrackScaleLevel if P["level_mode"] == LEVEL_PREDICTED else 0          # :1193
            r = F32(2.5) if float(pMP.mTrackViewCos) > 0.998 else F32(4.0)            # :1197, RadiusByViewingCos: a double literal
            if bFactor:
                r = r * th                                                            # :1201
            lists[i] = PS.features_in_area(grid, c["kpts"], c["octave"], P["bounds"], pMP.mTrackProjX, pMP.mTrackProjY,
                                           r * P["scale_factors"][nPredictedLevel], nPredictedLevel)       # :1205
    dist = PS.candidate_distances(oracle, c["q"], c["desc"], lists)
    owner = [-2 if s else -1 for s in c["skip"]]                                      # F.mvpMapPoints: -2 holds Observations() > 0
    observations = lambda k: k == -2 or (k >= 0 and c["observed"][k])   # noqa: E731
    best = []
    nmatches = 0
    for i in range(Np):
        bestDist, bestDist2, bestIdx = F32(256), F32(256), -1                         # :1214-1218
        for idx, d in zip(lists[i], dist[i]):
            if owner[idx] != -1 and observations(owner[idx]):                         # :1227
                continue
            if d < bestDist:                                                          # :1239
                bestDist2, bestDist, bestIdx = bestDist, d, idx
            elif d < bestDist2:
                bestDist2 = d
        best.append((bestIdx, bestDist, bestDist2))
        if lists[i] and bestDist <= PS.TH_HIGH:                                       # :1210, :1257
            owner[bestIdx] = i
            nmatches += 1
    return mps, reject, nToMatch, lists, best, owner, nmatches


@pytest.mark.parametrize("name,th,far_points,level_mode", CONFIGS)
def test_restatement_equals_the_per_point_loop(oracle, name, th, far_points, level_mode):
    P, c, r = solved(oracle, name, th, far_points, level_mode)
    mps, reject, nToMatch, lists, best, owner, nmatches = search_local_points(oracle, P, c)
    assert np.array_equal(reject, r["reject"]) and nToMatch == r["in_frustum"] and nmatches == r["nmatches"]
    assert lists == r["lists"]
    assert np.array_equal(np.array([b[0] for b in best], np.int32), r["best_idx"])
    assert np.array_equal(np.array([b[1] for b in best], F32), r["best_dist"]) and np.array_equal(np.array([b[2] for b in best], F32), r["second_dist"])
    assert np.array_equal(np.array([k if k >= 0 else -1 for k in owner], np.int32), r["assign"])
    same = lambda a, b: a == b or (a != a and b != b)   # noqa: E731
    for i, m in enumerate(mps):
        code = reject[i]
        if code == 1:
            assert m.mbTrackInView is None and tuple(r["proj"][i]) == (0, 0)
        else:
            assert m.mbTrackInView == (code in (0, 6)), i
            assert same(m.mTrackProjX, r["proj"][i, 0]) and same(m.mTrackProjY, r["proj"][i, 1]), i
            assert (m.mTrackProjX == -1 and m.mTrackProjY == -1) == (code in (2, 3)) or code in (0, 6), i
        if code in (0, 6):
            assert same(m.mTrackProjXR, r["proj_xr"][i]) and same(m.mTrackDepth, r["depth"][i]) and same(m.mTrackViewCos, r["view_cos"][i]), i
            assert m.mnTrackScaleLevel == r["level"][i], i
        else:
            assert m.mTrackDepth is None and r["proj_xr"][i] == 0 and r["depth"][i] == 0 and r["view_cos"][i] == 0 and r["level"][i] == -1, i
        assert (r["radius"][i] > 0) == (code == 0) or r["radius"][i] != r["radius"][i], i
    fields = LP.map_point_fields(r, {k: np.zeros(len(mps), bool if k == "in_view" else (np.int32 if k in ("level", "visible") else F32)) for k in LP.FIELDS})
    assert fields["visible"].sum() == nToMatch and np.array_equal(fields["in_view"], np.array([bool(m.mbTrackInView) for m in mps]))


@pytest.mark.parametrize("name", ("main", "main8"))
def test_projection_is_close_to_float64(oracle, name):
    P, c, r = solved(oracle, name, 1, True, LEVEL_ZERO)
    pc = c["pw"].astype(np.float64) @ P["rcw"].astype(np.float64).T + P["tcw"].astype(np.float64)
    fx, fy, cx, cy = (float(v) for v in P["intrinsics"])
    past = (r["reject"] == 0) | (r["reject"] >= 4)
    u, v = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
    err = np.maximum(np.abs(r["proj"][:, 0] - u), np.abs(r["proj"][:, 1] - v))[past]
    seen = (r["reject"] == 0) | (r["reject"] == 6)
    derr = np.abs(r["depth"] - np.sqrt((pc * pc).sum(1)))[seen]
    print(f"{name}: projection error against float64 at most {err.max():.2e} px over {past.sum()} points, depth {derr.max():.2e}")
    assert past.sum() > 1500 and err.max() < 1e-3 and derr.max() < 1e-4


# ---------------------------------------------------------------- the generated cases meet their conditions
def test_main_case_is_not_vacuous(oracle):
    Np = 2600
    for th in (1, 6):
        P, c, r = solved(oracle, "main", th, True, LEVEL_ZERO)
        codes = np.bincount(r["reject"], minlength=7)
        searched = r["reject"] == 0
        radii = {float(v): int(n) for v, n in zip(*np.unique(r["radius"][searched], return_counts=True))}
        _, _, static = solved(oracle, "main", th, True, LEVEL_ZERO, sequential=False)
        seq_differs = int((static["best_idx"] != r["best_idx"])[searched].sum())
        overwritten = r["nmatches"] - int((r["assign"] >= 0).sum())
        print(f"main, th {th}: reject codes {[int(n) for n in codes]}, radii {radii}, sequence changes {seq_differs} of {int(searched.sum())}, "
              f"candidates {r['candidates']}, nmatches {r['nmatches']} ({overwritten} overwritten), moved {c['moved']}")
        assert len(c["pw"]) == Np and (codes >= 50).all(), codes
        assert set(radii) == {2.5 * th, 4.0 * th} and min(radii.values()) >= 50
        assert seq_differs >= 100
        assert overwritten >= 1                                       # an unobserved accepted point was overwritten
        assert r["in_frustum"] == codes[0] + codes[6] and r["searched"] == codes[0]
        # past two trips of the 1024-stride loops, with results in the third
        assert Np > 2048 and Np % 256 != 0 and (r["best_dist"][2048:] <= PS.TH_HIGH).any() and (np.flatnonzero(r["assign"] >= 0) >= 1024).any()
    assert c["moved"] <= 0.02 * Np
    assert (c["kpts"] * 4 == np.round(c["kpts"] * 4)).all() and (c["kpts"] != np.round(c["kpts"])).any()      # quarter pixels
    assert 0.1 < c["skip"].mean() < 0.2 and 0.05 < 1 - c["observed"].mean() < 0.15
    _, _, off = solved(oracle, "main", 1, False, LEVEL_ZERO)
    assert (off["reject"] == 6).sum() == 0 and off["searched"] == off["in_frustum"] == r["in_frustum"]
    # one level: the level mode changes nothing
    _, _, pred = solved(oracle, "main", 6, True, LEVEL_PREDICTED)
    for k in LP.KEYS:
        assert np.array_equal(pred[k], r[k]), k


def test_eight_level_case_is_not_vacuous(oracle):
    P, c, zero = solved(oracle, "main8", 6, True, LEVEL_ZERO)
    _, _, pred = solved(oracle, "main8", 6, True, LEVEL_PREDICTED)
    seen = (zero["reject"] == 0) | (zero["reject"] == 6)
    assert set(np.unique(zero["level"][seen])) == set(range(8)) and np.array_equal(zero["level"], pred["level"])
    assert set(np.unique(c["octave"])) == set(range(8))
    steps = S3.level_steps(P, c["pw"], c["scale_dist"])
    assert (np.abs(steps - np.round(steps)) >= LP.STEP_MARGIN).all() and c["moved"] <= 0.02 * len(c["pw"])
    assert not np.array_equal(c["max_dist"], c["scale_dist"])                      # the gate's distance is not PredictScale's
    lists_differ = sum(a != b for a, b in zip(zero["lists"], pred["lists"]))
    searched = zero["reject"] == 0
    print(f"main8: levels {np.bincount(zero['level'][seen]).tolist()}, RFE_LEVEL_PREDICTED changes {lists_differ} candidate lists, nmatches "
          f"{zero['nmatches']} / {pred['nmatches']}, radii {len(np.unique(pred['radius'][searched]))}")
    assert lists_differ >= 100 and len(np.unique(pred["radius"][searched])) == 16 and len(np.unique(zero["radius"][searched])) == 2
    assert zero["nmatches"] > 20 and pred["nmatches"] > 20 and not np.array_equal(zero["assign"], pred["assign"])


def test_planted_points_sit_on_the_edges(oracle):
    P, c, r = solved(oracle, "planted", 1, True, LEVEL_ZERO)
    assert len(c["pw"]) == 24
    assert list(r["reject"]) == [code for _, code in LP.PLANTED_POINTS]
    assert list(r["assign"]) == list(LP.PLANTED_ASSIGN) and r["nmatches"] == LP.PLANTED_NMATCHES
    nxt = lambda v: np.nextafter(F32(v), F32(np.inf))   # noqa: E731
    assert tuple(r["proj"][0]) == (640.0, 240.0) and tuple(r["proj"][2]) == (0.0, 240.0) and tuple(r["proj"][22]) == (320.0, 480.0)
    assert tuple(r["proj"][23]) == (320.0, 0.0)
    front = LP.front(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], np.ones(24, np.uint8))
    assert tuple(r["proj"][1]) == (-1, -1) and c["pw"][1, 0] == F32(5) + F32(2.0 ** -20)
    with np.errstate(all="ignore"):
        assert (F32(256) * c["pw"][1, 0]) / F32(4) + F32(320) == nxt(640)                 # one ulp above max_x
    assert tuple(r["proj"][3]) == (-1, -1) and tuple(r["proj"][4]) == (-1, -1) and tuple(r["proj"][5]) == (-1, -1)
    assert np.signbit(c["pw"][4, 2]) and c["pw"][4, 2] == 0
    # the NaN point: searched, nothing found, and every field it derives is NaN
    assert np.isnan(r["proj"][6]).all() and r["radius"][6] == 4.0          # 0 * NaN: the rotation spreads it to every coordinate
    assert r["lists"][6] == [] and r["best_idx"][6] == -1
    assert np.isnan(r["depth"][6]) and np.isnan(r["view_cos"][6]) and r["level"][6] == 0
    assert c["min_dist"][7] == 4 and c["min_dist"][8] == nxt(4) and c["max_dist"][9] == 5 and nxt(c["max_dist"][10]) == 5
    assert tuple(r["proj"][8]) == (320.0, 240.0) and tuple(r["proj"][10]) == (512.0, 240.0)   # :740-741 ran before the distance gate
    assert r["view_cos"][11] == 0.5 and nxt(c["normal"][12, 2]) == 0.5 and tuple(r["proj"][12]) == (320.0, 240.0) and r["view_cos"][12] == 0
    # the radius threshold: fl32(0.998) is above the double literal, its lower neighbour below
    assert r["view_cos"][13] == LP.VIEWCOS_NEAR and nxt(r["view_cos"][14]) == LP.VIEWCOS_NEAR
    assert float(r["view_cos"][13]) > 0.998 > float(r["view_cos"][14]) and not r["view_cos"][13] > F32(0.998)
    assert r["radius"][13] == 2.5 and r["radius"][14] == 4.0 and r["best_idx"][13] == -1 and r["best_idx"][14] == 0 and r["lists"][14] == [0]
    assert r["depth"][15] == 8 and r["depth"][16] == nxt(8) and r["reject"][16] == 6 and r["level"][16] == 0 and r["radius"][16] == 0
    assert r["proj_xr"][15] == 320 - 64 / 8 and r["proj_xr"][0] == 640 - 16
    # the invalid point 17 would have taken feature 2, leaving the near copy to point 18
    v = LP.search(oracle, P, c, valid=np.ones(24, np.uint8))
    assert front["reject"][17] == 0 and v["assign"][2] == 17 and v["assign"][3] == 18 and v["nmatches"] == LP.PLANTED_NMATCHES + 1
    # point 19 has no observations: point 20 overwrites it; with observations it would block feature 4
    assert r["best_idx"][19] == 4 and r["best_idx"][20] == 4 and r["best_idx"][21] == 5 and r["best_dist"][19] == 0
    ob = LP.search(oracle, P, dict(c, observed=np.ones(24, np.uint8)))
    assert ob["assign"][4] == 19 and ob["assign"][5] == 20 and ob["best_idx"][21] == -1
    assert r["lists"][23] == [6] and r["best_idx"][23] == -1                              # the skipped feature is listed, never taken
    codes = [code for _, code in LP.PLANTED_POINTS]
    assert r["in_frustum"] == codes.count(0) + 1 == 16 and r["searched"] == codes.count(0) == 15
    off = LP.search(oracle, LP.P(case_of("planted")[0], 1, False), c)
    assert off["reject"][16] == 0 and off["searched"] == 16


# ---------------------------------------------------------------- the binding
def test_capi_binding_without_a_device():
    from rover_slam_amd import capi
    assert ctypes.sizeof(capi.FrustumParams) == 4 * (9 + 3 + 3 + 5 + 4 + 2 + 2 + 2 + capi.MAX_LEVELS + 1)
    assert {"rfe_search_local_points", "rfe_search_local_points_dev"} <= set(capi.EXPORTS)
    assert (capi.LEVEL_ZERO, capi.LEVEL_PREDICTED) == (LEVEL_ZERO, LEVEL_PREDICTED)
    base, _ = case_of("planted")
    p = to_capi(LP.P(base, 6, True, LEVEL_PREDICTED))
    assert list(p.rcw) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and p.th == 6 and p.nlevels == 1 and p.level_mode == 1 and p.fx == 256 and p.max_x == 640
    assert p.far_points == 1 and p.th_far == 8 and p.mbf == 64 and p.view_cos_limit == 0.5
    z = np.zeros((256,), np.float32).ctypes.data
    lib = capi.lib                                                 # a NULL ctx is refused before anything else is looked at
    assert lib.rfe_search_local_points(None, ctypes.byref(p), z, z, z, z, z, z, None, None, 1, z, z, None, None, None, 1, 1.4, z, *([None] * 10)) == -1
    assert lib.rfe_search_local_points_dev(None, ctypes.byref(p), z, z, z, z, z, z, None, None, 1, z, z, None, None, None, 1, None, 1.4, 16, z,
                                           *([None] * 9), z) == -1


# ---------------------------------------------------------------- the drop-in driver's case
def test_driver_case_round_trip(tmp_path, oracle):
    """the file the C++ driver reads keeps the problem: validity survives the translation into isBad() / mnLastFrameSeen, skip into the map
    point a feature holds"""
    P, c, r = solved(oracle, "planted", 1, True, LEVEL_ZERO)
    before, prior = LP.write_driver_case(str(tmp_path / "case.bin"), P, c)
    Np, Nf = len(c["pw"]), len(c["kpts"])
    assert np.array_equal(prior == -2, c["skip"] != 0) and (prior == -3).any()
    after = LP.map_point_fields(r, before)
    invalid = c["valid"] == 0
    for k in LP.FIELDS:
        assert np.array_equal(after[k][invalid], before[k][invalid]), k
    assert after["in_view"][16] and not after["in_view"][12] and after["proj_x"][12] == 320 and after["depth"][12] == before["depth"][12]
    assert (after["visible"] - before["visible"]).sum() == r["in_frustum"]
    import os
    size = 6 * 4 + 27 * 4 + 4 * P["nlevels"] + Np * (1 + 4 + 1 + 1 + 7 * 4) + Nf * 8 + 4 * Np * (3 + 3 + 1 + 1 + 1 + 256) + 4 * Nf * 258
    assert os.path.getsize(str(tmp_path / "case.bin")) == size
