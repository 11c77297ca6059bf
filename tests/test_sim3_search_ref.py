"""CPU: the restatement of the two Sim3 SearchByProjection overloads that the GPU tests compare against (tests/sim3_search_ref.py,
DESIGN.md 6e) holds its own definitions -- the vectorised front against a plain per-point loop of the reference text, the truncated scan
against the loop with `int dist` -- the main case is not vacuous, the planted points land on the gates' edges, and the binding refuses what
it can refuse without a device."""
import ctypes
import os

import numpy as np
import pytest

import projection_search_ref as PS
import sim3_search_ref as S3
from sim3_search_ref import MODES, main_case, solved, to_capi, write_driver_case

F32 = np.float32
# ---------------------------------------------------------------- the front against the reference text, one map point at a time
def front_of_one_point(P, c, i):
    """SPmatcher.cc:1578-1625 / :2096-2139 for map point i, statement by statement on np.float32 scalars"""
    if c.get("valid") is not None and not c["valid"][i]:
        return 1, None
    qx, qy, qz, qw = P["quat"]; t, ow = P["t"], P["ow"]
    fx, fy, cx, cy = P["intrinsics"]
    min_x, min_y, max_x, max_y = (F32(b) for b in P["bounds"])
    px, py, pz = c["pw"][i]
    ax, ay, az = qy * pz - qz * py, qz * px - qx * pz, qx * py - qy * px               # uv = q.vec().cross(p)
    ax, ay, az = ax + ax, ay + ay, az + az                                              # uv += uv
    wx, wy, wz = qy * az - qz * ay, qz * ax - qx * az, qx * ay - qy * ax               # q.vec().cross(uv)
    x, y, z = ((px + qw * ax) + wx) + t[0], ((py + qw * ay) + wy) + t[1], ((pz + qw * az) + wz) + t[2]
    if z < 0:
        return 2, None
    if P["proj_mode"] == S3.PROJ_INVZ:
        invz = F32(1) / z
        u, v = fx * (x * invz) + cx, fy * (y * invz) + cy
    else:
        u, v = fx * x / z + cx, fy * y / z + cy
    if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
        return 3, None
    ox, oy, oz = px - ow[0], py - ow[1], pz - ow[2]
    dist = np.sqrt((ox * ox + oy * oy) + oz * oz)
    if dist < c["min_dist"][i] or dist > c["max_dist"][i]:
        return 4, None
    nx, ny, nz = c["normal"][i]
    if (ox * nx + oy * ny) + oz * nz < F32(0.5) * dist:
        return 5, None
    ratio = c["scale_dist"][i] / dist                        # MapPoint::PredictScale: mfMaxDistance / currentDist, not the gate's 1.2f * mfMaxDistance
    n = np.ceil(np.log(ratio) / P["log_scale_factor"])
    level = 0 if not n > 0 else (P["nlevels"] - 1 if n >= P["nlevels"] else int(n))
    for s in (x, u, dist, ratio):
        assert s.dtype == np.float32
    return 0, (u, v, F32(P["th"]) * P["scale_factors"][level], level)


@pytest.mark.parametrize("name", ("main", "main8", "planted"))
@pytest.mark.parametrize("proj_mode", (S3.PROJ_INVZ, S3.PROJ_DIV))
def test_front_equals_the_per_point_loop(name, proj_mode):
    P, c = S3.planted_case() if name == "planted" else main_case(8 if name == "main8" else 1)
    P = dict(P, proj_mode=proj_mode)
    got = S3.project(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["valid"])
    with np.errstate(all="ignore"):
        for i in range(len(c["pw"])):
            rej, r = front_of_one_point(P, c, i)
            assert got["reject"][i] == rej, i
            if rej:
                assert got["radius"][i] == 0 and got["level"][i] == -1 and (got["proj"][i] == 0).all(), i
            else:
                assert (got["proj"][i, 0], got["proj"][i, 1], got["radius"][i], got["level"][i]) == r, i


def test_inverse_translation_is_the_camera_centre():
    quat, t = S3.pose()
    ow = S3.inverse_translation(quat, t)
    back = S3.rotate(quat, ow.reshape(1, 3))[0] + t                                   # Tcw * Ow = 0
    assert np.abs(back).max() < 1e-6
    assert abs(float((quat.astype(np.float64) ** 2).sum()) - 1) < 1e-6 and abs(2 * np.arccos(float(quat[3])) - 0.3) < 1e-6


# ---------------------------------------------------------------- the scans against the loops as the reference writes them
def loop_of_the_reference(oracle, P, c, front, lists, truncated, th_accept):
    """:1635-1664 (float bestDist) / :2149-2177 (int dist, int bestDist) over the candidate lists, vpMatched as the loop leaves it"""
    dist = PS.candidate_distances(oracle, c["q"], c["desc"], lists)
    taken = [bool(m) for m in c["matched_in"]]
    matched = [-1] * len(taken)
    best = []
    nmatches = 0
    for i, (cl, dl) in enumerate(zip(lists, dist)):
        best_dist, best_idx = (256 if truncated else F32(256)), -1
        for idx, d in zip(cl, dl):
            if taken[idx]:
                continue
            d = int(d) if truncated else d                        # const int dist = DescriptorDistance_sp(dMP, dKF);
            if d < best_dist:
                best_dist, best_idx = d, idx
        best.append(best_idx)
        if cl and F32(best_dist) <= F32(th_accept):
            taken[best_idx] = True; matched[best_idx] = i; nmatches += 1
    return np.array(matched, np.int32), np.array(best, np.int32), nmatches


@pytest.mark.parametrize("name", ("main", "main8"))
@pytest.mark.parametrize("dist_mode", (S3.DIST_FLOAT, S3.DIST_TRUNC))
def test_scan_equals_the_loop_of_the_reference(oracle, name, dist_mode):
    P, c, r = solved(oracle, name, S3.PROJ_INVZ, dist_mode)
    matched, best, n = loop_of_the_reference(oracle, P, c, r, r["lists"], dist_mode == S3.DIST_TRUNC, S3.TH_LOW)
    assert np.array_equal(matched, r["matched"]) and np.array_equal(best, r["best_idx"]) and n == r["nmatches"] > 100
    assert (r["matched"][c["matched_in"] != 0] == -1).all()                          # a pre-matched feature stays -1
    if dist_mode == S3.DIST_TRUNC:
        seen = r["best_idx"] >= 0
        assert np.array_equal(r["best_dist"][seen], np.trunc(r["best_dist"][seen])) and set(np.unique(r["best_dist"][seen])) <= {0.0, 1.0}
        assert (r["best_dist"][seen] == 1).any()                                      # 1 <= TH_LOW: the int comparison accepts those too


# ---------------------------------------------------------------- the main case exercises what it is there for
@pytest.mark.parametrize("name", ("main", "main8"))
def test_main_case_is_not_vacuous(oracle, name):
    P, c, r = solved(oracle, name)
    Np = len(c["pw"])
    codes = np.bincount(r["reject"], minlength=6)
    searched = r["reject"] == 0
    ns = int(searched.sum())
    _, _, static = solved(oracle, name, sequential=False)
    _, _, trunc = solved(oracle, name, dist_mode=S3.DIST_TRUNC)
    Pd = dict(P, proj_mode=S3.PROJ_DIV)
    div = S3.project(Pd, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["valid"])
    seq_differs = int((static["best_idx"] != r["best_idx"])[searched].sum())
    trunc_differs = int((trunc["best_idx"] != r["best_idx"])[searched].sum())
    proj_differs = int((div["proj"] != r["proj"]).any(1)[searched].sum())
    print(f"{name}: reject codes {[int(n) for n in codes]}, sequence changes {seq_differs} of {ns}, TRUNC changes {trunc_differs}, projection forms differ "
          f"in {proj_differs}, moved {c['moved']}, candidates {r['candidates']}, nmatches {r['nmatches']} / {trunc['nmatches']}")
    assert (codes[1:] >= 100).all() and ns >= 800
    assert seq_differs >= 0.2 * ns and trunc_differs >= 0.1 * ns and proj_differs >= 0.2 * ns
    assert c["moved"] <= 0.02 * Np
    assert np.array_equal(div["reject"], r["reject"])
    # past two trips of the 1024-stride loops, with results in the third
    assert Np > 2048 and Np % 256 != 0 and (r["best_dist"][2048:] <= S3.TH_LOW).any() and (np.flatnonzero(r["matched"] >= 0) >= 1024).any()
    assert (c["kpts"] * 4 == np.round(c["kpts"] * 4)).all() and (c["kpts"] != np.round(c["kpts"])).any()      # quarter pixels
    assert 0.1 < c["matched_in"].mean() < 0.2
    if name == "main8":
        assert set(np.unique(r["level"][searched])) == set(range(8)) and len(np.unique(r["radius"][searched])) == 8
    else:
        assert (r["level"][searched] == 0).all() and (r["radius"][searched] == 10).all()


def test_planted_points_sit_on_the_edges(oracle):
    for proj_mode, dist_mode in MODES:
        P, c, r = solved(oracle, "planted", proj_mode, dist_mode)
        assert list(r["reject"]) == [code for _, code in S3.PLANTED_POINTS], (proj_mode, dist_mode)
        assert list(r["matched"]) == list(S3.PLANTED_MATCHED)
        assert r["nmatches"] == 6 and r["searched"] == 6
        assert tuple(r["proj"][1]) == (0.0, 240.0) and tuple(r["proj"][10]) == (320.0, 0.0) and tuple(r["proj"][6]) == (512.0, 240.0)
        assert r["best_idx"][5] == 1 and 5 in r["lists"][5]          # feature 5 was in the window, and matched before the call
    # the invalid point 4 would have taken feature 1, and point 5 would have been left with nothing
    P, c, _ = solved(oracle, "planted")
    v = S3.search(oracle, P, c, valid=np.ones(len(c["pw"]), np.uint8))
    assert v["reject"][4] == 0 and v["matched"][1] == 4 and v["best_idx"][5] == -1
    # the edges in numbers: exact in fp32
    front = S3.project(dict(P, proj_mode=S3.PROJ_DIV), c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"])
    assert front["reject"][4] == 0 and tuple(front["proj"][4]) == (320.0, 240.0)


# ---------------------------------------------------------------- the binding
def test_capi_binding_without_a_device():
    from rover_slam_amd import capi
    assert ctypes.sizeof(capi.Sim3Params) == 4 * (4 + 3 + 3 + 4 + 4 + 3 + capi.MAX_LEVELS + 2)
    assert {"rfe_search_by_projection_sim3", "rfe_search_by_projection_sim3_dev"} <= set(capi.EXPORTS)
    assert (capi.PROJ_INVZ, capi.PROJ_DIV, capi.DIST_FLOAT, capi.DIST_TRUNC) == (S3.PROJ_INVZ, S3.PROJ_DIV, S3.DIST_FLOAT, S3.DIST_TRUNC)
    P, _ = S3.planted_case()
    p = to_capi(P, S3.DIST_TRUNC)
    assert list(p.quat) == [0, 0, 0, 1] and p.th == 10 and p.nlevels == 1 and p.dist_mode == 1 and p.fx == 256 and p.max_x == 640
    z = np.zeros((256,), np.float32).ctypes.data
    lib = capi.lib                                                 # a NULL ctx is refused before anything else is looked at
    assert lib.rfe_search_by_projection_sim3(None, ctypes.byref(p), z, z, z, z, z, z, None, 1, z, z, None, None, 1, 1.2, z, *([None] * 8)) == -1
    assert lib.rfe_search_by_projection_sim3_dev(None, ctypes.byref(p), z, z, z, z, z, z, None, 1, z, z, None, None, 1, None, 1.2, 16, z,
                                                 *([None] * 7), z) == -1


# ---------------------------------------------------------------- the drop-in driver's case
def test_driver_case_keeps_the_problem(tmp_path):
    """t * s / s is not t in general: the driver's pose is its own, and the case is written so that validity survives the translation
    into isBad() / vpMatched"""
    P, c = main_case()
    Pd, prior = write_driver_case(str(tmp_path / "case.bin"), P, c)
    assert Pd["t"].dtype == np.float32 and np.abs(Pd["t"] - P["t"]).max() < 1e-6
    assert np.array_equal(prior != -1, c["matched_in"] != 0)
    owners = prior[prior >= 0]
    assert len(set(owners)) == len(owners) and (c["valid"][owners] == 0).all()
    size = 5 * 4 + 18 * 4 + 4 * P["nlevels"] + len(c["pw"]) + 4 * len(prior) + 4 * len(c["pw"]) * (3 + 3 + 1 + 1 + 1 + 256) + 4 * len(prior) * 258
    assert os.path.getsize(str(tmp_path / "case.bin")) == size
