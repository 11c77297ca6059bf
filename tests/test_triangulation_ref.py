"""CPU: the numpy restatement of DESIGN.md 6g (tests/triangulation_ref.py) against a scalar, per-slot, float64 transcription of the reference
text (src/LocalMapping.cc:579-943, SPmatcher.cc:1376-1393, GeometricTools.cc:63-90, KeyFrame.cc:941-960): numpy.linalg.svd for Eigen's
JacobiSVD, cos(2 atan2) for the stereo parallax, and the sequential loop over the neighbours that marks a feature taken at once."""
import math

import numpy as np
import pytest

import triangulation_ref as T

F64 = np.float64


def transcription(P, c):
    """-> code [Nn,Kmax] (3 also for a feature an earlier neighbour took), x3d [Nn,Kmax,3] float64, created [(n, k)]"""
    v1 = {k: np.asarray(v, F64) for k, v in c["view1"].items()}
    Nn, Kmax = c["pairs"].shape[:2]
    N1 = len(c["kpts1"])
    has1 = c["has_mp1"].astype(bool).copy()
    k1raw = c["kpts1"] if c.get("kpts1_raw") is None else c["kpts1_raw"]
    k2raw = c["kpts2"] if c.get("kpts2_raw") is None else c["kpts2_raw"]
    sf, sig = np.asarray(P["scale_factors"], F64), np.asarray(P["level_sigma2"], F64)
    code = np.full((Nn, Kmax), T.NO_SLOT, np.int32)
    x3d = np.zeros((Nn, Kmax, 3), F64)
    created = []
    T1 = np.hstack([v1["rcw"], v1["tcw"][:, None]])
    for n in range(Nn):
        S = int(min(max(c["S"][n], 0), Kmax))
        if c.get("neighbour_valid") is not None and not c["neighbour_valid"][n]:
            code[n, :S] = 1
            continue
        v2 = {k: np.asarray(v, F64) for k, v in c["views2"][n].items()}
        T2 = np.hstack([v2["rcw"], v2["tcw"][:, None]])
        for k in range(S):
            i, j = (int(v) for v in c["pairs"][n, k])
            if not (0 <= i < N1 and 0 <= j < c["n2"][n]):
                code[n, k] = 2
                continue
            if has1[i] or c["has_mp2"][n, j]:
                code[n, k] = 3
                continue
            kp1, kp2 = c["kpts1"][i].astype(F64), c["kpts2"][n, j].astype(F64)
            ur1, ur2 = float(c["uright1"][i]), float(c["uright2"][n, j])
            st1, st2 = ur1 >= 0, ur2 >= 0
            xn1 = np.array([(kp1[0] - v1["cx"]) / v1["fx"], (kp1[1] - v1["cy"]) / v1["fy"], 1.0])
            xn2 = np.array([(kp2[0] - v2["cx"]) / v2["fx"], (kp2[1] - v2["cy"]) / v2["fy"], 1.0])
            ray1, ray2 = v1["rcw"].T @ xn1, v2["rcw"].T @ xn2
            with np.errstate(all="ignore"):
                cosr = ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2))
            cs1 = cs2 = cosr + 1
            if st1:
                cs1 = math.cos(2 * math.atan2(float(v1["mb"]) / 2, float(c["depth1"][i])))
            elif st2:
                cs2 = math.cos(2 * math.atan2(float(v2["mb"]) / 2, float(c["depth2"][n, j])))
            cst = cs2 if cs2 < cs1 else cs1
            stereo = False
            if cosr < cst and cosr > 0 and (st1 or st2 or (cosr < 0.9996 and P["inertial"]) or (cosr < 0.9998 and not P["inertial"])):
                A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
                h = np.linalg.svd(A)[2][3]
                if h[3] == 0:
                    code[n, k] = 4
                    continue
                X = h[:3] / h[3]
            elif st1 and cs1 < cs2:
                stereo = True
                z = float(c["depth1"][i])
                if not z > 0:
                    code[n, k] = 6
                    continue
                X = v1["rcw"].T @ np.array([(k1raw[i][0] - v1["cx"]) * z * v1["invfx"], (k1raw[i][1] - v1["cy"]) * z * v1["invfy"], z]) + v1["ow"]
            elif st2 and cs2 < cs1:
                stereo = True
                z = float(c["depth2"][n, j])
                if not z > 0:
                    code[n, k] = 6
                    continue
                X = v2["rcw"].T @ np.array([(k2raw[n, j][0] - v2["cx"]) * z * v2["invfx"], (k2raw[n, j][1] - v2["cy"]) * z * v2["invfy"], z]) + v2["ow"]
            else:
                code[n, k] = 5
                continue
            x3d[n, k] = X
            fail = 0
            with np.errstate(all="ignore"):
                z1 = v1["rcw"][2] @ X + v1["tcw"][2]
                z2 = v2["rcw"][2] @ X + v2["tcw"][2]
                if z1 <= 0:
                    fail = 7
                elif z2 <= 0:
                    fail = 8
                for v, z, kp, ur, st, o, base in ((v1, z1, kp1, ur1, st1, c["octave1"][i], 9), (v2, z2, kp2, ur2, st2, c["octave2"][n, j], 11)):
                    if fail:
                        break
                    x, y = v["rcw"][0] @ X + v["tcw"][0], v["rcw"][1] @ X + v["tcw"][1]
                    if not st:
                        ex, ey = v["fx"] * x / z + v["cx"] - kp[0], v["fy"] * y / z + v["cy"] - kp[1]
                        if ex * ex + ey * ey > 5.991 * sig[o]:
                            fail = base
                    else:
                        invz = 1.0 / z
                        u = v["fx"] * x * invz + v["cx"]
                        ex, ey, er = u - kp[0], v["fy"] * y * invz + v["cy"] - kp[1], u - v1["mbf"] * invz - ur
                        if ex * ex + ey * ey + er * er > 7.8 * sig[o]:
                            fail = base + 1
                if not fail:
                    d1, d2 = np.linalg.norm(X - v1["ow"]), np.linalg.norm(X - v2["ow"])
                    if d1 == 0 or d2 == 0:
                        fail = 13
                    elif P["far_points"] and (d1 >= P["th_far"] or d2 >= P["th_far"]):
                        fail = 14
                    else:
                        rd, ro, rf = d2 / d1, sf[c["octave1"][i]] / sf[c["octave2"][n, j]], float(P["ratio_factor"])
                        if rd * rf < ro or rd > ro * rf:
                            fail = 15
            code[n, k] = fail
            if not fail:
                has1[i] = True                                          # mpCurrentKeyFrame->AddMapPoint(pMP, idx1), :930
                created.append((n, k, stereo))
    return code, x3d, created


@pytest.fixture(scope="module")
def main():
    P, c, ref = T.solved("main", True, False)
    return P, c, ref, transcription(P, c)


def _pixels(v, X):
    pc = X @ np.asarray(v["rcw"], F64).T + np.asarray(v["tcw"], F64)
    return np.array([float(v["fx"]) * pc[0] / pc[2] + float(v["cx"]), float(v["fy"]) * pc[1] / pc[2] + float(v["cy"])])


@pytest.mark.parametrize("name,far,inertial", (("main", True, False), ("main", False, True), ("posed", True, False)))
def test_restatement_against_float64_transcription(name, far, inertial):
    P, c, ref = T.solved(name, far, inertial)
    code64, x64, created64 = transcription(P, c)
    made32, made64 = ref["code"] == 0, code64 == 0
    slots = int(ref["stats"][1])
    differ = made32 != made64
    print(f"{name}: {slots} slots, created {made32.sum()} / {made64.sum()} (float64), decisions that differ {differ.sum()}")
    assert differ.sum() <= 0.002 * slots                                # a cap, not a tolerance
    assert not (differ & c["clear"]).any() and c["clear"].sum() > 0.15 * slots
    # wherever the decisions agree: the same slots in the same (creation) order, and on the clear slots the same first failing gate
    agree = ~differ
    l32 = [(n, k) for n, k in zip(ref["out_n"], (np.flatnonzero(made32.reshape(-1)) % made32.shape[1])) if agree[n, k]]
    l64 = [(n, k) for n, k, _ in created64 if agree[n, k]]
    assert l32 == l64 and len(l32) > 100
    assert np.array_equal(ref["out_stereo"][[agree[n, k] for n, k in zip(ref["out_n"], np.flatnonzero(made32.reshape(-1)) % made32.shape[1])]],
                          np.array([s for n, k, s in created64 if agree[n, k]], np.uint8))
    c32 = np.where(ref["code"] == T.CLAIMED, 3, ref["code"])            # the transcription sees a taken feature as an existing map point
    untouched = c["clear"] & ~((ref["code"] != T.CLAIMED) & (code64 == 3) & (ref["code"] != 3))   # ... even where its own gates would fail
    assert np.array_equal(c32[untouched], code64[untouched])
    # the points: both reprojected into both views
    worst = 0.0
    for n, k in l32:
        if not np.isfinite(ref["x3d"][n, k]).all():
            continue
        for v in (c["view1"], c["views2"][n]):
            worst = max(worst, float(np.abs(_pixels(v, ref["x3d"][n, k].astype(F64)) - _pixels(v, x64[n, k])).max()))
    print(f"largest reprojection difference to the float64 points: {worst:.2e} px")
    assert worst <= 0.01


def test_lowest_neighbour_wins(main):
    P, c, ref, _ = main
    e = T.evaluate(P, c)
    passing = e["code"] == 0
    i = c["pairs"][..., 0]
    multi = 0
    for f in np.unique(i[passing]):
        ns = np.flatnonzero((passing & (i == f)).any(1))
        multi += len(ns) > 1
        for n in ns:
            k = int(np.flatnonzero(passing[n] & (i[n] == f))[0])
            assert ref["code"][n, k] == (0 if n == ns[0] else T.CLAIMED)
    assert multi >= 100
    # creation order: n ascending, then k
    key = ref["out_n"].astype(np.int64) * 10000 + np.array([int(np.flatnonzero((i[n] == f) & (ref["code"][n] == 0))[0])
                                                             for n, f in zip(ref["out_n"], ref["out_idx1"])])
    assert (np.diff(key) > 0).all() and len(np.unique(ref["out_idx1"])) == len(ref["out_idx1"]) == ref["created"]


def test_stereo_parallax_is_the_cosine_of_twice_the_angle():
    worst = 0.0
    for name in ("main", "posed"):
        _, c = T.case_of(name)
        for mb, d in [(c["view1"]["mb"], c["depth1"][c["uright1"] >= 0])] + [(v["mb"], c["depth2"][n][c["uright2"][n] >= 0]) for n, v in enumerate(c["views2"])]:
            d = d[d > 0]
            want = np.cos(2 * np.arctan2(float(mb) / 2, d.astype(F64)))
            got = T.stereo_parallax(mb, d)
            assert got.dtype == np.float32
            worst = max(worst, float(np.abs(got.astype(F64) - want).max()) if len(d) else 0.0)
    print(f"largest |(dd - hh) / (dd + hh) - cos(2 atan2(mb / 2, d))|: {worst:.3e} = {worst / np.spacing(np.float32(1)):.2f} ulp of 1")
    assert 0 < worst < 4 * np.spacing(np.float32(1))


def test_every_code_occurs_in_the_main_case(main):
    P, c, ref, _ = main
    hist = np.bincount(ref["code"][ref["code"] >= 0], minlength=len(T.CODES))
    for code, (name, count) in enumerate(zip(T.CODES, hist)):
        print(f"{code:2d} {name:34s} {count}")
    assert len(hist) == len(T.CODES) == 17 and (hist > 0).all()
    assert (ref["code"] == T.NO_SLOT).sum() == ref["code"].size - int(np.clip(c["S"], 0, None).sum())
    st = ref["stats"]
    assert st[0] == hist[0] and st[2] == hist[3] and 0 < st[3] < st[4] and st[5] == 0 and (st[6:] == 0).all()
    assert st[1] == sum(int(s) for s, v in zip(c["S"], c["neighbour_valid"]) if v)


def test_sweep_count():
    """The count from which decisions and created points no longer change on the generators' pairs (main: 3, posed: 4), plus two.  "No
    longer change" is: the same codes, and every created point within 1e-6 of its largest coordinate -- below the method's own distance to a
    float64 SVD.  Bit for bit they never stop changing: with `rotate unless gamma == 0` a converged pair still turns by an angle of
    rounding size, which moves last bits of V (about 50 rejected outlier slots of the main case, and a created point 570 m away in the
    posed one -- its w is small, so x / w moves by up to 3 ulps -- at every count up to 12)."""
    settled = {}
    for name in ("main", "posed"):
        base, c = T.case_of(name)
        runs = {s: T.triangulate(T.P(base, False, False), c, sweeps=s) for s in range(2, 11)}

        def same(a, b):
            if not np.array_equal(a["code"], b["code"]):
                return False
            scale = np.abs(a["out_x3d"]).max(1, keepdims=True)
            return bool((np.abs(a["out_x3d"] - b["out_x3d"]) <= 1e-6 * scale).all())
        settled[name] = min(s for s in runs if all(same(runs[s], runs[t]) for t in runs if t > s))
    print("settled from", settled, "sweeps on")
    assert T.SWEEPS == max(settled.values()) + 2


def test_planted_case_codes():
    base, c, expect = T.planted_case()
    for inertial in (False, True):
        r = T.triangulate(T.P(base, True, inertial), c)
        for name, (n, k, code, code_in) in expect.items():
            assert r["code"][n, k] == (code_in if inertial else code), name
        for name, (n, k, target) in c["expect_cos"].items():
            assert r["cosr"][n, k] == target, name
        assert r["stats"][5] == 1                                       # the NaN point
    n, k = expect["both_stereo"][:2]
    assert list(r["x3d"][n, k]) == [0, 0, 8] and r["point_stereo"][n, k] == 1
    n, k = expect["z1_minus_zero"][:2]
    assert r["x3d"][n, k][2] == 0 and np.signbit(r["x3d"][n, k][2])
    n, k = expect["far_at"][:2]
    assert T.triangulate(T.P(base, False, False), c)["code"][n, k] == 0
