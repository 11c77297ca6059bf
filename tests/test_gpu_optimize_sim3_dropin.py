"""GPU: the drop-in of include/rfe/optimize_sim3.h (OptimizeSim3_rfe) over mock KeyFrame / MapPoint / Sim3 types
(tests/cpp/optimize_sim3_driver.cpp) against the restatement tests/optimize_sim3_ref.py: the skip conditions of the reference's first loop,
the nulling of vpMatches1, g2oS12 untouched on `return 0`, mAcumHessian zeroed only past the second round."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import optimize_sim3_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SKIPS = (1, 2, 3, 4)            # vpMatches1[i] NULL; no pMP1; pMP1 bad; pMP2 bad


def spread(c, seed):
    """the case's n rows spread over n + 12 slots of vpMatches1, three of every skip kind in between; the case over those slots (a skipped
    slot holds a wild position and keypoint, and valid = 0) and the kinds"""
    rng = np.random.default_rng(seed)
    n = c["P"]["n"]
    kind = np.array([0] * n + list(SKIPS) * 3, np.int32)
    kind = kind[rng.permutation(len(kind))]
    M, where = len(kind), np.flatnonzero(kind == 0)
    d = dict(c, P=dict(c["P"], n=M))
    d["xw1"], d["xw2"] = rng.normal(0, 3, (M, 3)).astype(F32), rng.normal(0, 3, (M, 3)).astype(F32)
    d["kpts1"], d["octave1"] = rng.uniform(0, 700, (M, 2)).astype(F32), rng.integers(0, 4, M).astype(np.int32)
    d["idx2"], d["valid"] = rng.integers(-1, c["P"]["n2"], M).astype(np.int32), np.zeros(M, np.uint8)
    for k in ("xw1", "xw2", "kpts1", "octave1", "idx2", "valid"):
        d[k][where] = c[k][:n]
    return d, kind


def write_case(path, d, kind, cam2=0):
    P = d["P"]
    M, N2 = P["n"], P["n2"]
    slot = np.zeros(M, np.dtype([("kind", "<i4"), ("oct1", "<i4"), ("idx2", "<i4"), ("kp", "<f4", 2), ("x1", "<f4", 3), ("x2", "<f4", 3)]))
    slot["kind"], slot["oct1"], slot["idx2"], slot["kp"], slot["x1"], slot["x2"] = kind, d["octave1"], d["idx2"], d["kpts1"], d["xw1"], d["xw2"]
    slot["kind"][(kind == 0) & (d["valid"] == 0)] = 3          # a row the case itself marks invalid: a bad pMP1
    key2 = np.zeros(N2, np.dtype([("kp", "<f4", 2), ("oct", "<i4")]))
    key2["kp"], key2["oct"] = d["kpts2"][:N2], d["octave2"][:N2]
    with open(path, "wb") as f:
        np.array([M, N2, len(P["inv1"]), len(P["inv2"]), P["fix_scale"], P["all_points"], cam2], np.int32).tofile(f)
        np.array([P["th2"]], F32).tofile(f)
        np.asarray(d["s12_0"], F64).tofile(f)
        for a in (P["rcw1"], P["tcw1"], P["rcw2"], P["tcw2"], P["cam1"], P["cam2"], P["inv1"], P["inv2"]):
            np.ascontiguousarray(a, F32).tofile(f)
        slot.tofile(f)
        key2.tofile(f)


def read_out(path):
    raw = np.fromfile(path, np.uint8)
    hd = raw[:12].view(np.int32)
    return {"ret": int(hd[0]), "zeroed": int(hd[1]), "N": int(hd[2]), "stats": raw[12:44].view(np.int32), "s12": raw[44:108].view(F64),
            "matched": raw[108:]}


def run(exe, tmp_path, c, seed, **kw):
    d, kind = spread(c, seed)
    write_case(str(tmp_path / "case.bin"), d, kind, **kw)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    got = read_out(str(tmp_path / "out.bin"))
    assert got["N"] == len(kind) == len(got["matched"])
    return got, d, kind


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "optimize_sim3_driver")
    # 1. both rounds run: rows outside KF2 with and without bAllPoints, every skip kind in between
    for seed, all_points in ((1, True), (2, False)):
        c = R.scene(700 + seed, 150, mixed=True, pixel=False, all_points=all_points)
        got, d, kind = run(exe, tmp_path, c, seed)
        ref = R.solve(d)
        assert ref["stats"][3] == 2 and ref["ret"] > 60 and ref["stats"][2] > 0
        assert got["ret"] == ref["ret"] and np.array_equal(got["stats"], ref["stats"]) and np.array_equal(got["s12"], ref["s12"])
        assert got["zeroed"] == 1
        expect = (kind != 1) & (ref["keep"][:len(kind)] != 0)          # NULL stays NULL, a removed pair is nulled, everything else stays
        assert np.array_equal(got["matched"] != 0, expect)
        assert (got["matched"][np.isin(kind, (2, 3, 4))] == 1).all()   # skipped rows keep their pointer
        if not all_points:
            out = (kind == 0) & (d["idx2"] < 0)
            assert out.sum() > 20 and (got["matched"][out] == 1).all() and ref["stats"][1] == int(((kind == 0) & (d["idx2"] >= 0) & (d["valid"] != 0)).sum())
    # 2. `return 0`: nine survivors -- vpMatches1 already nulled, g2oS12 and mAcumHessian untouched
    c = R.forced("survivors9")
    got, d, kind = run(exe, tmp_path, c, 3)
    ref = R.solve(d)
    assert ref["stats"][7] & R.FLAG_EARLY and got["ret"] == 0 and np.array_equal(got["stats"], ref["stats"])
    assert np.array_equal(got["s12"], np.asarray(c["s12_0"], F64)) and got["zeroed"] == 0
    assert np.array_equal(got["matched"] != 0, (kind != 1) & (ref["keep"][:len(kind)] != 0)) and (got["matched"][kind == 0] == 0).sum() == 3
    # 3. a KannalaBrandt8 camera is refused: nothing is touched
    got, d, kind = run(exe, tmp_path, c, 3, cam2=1)
    assert got["ret"] == -100 and got["zeroed"] == 0          # RFE_OPTIMIZE_SIM3_NOT_SERVED, apart from every rfe_status
    assert got["zeroed"] == 0 and np.array_equal(got["s12"], np.asarray(c["s12_0"], F64))
    assert np.array_equal(got["matched"] != 0, kind != 1)
