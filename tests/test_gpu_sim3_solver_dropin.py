"""GPU: the drop-in of include/rfe/sim3_solver.h (Sim3Solver_rfe) over mock KeyFrame / MapPoint types (tests/cpp/sim3_solver_driver.cpp)
against the restatement tests/sim3_solver_ref.py: the constructor's five skip conditions and the scattering through mvnIndices1, the loop
while(!bConverge && !bNoMore) iterate(20, ..), and find()."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import sim3_solver_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SIGMA2 = (1.0, 1.44, 2.0736)
SKIPS = (1, 2, 3, 4, 5, 6)      # vpMatched12 NULL; no pMP1; pMP1 bad; pMP2 bad; pMP1 not in pKF1; pMP2 not in pKF2


def slots_of(c, seed):
    """the case's n correspondences spread over mN1 = n + 18 slots, three of every skip kind in between; returns kind [mN1] and the slot of
    every correspondence (mvnIndices1)"""
    rng = np.random.default_rng(seed)
    n = c["P"]["n"]
    kind = np.array([0] * n + list(SKIPS) * 3, np.int32)
    kind = kind[rng.permutation(len(kind))]
    return kind, np.flatnonzero(kind == 0)


def write_case(path, c, kind, where, probability, max_its, mode=0, cam2=0, third_kf=0, seed=0):
    rng = np.random.default_rng(seed)
    P, M = c["P"], len(kind)
    lv = {k: np.array([int(np.flatnonzero(np.asarray(SIGMA2, F32) == v)[0]) for v in c[k]], np.int32) for k in ("s1", "s2")}
    slot = np.zeros(M, np.dtype([("kind", "<i4"), ("oct1", "<i4"), ("oct2", "<i4"), ("idx2", "<i4"), ("x1", "<f4", 3), ("x2", "<f4", 3)]))
    slot["kind"], slot["idx2"] = kind, rng.permutation(M)
    slot["oct1"], slot["oct2"] = rng.integers(0, 3, M), rng.integers(0, 3, M)
    slot["x1"], slot["x2"] = rng.normal(0, 3, (M, 3)), rng.normal(0, 3, (M, 3))        # what a skipped slot holds must not matter
    slot["oct1"][where], slot["oct2"][where], slot["x1"][where], slot["x2"][where] = lv["s1"], lv["s2"], c["xw1"], c["xw2"]
    draws = np.ascontiguousarray(c["draws"], np.int32).reshape(-1)
    with open(path, "wb") as f:
        np.array([M, 3, 3, P["fix_scale"], P["min_inliers"], max_its, mode, cam2, len(draws), third_kf], np.int32).tofile(f)
        np.array([probability], np.float64).tofile(f)
        for a in (P["rcw1"], P["tcw1"], P["rcw2"], P["tcw2"], P["cam1"], P["cam2"], SIGMA2, SIGMA2):
            np.ascontiguousarray(a, F32).tofile(f)
        slot.tofile(f)
        draws.tofile(f)


def read_out(path):
    raw = np.fromfile(path, np.uint8)
    hd = raw[:40].view(np.int32)
    o = dict(zip(("status", "converged", "no_more", "n_inliers", "calls", "taken", "mN1", "N", "its", "bad_bounds"), (int(v) for v in hd)))
    f = raw[72:72 + 45 * 4].view(F32)
    o.update(stats=raw[40:72].view(np.int32), T=f[:16], T_best=f[16:32], R=f[32:41], t=f[41:44], s=f[44], inliers=raw[72 + 180:])
    assert len(o["inliers"]) == o["mN1"]
    return o


def run(exe, tmp_path, c, probability=0.99, max_its=300, seed=0, **kw):
    kind, where = slots_of(c, seed)
    write_case(str(tmp_path / "case.bin"), c, kind, where, probability, max_its, seed=seed, **kw)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin")), where


def expected(c, probability, max_its):
    """the restatement under the iteration count SetRansacParameters arrives at"""
    c = dict(c, P=dict(c["P"], its=R.ransac_iterations(probability, c["P"]["min_inliers"], c["P"]["n"], max_its)))
    return c, R.solve(c)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "sim3_solver_driver")
    # 1. the loop converges: planted scene, 40 % outliers
    c0 = R.scene(5, 150, outliers=0.4, H=300)
    c, ref = expected(c0, 0.99, 300)
    for third_kf in (0, 1):                               # a vpKeyFrameMatchedMP list leaves pKFm = pKF2 (:40-45, :85-86 as written)
        got, where = run(exe, tmp_path, c, third_kf=third_kf)
        assert got["status"] == 0 and got["bad_bounds"] == 0 and got["N"] == 150 and got["mN1"] == 168 and got["its"] == c["P"]["its"]
        assert got["taken"] == 3 * got["its"]                                         # departure (d): every draw up front
        assert np.array_equal(got["stats"], ref["stats"]) and ref["stats"][0] == 1
        assert (got["converged"], got["no_more"], got["n_inliers"]) == (1, 0, ref["stats"][1]) and got["calls"] == -(-ref["stats"][4] // 20)
        assert np.array_equal(got["T"], ref["T12"]) and np.array_equal(got["T_best"], ref["T12"]) and np.array_equal(got["R"], ref["R"])
        assert np.array_equal(got["t"], ref["t"]) and got["s"] == ref["s"]
        scattered = np.zeros(got["mN1"], np.uint8)
        scattered[where] = ref["inliers"]
        assert np.array_equal(got["inliers"], scattered) and scattered.sum() == 90
    # 2. it does not: min_inliers above the inliers there are; the best so far comes back with bNoMore after ceil(its / 20) calls
    c, ref = expected(R.scene(6, 150, outliers=0.4, min_inliers=100, H=300), 0.99999, 300)
    got, where = run(exe, tmp_path, c, probability=0.99999, seed=1)
    assert np.array_equal(got["stats"], ref["stats"]) and ref["stats"][0] == 0 and ref["stats"][2] == 90 and got["its"] > 20
    assert (got["converged"], got["no_more"], got["n_inliers"]) == (0, 1, 0) and got["calls"] == -(-got["its"] // 20) and not got["inliers"].any()
    assert np.array_equal(got["T"], ref["T12"]) and np.array_equal(got["R"], ref["R"]) and np.array_equal(got["t"], ref["t"]) and got["s"] == ref["s"]
    # 3. find(): the four-argument overload over all iterations -- the transform on convergence, the identity without
    c, ref = expected(c0, 0.97, 300)
    got, where = run(exe, tmp_path, c, probability=0.97, mode=1)
    assert got["calls"] == 1 and np.array_equal(got["T"], ref["T12"]) and got["n_inliers"] == ref["stats"][1] == 90
    c, ref = expected(R.scene(6, 150, outliers=0.4, min_inliers=100, H=300), 0.99, 300)
    got, where = run(exe, tmp_path, c, mode=1)
    assert np.array_equal(got["T"].reshape(4, 4), np.eye(4)) and np.array_equal(got["T_best"], ref["T12"]) and got["n_inliers"] == 0
    # 4. fewer correspondences than min_inliers: bNoMore at once, nothing drawn
    c = R.scene(7, 5, outliers=0.0, min_inliers=6)
    got, where = run(exe, tmp_path, c)
    assert (got["converged"], got["no_more"], got["taken"], got["calls"]) == (0, 1, 0, 1) and np.array_equal(got["T"].reshape(4, 4), np.eye(4))
    # 5. a KannalaBrandt8 camera is refused, nothing is drawn
    got, where = run(exe, tmp_path, c0, cam2=1)
    assert got["status"] == -1 and (got["converged"], got["no_more"], got["taken"]) == (0, 1, 0) and np.array_equal(got["T"].reshape(4, 4), np.eye(4))
