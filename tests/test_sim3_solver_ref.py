"""CPU: the contract of DESIGN.md 6j as tests/sim3_solver_ref.py restates it.
  1. the vectorised restatement equals, in every output bit, the sequential transcription of Sim3Solver.cc (np.float32 scalars, a real
     vAvailableIndices list, the iterate(20) loop with mnBestInliers carried across chunks);
  2. departures (a)-(c) measured against the transcription with the reference's own choices (eigh on float64, the angle-axis route,
     float64 sums), inlier sets included;
  3. a planted Sim3 is recovered;
  4. the forced paths;
  5. rfe_sim3_ransac_iterations against SetRansacParameters' formula.
Measured over every hypothesis these cases run (1325, one degenerate triple apart; profiles/sim3_solver.md): the rotations differ by at most
3.3e-6 rad, s by 3.9e-7 and t by 9.7e-6 relative, the Jacobi leaves |N q - lambda q| <= 3.3e-16 |N|, no count and no flag differs, and no
e1 / e2 of the float64 run comes closer than 7.6e-3 relative to its bound.  The bounds below are four times those maxima (the project's
factor for fp32 noise, profiles/lg_assign.md)."""
import math

import numpy as np
import pytest

import sim3_solver_ref as R

F32 = np.float32
SIZES = [(n, its, fs) for n in (3, 4, 20, 64, 65, 300) for its in (1, 5, 300) for fs in (0, 1)]
ANGLE_BOUND, S_BOUND, T_BOUND, RESIDUAL_BOUND = 4 * 3.3e-6, 4 * 3.9e-7, 4 * 9.7e-6, 4 * 3.3e-16
MARGIN = 1e-3


def sized(n, its, fs):
    return R.scene(1000 + 17 * n + its + fs, n, its=its, fix_scale=fs)


def planted():
    return R.scene(5, 150, outliers=0.4, s=1.3, angle=0.4)


def same_as_sequential(c, chunk=20):
    v, q = R.solve(c), R.Sequential(c)
    r = q.run(chunk)
    ran = len(r["counts"])
    assert ran == r["stats"][4] == v["stats"][4]
    for k in r:
        a = v[k][:ran] if k == "counts" else v[k]
        assert a.dtype == r[k].dtype == R.OUT[k] and a.shape == r[k].shape, (k, a.dtype, r[k].dtype, a.shape, r[k].shape)
        assert np.array_equal(a, r[k], equal_nan=True), (k, a, r[k])
    for h, (Rh, th, sh) in enumerate(q.log):                        # and every hypothesis' record, as far as the loop ran
        rec = v["hyps"][h]
        assert np.array_equal(rec[16:25], np.asarray(Rh, F32).reshape(9), equal_nan=True) and np.array_equal(rec[25:28], th, equal_nan=True)
        assert np.array_equal(rec[28], F32(sh), equal_nan=True)
    return v, q


# ---------------------------------------------------------------- 1. restatement == sequential transcription
@pytest.mark.parametrize("n,its,fs", SIZES)
def test_restatement_equals_sequential(n, its, fs):
    v, q = same_as_sequential(sized(n, its, fs))
    print(f"n={n} its={its} fix_scale={fs}: stats {v['stats'].tolist()}")


def test_sizes_cover_both_ends_of_the_choice():
    st = np.array([R.solve(sized(*a))["stats"] for a in SIZES])
    assert (st[:, 0] == 1).any() and (st[:, 0] == 0).any() and (st[:, 4] > 20).any()       # converged, not converged, past one chunk


@pytest.mark.parametrize("chunk", [1, 3, 20, 1000])
def test_chunking_does_not_matter(chunk):
    same_as_sequential(sized(64, 300, 0), chunk)
    same_as_sequential(R.forced("max_three_times"), chunk)


# ---------------------------------------------------------------- 2. the departures, measured
def test_departures_measured():
    cases = [sized(*a) for a in SIZES] + [R.forced(k) for k in R.FORCED] + [planted()]
    m = R.measure(cases)
    print("departures:", m)
    assert m["margin"] > MARGIN                   # first, on the float64 transcription alone: no error near its integer bound
    assert m["hypotheses"] > 1000 and m["degenerate"] == 1          # the collinear triple of forced("collinear")
    assert m["same_inliers"]
    assert m["angle"] <= ANGLE_BOUND and m["s"] <= S_BOUND and m["t"] <= T_BOUND and m["residual"] <= RESIDUAL_BOUND
    assert min(ANGLE_BOUND, S_BOUND, T_BOUND) > 4 * np.finfo(F32).eps


# ---------------------------------------------------------------- 3. it solves the problem
def test_planted_sim3_is_recovered():
    c = planted()
    v = R.solve(c)
    tr = c["truth"]
    assert c["P"]["n"] == 150 and c["is_out"].sum() == 60
    assert v["stats"][0] == 1 and v["stats"][5] == 0 and v["stats"][1] == 90
    assert np.array_equal(v["inliers"] != 0, ~c["is_out"]) and np.array_equal(v["best_inliers"], v["inliers"])
    Rm = v["R"].reshape(3, 3).astype(np.float64)
    assert np.linalg.norm(Rm - tr["R"]) / math.sqrt(2) <= ANGLE_BOUND
    assert abs(float(v["s"]) - tr["s"]) / tr["s"] <= S_BOUND
    assert np.linalg.norm(v["t"] - tr["t"]) / np.linalg.norm(tr["t"]) <= T_BOUND
    T = v["T12"].reshape(4, 4)
    assert np.array_equal(T[:3, :3], v["s"] * v["R"].reshape(3, 3)) and np.array_equal(T[:3, 3], v["t"]) and T[3].tolist() == [0, 0, 0, 1]


# ---------------------------------------------------------------- 4. forced paths
@pytest.mark.parametrize("name", [k for k in R.FORCED if k != "n_lt_min"])
def test_forced_equals_sequential(name):
    same_as_sequential(R.forced(name))


def test_convergence_first_and_last():
    a, b = R.solve(R.forced("conv_first")), R.solve(R.forced("conv_last"))
    assert a["stats"].tolist() == [1, 20, 20, 0, 1, 0, 0, 0] and a["counts"].tolist() == [20, 0, 0, 20, 0]    # those behind the winner are still counted
    assert b["stats"].tolist() == [1, 20, 20, 4, 5, 0, 0, 0]                                                  # at its - 1: bNoMore stays false


def test_last_maximum_is_chosen():
    c = R.forced("max_three_times")
    v = R.solve(c)
    assert v["counts"].tolist() == [0, 20, 0, 20, 20, 0] and v["stats"].tolist() == [0, 0, 20, 4, 6, 1, 0, 0]
    assert not v["inliers"].any() and v["best_inliers"].sum() == 20
    assert np.array_equal(v["T12"], v["hyps"][4, :16]) and not np.array_equal(v["hyps"][4, :16], v["hyps"][3, :16])


def test_n_equal_and_below_min_inliers():
    c = R.forced("n_eq_min")
    assert c["P"]["its"] == 1
    v = R.solve(c)
    assert v["stats"].tolist() == [0, 0, 12, 0, 1, 1, 0, 0] and not v["inliers"].any() and v["best_inliers"].all()     # > is strict
    c = R.forced("n_lt_min")
    v = R.solve(c, fill={"counts": np.full(4, 77), "inliers": np.full(5, 9)})
    assert v["stats"].tolist() == [0, 0, 0, -1, 0, 1, 0, R.FLAG_FEW] and np.array_equal(v["T12"].reshape(4, 4), np.eye(4))
    assert (v["counts"] == 77).all() and not v["inliers"].any()
    assert R.Sequential(c).iterate(20)[1] is True
    two = R.scene(3, 2, outliers=0.0, min_inliers=1, its=2)
    assert R.solve(two)["stats"].tolist() == [0, 0, 0, -1, 0, 1, 0, R.FLAG_BELOW_THREE]


def test_pure_translation_is_a_nan_rotation():
    v = R.solve(R.forced("pure_translation"))
    assert np.isnan(v["hyps"][0, 16:28]).all() and np.isnan(v["hyps"][0, :12]).all() and v["hyps"][0, 12:16].tolist() == [0, 0, 0, 1]
    assert v["counts"][0] == 0 and v["hyps"][0, 29:30].view(np.int32)[0] == R.HYP_NAN and v["stats"][6] == 1 and v["stats"][0] == 1
    v = R.solve(R.forced("pure_translation_only"))                   # 0 >= mnBestInliers = 0: the NaN transform is the best one
    assert v["stats"].tolist() == [0, 0, 0, 0, 1, 1, 1, 0] and np.isnan(v["T12"][:12]).all() and np.isnan(v["R"]).all() and np.isnan(v["t"]).all()
    assert not v["best_inliers"].any()


def test_collinear_triple_runs():
    v = R.solve(R.forced("collinear"))
    assert np.isfinite(v["hyps"][0, :29]).all() and v["counts"].tolist() == [3, 12]


def test_threshold_is_truncated():
    c = R.forced("threshold")
    f = R.front(c["P"], c["xw1"], c["xw2"], c["s1"], c["s2"])
    assert (f["max1"] == 13).all() and 9.210 * 1.44 > 13.26 - 1e-9
    v = R.solve(c)
    rec = v["hyps"][0]
    Rm, t, s = rec[16:25].reshape(1, 3, 3), rec[25:28].reshape(1, 3), rec[28:29]
    e1, e2 = R.errors(c["P"], f, *R.transforms(Rm, s, t)[:1], t, *R.transforms(Rm, s, t)[1:])
    assert 13 < e1[0, 0] < 13.26 and 12.5 < e1[0, 1] < 13 and (e2[0, :2] < 921).all()
    assert v["best_inliers"][:2].tolist() == [0, 1] and v["best_inliers"][2:].all()


def test_behind_the_camera_and_nan():
    c = R.forced("behind")
    v = R.solve(c)
    assert v["best_inliers"].tolist() == [0] + [1] * 11               # no depth gate: it is the error that rejects it
    c = R.forced("nan")
    v = R.solve(c)
    assert v["best_inliers"].tolist() == [0, 0] + [1] * 10 and np.isfinite(v["T12"]).all()


def test_displaced_entries_and_out_of_range_draws():
    c = R.forced("displaced")
    n = c["P"]["n"]
    idx, clamped = R.resolve_draws(c["draws"], n)
    assert idx.tolist() == [[5, n - 1, 1], [n - 1, 3, n - 2], [n - 2, 2, n - 1], [n - 2, n - 1, n - 3], [4, 7, n - 1], [n - 1, n - 2, n - 3], [0, n - 1, n - 2]]
    assert not clamped.any() and all(len(set(r)) == 3 for r in idx.tolist())
    c = R.forced("out_of_range")
    idx, clamped = R.resolve_draws(c["draws"], n)
    assert clamped.all() and idx.min() >= 0 and idx.max() <= n - 1 and all(len(set(r)) == 3 for r in idx.tolist())
    v = R.solve(c)
    assert v["stats"][7] == R.FLAG_CLAMPED and (v["hyps"][:4, 29].view(np.int32) == R.HYP_CLAMPED).all()


# ---------------------------------------------------------------- 5. SetRansacParameters
def test_ransac_iterations():
    from rover_slam_amd import capi

    def formula(p, mn, n, mx):
        if mn == n:
            return 1
        eps = float(F32(mn) / F32(n))
        return max(1, min(math.ceil(math.log(1 - p) / math.log(1 - math.pow(eps, 3))), mx))

    cases = [(0.99, 20, 20, 300), (0.99, 6, 20, 300), (0.97, 10, 100, 300), (0.99, 3, 150, 300), (0.99, 15, 16, 300), (0.5, 19, 20, 300),
             (0.99, 8, 40, 300), (0.999999, 2, 300, 300), (0.99, 40, 4096, 1024)]
    for a in cases:
        assert capi.sim3_ransac_iterations(*a) == R.ransac_iterations(*a) == formula(*a), a
    assert formula(0.99, 20, 20, 300) == 1                                             # min == n
    assert formula(0.99, 3, 150, 300) == 300 and formula(0.99, 40, 4096, 1024) == 1024  # lands on the cap
    assert 1 < formula(0.99, 6, 20, 300) < 300
    # epsilon = 1 is min == n.  A quotient that is NaN (epsilon past 1: the log of a negative number; n = 0) or past int (probability 1;
    # 1 / 4096 cubed: 3.2e11 iterations) converts to INT_MIN on x86-64, so the reference runs ONE iteration there, and so does this
    for a in ((0.99, 21, 20, 300), (0.99, 5, 0, 300), (1.0, 6, 20, 300), (0.99, 1, 4096, 1024)):
        assert capi.sim3_ransac_iterations(*a) == R.ransac_iterations(*a) == 1, a
