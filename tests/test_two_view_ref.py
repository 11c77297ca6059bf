"""CPU: the restatement of DESIGN.md 6o (tests/two_view_ref.py, what rfe_two_view computes) against the sequential transcription of the
reference's lines (tests/two_view_seq.py) on four planted generators, the cost of departures (a) - (c), the sweep-count study, the draw
resolution against a literal transcription of :99-115, the forced paths, the exports and the drop-in's compile check.

Measured on the generators below (seeds 1 - 3, 300 matches, 200 iterations), restatement against transcription: rotation between the two
R21 at most 0.0800 degrees, angle between the two t21 at most 0.0307 degrees, largest p3d difference 1.0e-4, differing triangulated flags
0, differing inlier flags 0 (H) and 0 (F).  The asserts below are four times the maxima; the flag counts are asserted as measured."""
import os
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import two_view_ref as R
import two_view_seq as Q

F32 = np.float32
MEASURED = {"rot_deg": 0.0800, "t_deg": 0.0307, "p3d": 1.0e-4, "triangulated": 0, "inliers_h": 0, "inliers_f": 0}
# generator -> (model, ret, exit) the transcription must give; "rotation" runs twice: with the threshold above RH (F) and below it (H)
GENERATORS = {"general": (2, 1, R.EXIT_OK), "plane": (1, 1, R.EXIT_OK), "rotation": (2, 0, R.EXIT_NO_WINNER), "rotation_h": (1, 0, R.EXIT_NO_WINNER),
              "low_parallax": (2, 0, R.EXIT_PARALLAX)}
SEEDS = (1, 2, 3)
_CACHE = {}


def pair(kind, seed):
    """the case, the restatement's answer and the transcription's, computed once"""
    if (kind, seed) not in _CACHE:
        c = R.scene(seed, kind=kind)
        _CACHE[kind, seed] = (c, R.run(c), Q.reconstruct(c["P"], c["kpts1"], c["kpts2"], c["pairs"], c["draws"]))
    return _CACHE[kind, seed]


@pytest.mark.parametrize("kind", list(GENERATORS))
def test_restatement_against_transcription(kind):
    model, ret, exit_code = GENERATORS[kind]
    for seed in SEEDS:
        c, r, q = pair(kind, seed)
        thr = 0.5 if c["P"]["rh_threshold"] == 0 else c["P"]["rh_threshold"]
        print(f"{kind} seed {seed}: RH {float(q['RH']):.4f} (threshold {thr}), model {q['model']}, ret {int(q['ret'])}, exit {q['exit']}")
        assert (q["model"], int(q["ret"]), q["exit"]) == (model, ret, exit_code)          # the generator gives the stated outcome ...
        assert abs(float(q["RH"]) - thr) >= 0.02                                          # ... at least 0.02 from the threshold in use
        assert (int(r["stats"][1]), int(r["stats"][0]), int(r["stats"][11])) == (q["model"], int(q["ret"]), q["exit"])
        assert r["stats"][12] == 0 and r["stats"][3] == q["win"][0] and r["stats"][4] == q["win"][1]
        assert int((r["inliers_h"].astype(bool) != q["inliers_h"]).sum()) == MEASURED["inliers_h"]
        assert int((r["inliers_f"].astype(bool) != q["inliers_f"]).sum()) == MEASURED["inliers_f"]
        if not ret:
            assert np.array_equal(r["R21"].reshape(3, 3), np.eye(3)) and not r["t21"].any() and not r["triangulated"].any()
            continue
        Rr, Rq = r["R21"].reshape(3, 3).astype(np.float64), q["R21"].astype(np.float64)
        rot = np.degrees(np.arccos(np.clip((np.trace(Rr @ Rq.T) - 1) / 2, -1, 1)))
        tdeg = np.degrees(np.arccos(np.clip(r["t21"].astype(np.float64) @ q["t21"].astype(np.float64), -1, 1)))
        p3d = float(np.abs(r["p3d"] - q["p3d"]).max())
        tri = int((r["triangulated"].astype(bool) != q["triangulated"]).sum())
        print(f"    rotation {rot:.4f} deg, translation {tdeg:.4f} deg, p3d {p3d:.2e}, triangulated flags {tri}")
        assert rot <= 4 * MEASURED["rot_deg"] and tdeg <= 4 * MEASURED["t_deg"] and p3d <= 4 * MEASURED["p3d"] and tri == MEASURED["triangulated"]
        # and the planted motion is what came out
        tt = c["t"] / np.linalg.norm(c["t"])
        assert np.degrees(np.arccos(np.clip((np.trace(Rr @ c["R"].T) - 1) / 2, -1, 1))) < 1.0 and np.degrees(np.arccos(np.clip(r["t21"] @ tt, -1, 1))) < 5.0


def test_sweep_counts_have_settled():
    """departure (a): every output at the kernels' sweep counts equals the one at those counts + 2, and the counts are where the outputs
    first settle (7, 8, 4, 4 for the 16 x 9, 8 x 9, 3 x 3 and 4 x 4 problems) plus two"""
    assert R.SWEEPS == {"H": 9, "F": 10, "S3": 6, "TRI": 6}
    more = {k: v + 2 for k, v in R.SWEEPS.items()}
    for kind in GENERATORS:
        for seed in SEEDS:
            c, r, _ = pair(kind, seed)
            r2 = R.run(c, sweeps=more)
            for k in R.OUT:
                assert np.array_equal(r[k], r2[k], equal_nan=True), (kind, seed, k)
    # two sweeps fewer than where they settle is too few somewhere
    c, r, _ = pair("general", 1)
    less = R.run(c, sweeps={"H": 5, "F": 6, "S3": 2, "TRI": 2})
    assert not all(np.array_equal(r[k], less[k], equal_nan=True) for k in R.OUT)


def test_draw_resolution():
    g = np.random.default_rng(9)
    for N in (8, 9, 10, 17, 300, 4096):
        draws = g.integers(0, 2 ** 31, (50, 8)).astype(np.int32)
        draws[0] = 0
        draws[1] = 2 ** 31 - 1
        draws[2] = [0, 2 ** 31 - 1] * 4
        lit = Q.random_int_sets(draws, N, 50)
        for h in range(50):
            got = R.resolve_draws(draws[h], N)
            assert got == lit[h] and len(set(got)) == 8 and all(0 <= v < N for v in got), (N, h)


@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(name):
    c, want = R.forced(name)
    r = R.run(c)
    st = r["stats"]
    got = (st[0], st[1], st[11], st[12])
    assert all(w is None or w == g for w, g in zip(want, got)), (name, want, got)
    if name == "identical_sets":
        assert st[3] == 0 and st[4] == 0 and r["scores"][0, 1] == r["scores"][1, 1] == r["scores"][3, 1]
    if name in ("s7", "index_out_of_range"):
        assert not r["scores"].any() and st[3] == st[4] == -1
    if name == "nan_keypoint":
        assert np.isnan(r["scores"][:5]).all() and st[3] == st[4] == -1
    if name == "h_success":
        assert r["triangulated"].sum() > 200 and r["p3d"][r["triangulated"] == 1][:, 2].min() > 0


def test_gates_at_their_bounds():
    """the strict comparisons: chi2 == bound is an inlier, its upper neighbour is not; cosParallax == fl32(0.99998) is below the double literal"""
    for model, th in ((0, R.TH_H), (1, R.TH_F)):
        M = np.eye(3, dtype=F32).reshape(-1) if model == 0 else np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F32)
        for e in np.arange(0.5, 4.0, 1.0 / 1024, dtype=F32):
            contrib, inl = R.check(model, M, [[0, 0, 0, e]])
            assert inl[0] == (e * e <= th)
    assert float(F32(0.99998)) < 0.99998 < float(R.COS_99998) and np.nextafter(F32(0.99998), F32(2)) == R.COS_99998


def test_exports_present():
    from rover_slam_amd import capi
    for sym in ("rfe_two_view", "rfe_two_view_dev", "rfe_k_two_view_check", "rfe_k_two_view_check_rt"):
        assert sym in capi.EXPORTS and getattr(capi.lib, sym)
    assert hasattr(capi.Context, "two_view") and hasattr(capi.Context, "two_view_dev")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_compiles_and_links(tmp_path):
    exe = DD.build(tmp_path, "two_view_driver")
    DD.run(exe)                                                            # without arguments: exit 0
    assert os.path.exists(exe)
