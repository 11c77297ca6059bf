"""GPU: the drop-ins of include/rfe/pose_inertial_optimization.h (PoseInertialOptimizationLastKeyFrame_rfe / LastFrame_rfe) over mock
types (tests/cpp/pose_inertial_driver.cpp) against the restatement tests/pose_inertial_ref.py: the return value, the values handed to
SetImuPoseVelocity and mImuBias, mvbOutlier, the stored constraint, the freed previous constraint, and the two -1 cases."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import pose_inertial_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
KF, LF = R.MODE_LAST_KEYFRAME, R.MODE_LAST_FRAME
SENTINEL_OUTLIER = 1                      # mvbOutlier before the call: true everywhere, so a feature the call leaves alone shows


def write_case(path, c, camera2=False, prev_has_prior=True):
    P, a = c["P"], c["args"]
    N = len(a["has_mp"])
    prior = a["prior_in"] if a["prior_in"] is not None else np.full(R.PRIOR_DOUBLES, 7.0)
    with open(path, "wb") as f:
        np.array([N, P["nlevels"], a["mode"], a["rec_init"], int(camera2), int(prev_has_prior)], np.int32).tofile(f)
        np.array([P["fx"], P["fy"], P["cx"], P["cy"], P["bf"]], F32).tofile(f)
        np.asarray(P["inv_level_sigma2"], F32).tofile(f)
        for x, dt in ((a["cam"], F32), (a["state"], F32), (a["prev_state"], F32), (a["preint"], F32), (a["cov_rw"], F32), (prior, F64), (a["kpts"], F32),
                      (a["octave"], np.int32), (a["uright"], F32), (a["xw"], F32), (a["has_mp"], np.uint8), (a["track_depth"], F32),
                      (np.full(N, SENTINEL_OUTLIER, np.uint8), np.uint8)):
            np.ascontiguousarray(x, dt).tofile(f)


def read_out(path):
    raw = np.fromfile(path, np.uint8)
    ret, calls, N, prev_gone, has = (int(v) for v in raw[:20].view(np.int32))
    o = 20
    out = {"ret": ret, "set_calls": calls, "prev_gone": prev_gone, "has_constraint": has, "stats": raw[o:o + 64].view(np.int32)}
    o += 64
    out["pose_velocity"] = raw[o:o + 60].view(F32); o += 60
    out["bias"] = raw[o:o + 24].view(F32); o += 24
    out["stored"] = raw[o:o + 246 * 8].view(F64); o += 246 * 8
    out["converted"] = raw[o:o + 246 * 8].view(F64); o += 246 * 8
    out["outlier"] = raw[o:o + N]
    assert len(raw) == o + N
    return out


def run(exe, tmp_path, c, **kw):
    write_case(str(tmp_path / "case.bin"), c, **kw)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "pose_inertial_driver")
    for mode, kind, rec in ((KF, "mono", 0), (LF, "stereo", 0), (LF, "mixed", 0), (KF, "mixed", 1)):
        c = R.scene(90, 300, mode, kind)
        c["args"]["rec_init"] = rec
        ref = R.solve(c, outlier=np.full(300, SENTINEL_OUTLIER, np.uint8))
        got = run(exe, tmp_path, c)
        hm = c["args"]["has_mp"]
        assert got["ret"] == ref["ret"] > 150 and got["set_calls"] == 1 and np.array_equal(got["stats"], ref["stats"])
        # SetImuPoseVelocity(Rwb, twb, v) and IMU::Bias(bax, bay, baz, bwx, bwy, bwz) receive the float casts
        assert np.array_equal(got["pose_velocity"], ref["state_f32"][:15])
        assert np.array_equal(got["bias"], np.concatenate([ref["state_f32"][18:21], ref["state_f32"][15:18]]))
        assert np.array_equal(got["outlier"], ref["outlier"]) and (got["outlier"][hm == 0] == SENTINEL_OUTLIER).all() and (hm == 0).sum() > 10
        # the frame holds the new constraint, in the prior layout, and ToConstraintPoseImu hands the same numbers on
        assert got["has_constraint"] == 1 and np.array_equal(got["stored"], ref["prior_out"]) and np.array_equal(got["converted"], ref["prior_out"])
        # LastFrame frees the previous frame's constraint (Optimizer.cc:1618); LastKeyFrame does not look at it
        assert got["prev_gone"] == (1 if mode == LF else 0)
    # the two -1 cases: a second camera; LastFrame with a previous frame that has no constraint.  Nothing is touched
    for mode, kw in ((KF, {"camera2": True}), (LF, {"camera2": True}), (LF, {"prev_has_prior": False})):
        c = R.scene(91, 120, mode)
        got = run(exe, tmp_path, c, **kw)
        assert got["ret"] == -1 and got["set_calls"] == 0 and got["has_constraint"] == 0 and (got["stats"] == 0).all()
        assert np.array_equal(got["pose_velocity"], c["args"]["state"][:15])
        assert np.array_equal(got["bias"], np.concatenate([c["args"]["state"][18:21], c["args"]["state"][15:18]]))
        assert (got["outlier"] == SENTINEL_OUTLIER).all() and (got["stored"] == 0).all()
        assert got["prev_gone"] == (0 if kw.get("prev_has_prior", True) else 1)        # a constraint that was there is still there
    # a refusal by the library (a dT that is not positive) is not -1: -100 + RFE_ERR_INVALID, nothing touched, the previous constraint kept
    for mode in (KF, LF):
        c = R.scene(92, 60, mode)
        c["args"]["preint"][0] = 0.0
        got = run(exe, tmp_path, c)
        assert got["ret"] == -101 and got["set_calls"] == 0 and got["has_constraint"] == 0 and got["prev_gone"] == 0
        assert np.array_equal(got["pose_velocity"], c["args"]["state"][:15]) and (got["outlier"] == SENTINEL_OUTLIER).all()
