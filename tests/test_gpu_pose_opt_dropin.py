"""GPU: the drop-in of include/rfe/pose_optimization.h (PoseOptimization_rfe) over a mock Frame (tests/cpp/pose_opt_driver.cpp) against the
restatement tests/pose_opt_ref.py: the return value, mvbOutlier and the pose handed to SetPose."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import pose_opt_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL_OUTLIER = 1                      # mvbOutlier before the call: true everywhere, so a feature the call leaves alone shows


def write_case(path, c, camera2=False):
    P, N = c["P"], len(c["kpts"])
    with open(path, "wb") as f:
        np.array([N, P["nlevels"], int(camera2)], np.int32).tofile(f)
        np.array([P["fx"], P["fy"], P["cx"], P["cy"], P["bf"]], F32).tofile(f)
        np.asarray(P["inv_level_sigma2"], F32).tofile(f)
        for a, dt in ((c["pose0"], F32), (c["kpts"], F32), (c["octave"], np.int32), (c["uright"], F32), (c["xw"], F32), (c["has_mp"], np.uint8),
                      (np.full(N, SENTINEL_OUTLIER, np.uint8), np.uint8)):
            np.ascontiguousarray(a, dt).tofile(f)


def read_out(path):
    raw = np.fromfile(path, np.uint8)
    ret, calls, N = (int(v) for v in raw[:12].view(np.int32))
    out = {"ret": ret, "set_pose_calls": calls, "stats": raw[12:44].view(np.int32), "pose": raw[44:72].view(F32), "outlier": raw[72:72 + N]}
    assert len(raw) == 72 + N
    return out


def run(exe, tmp_path, c, **kw):
    write_case(str(tmp_path / "case.bin"), c, **kw)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "pose_opt_driver")
    for kind in ("mono", "stereo", "mixed"):
        c = R.scene(90, 500, kind)
        ref = R.solve(c, outlier=np.full(500, SENTINEL_OUTLIER, np.uint8))
        got = run(exe, tmp_path, c)
        assert got["ret"] == ref["ret"] > 250 and got["set_pose_calls"] == 1 and np.array_equal(got["stats"], ref["stats"])
        assert np.array_equal(got["pose"], ref["pose_f32"]) and np.array_equal(got["outlier"], ref["outlier"])
        assert (got["outlier"][c["has_mp"] == 0] == SENTINEL_OUTLIER).all() and (c["has_mp"] == 0).sum() > 20
    # below three correspondences: 0, the flags cleared, SetPose not called
    c = R.forced("two")
    got = run(exe, tmp_path, c)
    assert got["ret"] == 0 and got["set_pose_calls"] == 0 and np.array_equal(got["pose"], c["pose0"]) and (got["outlier"] == 0).all()
    # a frame with a second camera is refused, nothing is touched
    c = R.scene(90, 500, "mixed")
    got = run(exe, tmp_path, c, camera2=True)
    assert got["ret"] == -1 and got["set_pose_calls"] == 0 and np.array_equal(got["pose"], c["pose0"])
    assert (got["outlier"] == SENTINEL_OUTLIER).all() and (got["stats"] == 0).all()
