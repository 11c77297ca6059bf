"""GPU: the drop-in of include/rfe/two_view_reconstruction.h (TwoViewReconstruction_rfe) over mock KeyPoint / Point3f types
(tests/cpp/two_view_driver.cpp) against the restatement tests/two_view_ref.py: vMatches12 packed into the match list, the outputs sized
vKeys1.size(), the position of the random stream behind the call, and status() == -1 for what is not served."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import two_view_ref as R

pytestmark = pytest.mark.gpu
F32, I32 = np.float32, np.int32


def write_case(path, c, numbers, its):
    P = c["P"]
    n1, n2 = P["n1"], P["n2"]
    m12 = np.full(n1, -1, I32)
    m12[c["pairs"][:c["S"], 0]] = c["pairs"][:c["S"], 1]
    with open(path, "wb") as f:
        np.array([n1, n2, its, len(numbers)], I32).tofile(f)
        np.array([P["fx"], P["fy"], P["cx"], P["cy"], P["sigma"], P["rh_threshold"]], F32).tofile(f)
        np.ascontiguousarray(c["kpts1"][:n1], F32).tofile(f)
        np.ascontiguousarray(c["kpts2"][:n2], F32).tofile(f)
        m12.tofile(f)
        np.ascontiguousarray(numbers, I32).tofile(f)


def read_out(path):
    raw = np.fromfile(path, np.uint8)
    hd = raw[:24].view(I32)
    o = dict(zip(("ret", "status", "model", "taken", "n_p3d", "n_tri"), (int(v) for v in hd)))
    o["stats"] = raw[24:88].view(I32)
    f = raw[88:88 + 48].view(F32)
    o["R21"], o["t21"] = f[:9], f[9:12]
    at = 136
    o["p3d"] = raw[at:at + 12 * o["n_p3d"]].view(F32).reshape(-1, 3)
    o["triangulated"] = raw[at + 12 * o["n_p3d"]:]
    assert len(o["triangulated"]) == o["n_tri"]
    return o


def run(exe, tmp_path, c, its, spare=5):
    numbers = np.concatenate([np.asarray(c["draws"][:its], I32).reshape(-1), np.arange(spare, dtype=I32)])
    write_case(str(tmp_path / "case.bin"), c, numbers, its)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    return read_out(str(tmp_path / "out.bin"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in(tmp_path):
    exe = DD.build(tmp_path, "two_view_driver")
    for kind, ret, model in (("general", 1, 2), ("plane", 1, 1), ("rotation", 0, 2)):
        c = R.scene(21, kind=kind, its=60, sigma=1.0)
        ref = R.run(c)
        got = run(exe, tmp_path, c, 60)
        n1 = c["P"]["n1"]
        assert (got["ret"], got["status"], got["model"]) == (ret, 0, model) == (ref["stats"][0], 0, ref["stats"][1])
        assert got["taken"] == 8 * 60                                      # the stream stands where the reference's would
        assert np.array_equal(got["stats"], ref["stats"]) and got["n_p3d"] == got["n_tri"] == n1
        assert np.array_equal(got["p3d"], ref["p3d"][:n1]) and np.array_equal(got["triangulated"], ref["triangulated"][:n1])
        if ret:
            assert np.array_equal(got["R21"], ref["R21"]) and np.array_equal(got["t21"], ref["t21"]) and got["triangulated"].sum() > 200
        else:
            assert (got["R21"] == -2).all() and (got["t21"] == -2).all() and not got["triangulated"].any()
    # fewer than 8 matches: false, the draws still taken
    c = R.scene(22, n=5, its=4, sigma=1.0)
    got = run(exe, tmp_path, c, 4)
    assert (got["ret"], got["status"], got["taken"]) == (0, 0, 32) and got["stats"][12] == R.FLAG_FEW
    # more than 1024 iterations: not served, nothing drawn, nothing touched
    got = run(exe, tmp_path, c, 1025)
    assert (got["ret"], got["status"], got["taken"], got["n_p3d"], got["n_tri"]) == (0, -1, 0, 3, 5) and (got["R21"] == -2).all()
    # more than 4096 keypoints
    big = R.scene(23, n=20, its=4, extra1=4080, extra2=3)
    got = run(exe, tmp_path, big, 4)
    assert big["P"]["n1"] == 4100 and (got["ret"], got["status"], got["taken"], got["n_p3d"]) == (0, -1, 0, 3)
