"""GPU: the drop-ins of include/rfe/triangulation.h (TriangulateMatches_rfe, CreateNewMapPoints_rfe) over mock keyframe classes
(tests/cpp/triangulation_driver.cpp) against the restatement tests/triangulation_ref.py: the returned list, matchsum and the statistics."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import triangulation_ref as T

pytestmark = pytest.mark.gpu
F32 = np.float32


def write_case(path, P, c, nleft=-1, desc=None):
    """a case as the driver reads it.  The baseline test is the monocular one: a neighbour that is to fail it stands in front of a scene a
    million metres deep.  mfScaleFactor is the float with 1.5f * mfScaleFactor == ratio_factor."""
    Nn, Kmax = c["pairs"].shape[:2]
    N1, N2max = len(c["kpts1"]), c["kpts2"].shape[1]
    scale = F32(P["ratio_factor"] / F32(1.5))
    assert F32(1.5) * scale == P["ratio_factor"]
    nv = np.ones((Nn,), np.uint8) if c.get("neighbour_valid") is None else c["neighbour_valid"]

    def keyframe(f, v, median, n, kp, raw, octave, ur, dep, mp):
        np.array([*v["rcw"].reshape(-1), *v["tcw"], *v["ow"], v["fx"], v["fy"], v["cx"], v["cy"], v["invfx"], v["invfy"], v["mb"], v["mbf"], median],
                 F32).tofile(f)
        np.array([n], np.int32).tofile(f)
        for a, dt in ((kp, F32), (kp if raw is None else raw, F32), (octave, np.int32), (ur, F32), (dep, F32), (mp, np.uint8)):
            np.ascontiguousarray(a, dt).tofile(f)
    with open(path, "wb") as f:
        np.array([Nn, N1, N2max, Kmax, P["nlevels"], 1, int(P["inertial"]), int(P["far_points"]), nleft, int(desc is not None)], np.int32).tofile(f)
        np.array([P["th_far"], scale], F32).tofile(f)
        P["scale_factors"].astype(F32).tofile(f); P["level_sigma2"].astype(F32).tofile(f)
        keyframe(f, c["view1"], 1.0, N1, c["kpts1"], c.get("kpts1_raw"), c["octave1"], c["uright1"], c["depth1"], c["has_mp1"])
        for n in range(Nn):
            raw = None if c.get("kpts2_raw") is None else c["kpts2_raw"][n]
            keyframe(f, c["views2"][n], 1.0 if nv[n] else 1e6, int(c["n2"][n]), c["kpts2"][n], raw, c["octave2"][n], c["uright2"][n], c["depth2"][n],
                     c["has_mp2"][n])
        c["S"].astype(np.int32).tofile(f); np.ascontiguousarray(c["pairs"], np.int32).tofile(f)
        if desc is not None:
            for d in desc:
                np.ascontiguousarray(d, F32).tofile(f)


def read_out(path, with_matches=False):
    raw = np.fromfile(path, np.uint8)
    ret, Nn, Kmax, npts = (int(v) for v in raw[:16].view(np.int32))
    o = 16
    out = {"ret": ret, "Kmax": Kmax, "matchsum": float(raw[o:o + 4].view(F32)[0])}; o += 4
    out["matches"] = raw[o:o + 4 * Nn].view(np.int32); o += 4 * Nn
    out["stats"] = raw[o:o + 32].view(np.int32); o += 32
    idx = raw[o:o + 16 * npts].view(np.int32).reshape(npts, 4); o += 16 * npts
    out["out_x3d"] = raw[o:o + 12 * npts].view(F32).reshape(npts, 3); o += 12 * npts
    out.update(out_n=idx[:, 0], out_idx1=idx[:, 1], out_idx2=idx[:, 2], out_stereo=idx[:, 3].astype(np.uint8))
    if with_matches and ret >= 0:
        out["S"] = raw[o:o + 4 * Nn].view(np.int32); o += 4 * Nn
        out["pairs"] = raw[o:o + 8 * Nn * Kmax].view(np.int32).reshape(Nn, Kmax, 2); o += 8 * Nn * Kmax
    assert o == len(raw)
    return out


def same(got, ref):
    assert got["ret"] == ref["created"] and np.array_equal(got["stats"], ref["stats"]), (got["ret"], got["stats"], ref["stats"])
    for k in ("out_n", "out_idx1", "out_idx2", "out_x3d", "out_stereo", "matches"):
        assert np.array_equal(got[k], ref[k], equal_nan=k == "out_x3d"), k
    assert got["matchsum"] == float(np.float32(ref["matches"].sum()))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_on_resident_matches(tmp_path):
    exe = DD.build(tmp_path, "triangulation_driver")
    for name, far, inertial in (("main", True, False), ("planted", True, True), ("posed", False, False)):
        P, c, ref = T.solved(name, far, inertial)
        write_case(str(tmp_path / "case.bin"), P, c)
        DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
        got = read_out(str(tmp_path / "out.bin"))
        assert ref["created"] > 5
        same(got, ref)
    # a two-camera neighbour is refused, nothing is computed
    write_case(str(tmp_path / "rig.bin"), P, c, nleft=200)
    DD.run(exe, str(tmp_path / "rig.bin"), str(tmp_path / "rig_out.bin"))
    got = read_out(str(tmp_path / "rig_out.bin"))
    assert got["ret"] == -1 and len(got["out_n"]) == 0 and (got["stats"] == 0).all()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_with_lightglue_in_front(tmp_path):
    """CreateNewMapPoints_rfe: LightGlue (synthetic weights) matches all neighbours in one call; whatever it matched, the list is the
    restatement's on those matches"""
    from rover_slam_amd import weights as Wt
    exe = DD.build(tmp_path, "triangulation_driver")
    P, c, _ = T.solved("posed", True, False)
    rng = np.random.default_rng(11)
    N1, Nn, N2max = len(c["kpts1"]), len(c["views2"]), c["kpts2"].shape[1]
    unit = lambda d: (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)   # noqa: E731
    d1 = unit(rng.standard_normal((N1, 256)))
    # a neighbour's feature carries the descriptor of the feature it is matched with in the case, plus noise
    d2 = unit(rng.standard_normal((Nn, N2max, 256)))
    for n in range(Nn):
        i, j = c["pairs"][n, :c["S"][n], 0], c["pairs"][n, :c["S"][n], 1]
        d2[n, j] = unit(d1[i] + 0.02 * rng.standard_normal((len(i), 256)))
    Wt.make_lightglue(seed=11).astype(F32).tofile(str(tmp_path / "lg.bin"))
    write_case(str(tmp_path / "case.bin"), P, c, desc=[d1] + list(d2))
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"), str(tmp_path / "lg.bin"))
    got = read_out(str(tmp_path / "out.bin"), with_matches=True)
    assert got["Kmax"] == min(N1, N2max) and got["S"].shape == (Nn,) and (got["S"] >= 0).all() and (got["S"] <= got["Kmax"]).all()
    print("LightGlue matches per neighbour:", got["S"].tolist(), "points:", got["ret"])
    assert got["S"].sum() > 100 and got["ret"] > 20                                # the synthetic weights do match these descriptors
    same(got, T.triangulate(P, dict(c, S=got["S"], pairs=got["pairs"])))
