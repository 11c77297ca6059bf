"""GPU: LocalMapping::CreateNewMapPoints behind the matcher on the device (rfe_triangulate_neighbours / _dev) against the contract of
DESIGN.md 6g restated in tests/triangulation_ref.py.  Every comparison is exact (np.array_equal on every output array), in host and device
form."""
import ctypes

import numpy as np
import pytest

import triangulation_ref as T
from triangulation_ref import solved, to_capi, view_to_capi

pytestmark = pytest.mark.gpu
OUT = {"code": np.int32, "x3d": np.float32, "point_stereo": np.uint8, "out_n": np.int32, "out_idx1": np.int32, "out_idx2": np.int32,
       "out_x3d": np.float32, "out_stereo": np.uint8, "matches": np.int32}
assert tuple(OUT) == T.KEYS


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def same(got, ref, keys=T.KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=k in ("x3d", "out_x3d")), (k, np.argwhere(got[k] != ref[k])[:8])
    assert got["created"] == ref["created"] and np.array_equal(got["stats"], ref["stats"]), (got["stats"], ref["stats"])


def host(ctx, P, c, outputs=T.KEYS, **kw):
    a = dict(kpts1_raw=c.get("kpts1_raw"), kpts2_raw=c.get("kpts2_raw"), neighbour_valid=c.get("neighbour_valid"))
    a.update(kw)
    return ctx.triangulate_neighbours(to_capi(P), view_to_capi(c["view1"]), c["kpts1"], c["octave1"], c["uright1"], c["depth1"], c["has_mp1"],
                                      [view_to_capi(v) for v in c["views2"]], c["kpts2"], c["octave2"], c["uright2"], c["depth2"], c["has_mp2"],
                                      c["n2"], c["S"], c["pairs"], outputs=outputs, **a)


def dev(ctx, P, c, outputs=T.KEYS):
    """rfe_triangulate_neighbours_dev on uploaded copies of the host arrays; returns the host form's dict"""
    from rover_slam_amd import capi
    Nn, Kmax = c["pairs"].shape[:2]
    N1, N2max = len(c["kpts1"]), c["kpts2"].shape[1]
    bufs = []

    def up(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        bufs.append(ctx.alloc(max(a.nbytes, 4)))
        return bufs[-1].upload(a) if a.nbytes else bufs[-1]
    views = (capi.TriView * max(Nn, 1))(*[view_to_capi(v) for v in c["views2"]])
    shape = {"code": (Nn, Kmax), "x3d": (Nn, Kmax, 3), "point_stereo": (Nn, Kmax), "out_n": (N1,), "out_idx1": (N1,), "out_idx2": (N1,),
             "out_x3d": (N1, 3), "out_stereo": (N1,), "matches": (Nn,)}
    out = {k: ctx.alloc(max(int(np.prod(shape[k])) * np.dtype(OUT[k]).itemsize, 4)) for k in outputs}
    out["stats"] = ctx.alloc(32).upload(np.full((8,), 77, np.int32))               # the call clears it
    try:
        ctx.triangulate_neighbours_dev(to_capi(P), view_to_capi(c["view1"]), up(c["kpts1"], np.float32), up(c["octave1"], np.int32),
                                       up(c["uright1"], np.float32), up(c["depth1"], np.float32), up(c["has_mp1"], np.uint8), N1,
                                       up(np.frombuffer(bytes(views), np.uint8), np.uint8), up(c["kpts2"], np.float32), up(c["octave2"], np.int32),
                                       up(c["uright2"], np.float32), up(c["depth2"], np.float32), up(c["has_mp2"], np.uint8), up(c["n2"], np.int32),
                                       Nn, N2max, up(c["S"], np.int32), up(c["pairs"], np.int32), Kmax, out["stats"],
                                       kpts1_raw=up(c.get("kpts1_raw"), np.float32), kpts2_raw=up(c.get("kpts2_raw"), np.float32),
                                       neighbour_valid=up(c.get("neighbour_valid"), np.uint8), **{k: out[k] for k in outputs})
        ctx.synchronize()
        r = {k: out[k].download(shape[k], OUT[k]) if np.prod(shape[k]) else np.zeros(shape[k], OUT[k]) for k in outputs}
        r["stats"] = out["stats"].download((8,), np.int32)
        r["created"] = int(r["stats"][0])
        for k in ("out_n", "out_idx1", "out_idx2", "out_x3d", "out_stereo"):
            if k in r:
                r[k] = r[k][:r["created"]]
        return r
    finally:
        for b in bufs + list(out.values()):
            b.free()


# ---------------------------------------------------------------- 1. the main case: far points and the inertial bound on and off
@pytest.mark.parametrize("inertial", (False, True))
@pytest.mark.parametrize("far_points", (True, False))
def test_main_case(ctx, far_points, inertial):
    P, c, ref = solved("main", far_points, inertial)
    assert c["pairs"].shape == (5, 1100, 2) and list(c["S"]) == [1100, 640, 0, 1, 257] and list(c["n2"]) == [1100, 900, 1100, 1, 700]
    assert ref["created"] > 500 and (ref["code"] == T.CLAIMED).sum() >= 100 and (c["neighbour_valid"] == 0).sum() == 1
    h = host(ctx, P, c)
    same(h, ref)
    d = dev(ctx, P, c)
    same(d, ref)
    print(f"far_points {far_points}, inertial {inertial}: stats {h['stats'].tolist()}, codes {np.bincount(h['code'][h['code'] >= 0], minlength=17).tolist()}")


def test_a_current_keyframe_that_is_not_the_world_frame(ctx):
    P, c, ref = solved("posed", True, False)
    assert ref["created"] > 200 and c["neighbour_valid"].all()
    same(host(ctx, P, c), ref)
    same(dev(ctx, P, c), ref)
    # neighbour_valid = NULL is "all valid"
    same(host(ctx, P, c, neighbour_valid=None), ref)


# ---------------------------------------------------------------- 2. the planted slots
@pytest.mark.parametrize("inertial", (False, True))
@pytest.mark.parametrize("far_points", (True, False))
def test_planted_case(ctx, far_points, inertial):
    base, c, expect = T.planted_case()
    P = T.P(base, far_points, inertial)
    ref = T.triangulate(P, c)
    h = host(ctx, P, c)
    same(h, ref)
    same(dev(ctx, P, c), ref)
    for name, (n, k, code, code_in) in expect.items():
        want = code_in if inertial else code
        if name == "far_at" and not far_points:
            want = 0
        assert h["code"][n, k] == want, (name, h["code"][n, k], want)
    assert h["stats"][5] == 1                                                      # the NaN point is created, and counted
    n, k = expect["nan_point"][:2]
    assert np.isnan(h["x3d"][n, k]).all() and np.isnan(h["out_x3d"]).any(1).sum() == 1
    n, k = expect["both_stereo"][:2]
    assert list(h["x3d"][n, k]) == [0, 0, 8] and h["point_stereo"][n, k] == 1     # from the current keyframe's depth, not the neighbour's
    n, k = expect["z1_minus_zero"][:2]
    assert h["x3d"][n, k][2] == 0 and np.signbit(h["x3d"][n, k][2]) and list(h["x3d"][n, k][:2]) == [-1, -4]
    n, k = expect["z1_zero"][:2]
    assert list(h["x3d"][n, k]) == [-1, -1, 0] and not np.signbit(h["x3d"][n, k][2])
    n, k = expect["claim0"][:2]
    assert h["out_n"][0] == 0 and h["out_idx1"][0] == c["pairs"][n, k, 0]        # neighbour 0 takes the feature neighbours 1 and 2 pass too
    # without the raw keypoints the undistorted ones are unprojected: the planted reprojection errors move into the points
    nr = dict(c, kpts1_raw=None, kpts2_raw=None)
    same(host(ctx, P, nr), T.triangulate(P, nr))


# ---------------------------------------------------------------- 3. other shapes
def test_no_neighbours_and_empty_sides(ctx):
    P, c, _ = solved("posed", True, False)
    per = ("views2", "kpts2", "octave2", "uright2", "depth2", "has_mp2", "n2", "neighbour_valid", "S", "pairs", "kpts2_raw")
    none = {k: (v[:0] if k in per and v is not None else v) for k, v in c.items()}
    ref = T.triangulate(P, none)
    assert ref["created"] == 0 and ref["code"].shape == (0, 320)
    same(host(ctx, P, none), ref)
    same(dev(ctx, P, none), ref)
    nok = dict(c, pairs=c["pairs"][:, :0])                                         # Kmax = 0: S is clamped to it
    ref = T.triangulate(P, nok)
    assert list(ref["matches"]) == [0, 0, 0] and ref["stats"][1] == 0
    same(host(ctx, P, nok), ref)
    same(dev(ctx, P, nok), ref)
    nof = dict(c, kpts1=c["kpts1"][:0], octave1=c["octave1"][:0], uright1=c["uright1"][:0], depth1=c["depth1"][:0], has_mp1=c["has_mp1"][:0])
    ref = T.triangulate(P, nof)                                                    # N1 = 0: every index is out of range
    assert ((ref["code"] == 2) | (ref["code"] == T.NO_SLOT)).all() and ref["stats"][1] == 900
    same(host(ctx, P, nof), ref)
    same(dev(ctx, P, nof), ref)


def test_every_slot_rejected(ctx):
    P, c, _ = solved("main", True, False)
    for other in (dict(has_mp1=np.ones_like(c["has_mp1"])), dict(neighbour_valid=np.zeros_like(c["neighbour_valid"]))):
        nobody = dict(c, **other)
        ref = T.triangulate(P, nobody)
        assert ref["created"] == 0 and len(ref["out_n"]) == 0
        same(host(ctx, P, nobody), ref)
        same(dev(ctx, P, nobody), ref)
        assert set(np.unique(ref["code"])) <= {T.NO_SLOT, 1, 2, 3}


def test_every_optional_output_null(ctx):
    P, c, ref = solved("main", True, False)
    h = host(ctx, P, c, outputs=())
    assert h["created"] == ref["created"] and np.array_equal(h["stats"], ref["stats"]) and set(h) == {"created", "stats"}
    d = dev(ctx, P, c, outputs=())
    assert np.array_equal(d["stats"], ref["stats"])
    for keys in (("out_x3d",), ("code", "matches"), ("x3d", "out_idx1", "out_stereo")):
        same(host(ctx, P, c, outputs=keys), ref, keys)
        same(dev(ctx, P, c, outputs=keys), ref, keys)


def test_one_ctx_across_cases_is_bit_for_bit():
    from rover_slam_amd import capi
    c0 = capi.Context(0)
    try:
        first = None
        for name in ("main", "planted", "main"):
            P, c, ref = solved(name, True, False)
            got = host(c0, P, c)
            same(got, ref)
            if first is None:
                first = got
        for k in T.KEYS + ("stats",):
            assert np.array_equal(got[k], first[k], equal_nan=True), k
    finally:
        c0.close()


# ---------------------------------------------------------------- 4. refusals and profile stages
def test_refusals(ctx):
    from rover_slam_amd import capi
    P, c, ref = solved("posed", True, False)

    def refused(msg, fn):
        with pytest.raises(capi.RfeError) as ex:
            fn()
        assert "error -1" in str(ex.value) and msg in str(ex.value), str(ex.value)
    nan, inf = np.float32(np.nan), np.float32(np.inf)

    def with_view1(**kw):
        return host(ctx, P, dict(c, view1=dict(c["view1"], **kw)))

    def with_view2(n, **kw):
        return host(ctx, P, dict(c, views2=[dict(v, **kw) if m == n else v for m, v in enumerate(c["views2"])]))

    def with_params(**kw):
        p = to_capi(P)
        for k, v in kw.items():
            if k in ("scale_factors", "level_sigma2"):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return ctx.triangulate_neighbours(p, view_to_capi(c["view1"]), c["kpts1"], c["octave1"], c["uright1"], c["depth1"], c["has_mp1"],
                                          [view_to_capi(v) for v in c["views2"]], c["kpts2"], c["octave2"], c["uright2"], c["depth2"],
                                          c["has_mp2"], c["n2"], c["S"], c["pairs"], neighbour_valid=c["neighbour_valid"])
    refused("nlevels", lambda: with_params(nlevels=0))
    refused("nlevels", lambda: with_params(nlevels=17))
    refused("non-finite", lambda: with_params(th_far=nan))
    refused("non-finite", lambda: with_params(ratio_factor=inf))
    refused("non-finite", lambda: with_params(scale_factors=(3, nan)))
    refused("non-finite", lambda: with_params(level_sigma2=(7, inf)))
    same(with_params(scale_factors=(12, nan)), ref)                                # behind nlevels = 8: not looked at
    refused("non-finite", lambda: with_view1(tcw=np.array([0, inf, 0], np.float32)))
    refused("non-finite", lambda: with_view1(rcw=np.where(np.eye(3) > 0, nan, 0).astype(np.float32)))
    refused("non-finite", lambda: with_view1(ow=np.array([nan, 0, 0], np.float32)))
    for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf"):
        refused("non-finite", lambda: with_view1(**{k: inf}))
        refused("non-finite", lambda: with_view2(2, **{k: nan}))
    refused("non-finite", lambda: with_view2(1, tcw=np.array([nan, 0, 0], np.float32)))
    # sizes and required pointers, both forms: refused before a pointer is touched
    lib, h = capi.lib, ctx.h
    o = np.zeros((64,), np.float32).ctypes.data
    p0, v0 = to_capi(P), view_to_capi(c["view1"])

    def raw(fn, p=p0, v=v0, k1=o, N1=4, v2=o, k2=o, n2=o, Nn=2, N2max=4, S=o, pairs=o, Kmax=4, st=o, mp2=o):
        return fn(h, ctypes.byref(p) if p else None, ctypes.byref(v) if v else None, k1, None, o, o, o, o, N1, v2, k2, None, o, o, o, mp2, n2, None, Nn,
                  N2max, S, pairs, Kmax, None, None, None, None, None, None, None, None, None, st)
    bad_levels = to_capi(P, nlevels=0)
    for fn in (lib.rfe_triangulate_neighbours, lib.rfe_triangulate_neighbours_dev):
        for kw, msg in ((dict(Nn=-1), "Nn"), (dict(Nn=65), "Nn"), (dict(N1=-1), "N1"), (dict(N1=4097), "N1"), (dict(N2max=-1), "N2max"),
                        (dict(N2max=4097), "N2max"), (dict(Kmax=-1), "Kmax"), (dict(Kmax=4097), "Kmax"), (dict(p=bad_levels), "nlevels"),
                        (dict(p=0), "null"), (dict(v=0), "null"), (dict(k1=None), "null"), (dict(v2=None), "null"), (dict(k2=None), "null"),
                        (dict(n2=None), "null"), (dict(S=None), "null"), (dict(pairs=None), "null"), (dict(st=None), "null"),
                        (dict(mp2=None), "null")):
            assert raw(fn, **kw) == -1 and msg in lib.rfe_last_error(h).decode(), (kw, lib.rfe_last_error(h).decode())
    same(host(ctx, P, c), ref)                                                     # the ctx is still usable


def test_profile_names_both_stages(ctx):
    P, c, _ = solved("main", True, False)
    ctx.profile(True); ctx.profile_reset()
    try:
        host(ctx, P, c)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False); ctx.profile_reset()
    for name in ("tri_eval", "tri_resolve"):
        assert name in prof and prof[name][1] >= 1 and prof[name][0] > 0, prof
