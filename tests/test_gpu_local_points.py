"""GPU: steps 2 and 3 of Tracking::SearchLocalPoints on the device (rfe_search_local_points / _dev, SearchLocalPoints_rfe) against the
contract of DESIGN.md 6f restated in tests/local_points_ref.py.  Every comparison is exact (np.array_equal on every output array), in host
and device form."""
import ctypes
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import local_points_ref as LP
from local_points_ref import LEVEL_PREDICTED, LEVEL_ZERO, read_driver_out, solved, to_capi, write_driver_case

pytestmark = pytest.mark.gpu
OUT = {"assign": np.int32, "best_idx": np.int32, "best_dist": np.float32, "second_dist": np.float32, "proj": np.float32, "proj_xr": np.float32,
       "depth": np.float32, "view_cos": np.float32, "level": np.int32, "reject": np.int32}
assert tuple(OUT) == LP.KEYS


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def same(got, ref, keys=LP.KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(1))[:8])
    assert got["nmatches"] == ref["nmatches"]


def check_stats(st, ref):
    assert list(st[[0, 1, 3, 4, 5]]) == [ref["nmatches"], ref["candidates"], 0, ref["in_frustum"], ref["searched"]] and st[2] >= 1, st
    assert (st[6:] == 0).all(), st


def host(ctx, P, c, **kw):
    a = dict(valid=c.get("valid"), observed=c.get("observed"), kpts=c["kpts"], octave=c.get("octave"), skip=c.get("skip"))
    a.update(kw)
    return ctx.search_local_points(to_capi(P), c["q"], c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["desc"], **a)


def dev(ctx, P, c, cand_cap, outputs=LP.KEYS, kxy=False, nf_dev=None):
    """rfe_search_local_points_dev on uploaded copies of the host arrays; returns the host form's dict"""
    Np, Nf = len(c["pw"]), len(c["desc"])
    bufs = []

    def up(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        bufs.append(ctx.alloc(max(a.nbytes, 4)))
        return bufs[-1].upload(a) if a.nbytes else bufs[-1]
    shape = {k: (Nf,) if k == "assign" else ((Np, 2) if k == "proj" else (Np,)) for k in OUT}
    out = {k: ctx.alloc(max(int(np.prod(shape[k])), 1) * 4) for k in outputs}
    out["stats"] = ctx.alloc(32).upload(np.full((8,), 77, np.int32))               # the call clears the words it adds to
    pos = dict(kxy=up(c["kxy"], np.int32)) if kxy else dict(kpts=up(c["kpts"], np.float32))
    try:
        ctx.search_local_points_dev(to_capi(P), up(c["q"], np.float32), up(c["pw"], np.float32), up(c["normal"], np.float32),
                                    up(c["min_dist"], np.float32), up(c["max_dist"], np.float32), up(c["scale_dist"], np.float32), Np,
                                    up(c["desc"], np.float32), Nf, cand_cap, out["assign"], out["stats"], valid=up(c.get("valid"), np.uint8),
                                    observed=up(c.get("observed"), np.uint8), octave=up(c.get("octave"), np.int32), skip=up(c.get("skip"), np.uint8),
                                    nf_dev=up(None if nf_dev is None else np.array([nf_dev], np.int32), np.int32),
                                    **pos, **{k: out[k] for k in outputs if k != "assign"})
        ctx.synchronize()
        r = {k: out[k].download(shape[k], OUT[k]) if np.prod(shape[k]) else np.zeros(shape[k], OUT[k]) for k in outputs}
        r["stats"] = out["stats"].download((8,), np.int32)
        r["nmatches"] = int(r["stats"][0])
        return r
    finally:
        for b in bufs + list(out.values()):
            b.free()


# ---------------------------------------------------------------- 1. the main case: th, far points, level mode, one and eight levels
@pytest.mark.parametrize("level_mode", (LEVEL_ZERO, LEVEL_PREDICTED))
@pytest.mark.parametrize("far_points", (True, False))
@pytest.mark.parametrize("th", (1, 6))
@pytest.mark.parametrize("name", ("main", "main8"))
def test_main_case(ctx, oracle, name, th, far_points, level_mode):
    P, c, ref = solved(oracle, name, th, far_points, level_mode)
    assert ref["searched"] > 700 and ref["nmatches"] > 20
    h = host(ctx, P, c)
    same(h, ref)
    check_stats(h["stats"], ref)
    d = dev(ctx, P, c, ref["candidates"])                                          # exactly the slots the lists need
    same(d, ref)
    assert np.array_equal(d["stats"], h["stats"])
    print(f"{name}, th {th}, far_points {far_points}, level_mode {level_mode}: stats {list(h['stats'])}")


def test_device_form_with_integer_positions_and_a_device_count(ctx, oracle):
    """kxy instead of kpts, and *nf_dev = Nf - 100: the last 100 rows are no features"""
    P, c, _ = solved(oracle, "main8", 6, True, LEVEL_PREDICTED)
    nf = len(c["desc"]) - 100
    ref = LP.search(oracle, P, c, nf=nf, kxy=True)
    assert ref["nmatches"] > 100 and (ref["assign"][nf:] == -1).all() and (c["kxy"] != c["kpts"]).any()
    d = dev(ctx, P, c, ref["candidates"] + 50, kxy=True, nf_dev=nf)
    same(d, ref)
    check_stats(d["stats"], ref)


# ---------------------------------------------------------------- 2. the planted points
@pytest.mark.parametrize("level_mode", (LEVEL_ZERO, LEVEL_PREDICTED))
def test_planted_case(ctx, oracle, level_mode):
    P, c, ref = solved(oracle, "planted", 1, True, level_mode)
    h = host(ctx, P, c)
    same(h, ref)
    check_stats(h["stats"], ref)
    assert list(h["reject"]) == [code for _, code in LP.PLANTED_POINTS] and list(h["assign"]) == list(LP.PLANTED_ASSIGN)
    assert h["nmatches"] == LP.PLANTED_NMATCHES
    # fl32(0.998) is above the double literal 0.998: radius 2.5, feature 0 out of reach; its lower neighbour gets radius 4 and the feature
    assert h["view_cos"][13] == np.float32(0.998) and h["best_idx"][13] == -1 and h["best_idx"][14] == 0 and h["assign"][0] == 14
    assert h["reject"][6] == 0 and np.isnan(h["proj"][6]).all() and h["best_idx"][6] == -1                  # the NaN point: searched, no candidates
    d = dev(ctx, P, c, ref["candidates"])
    same(d, ref)
    assert np.array_equal(d["stats"], h["stats"])
    # valid = NULL: every point is valid, and the would-be winner takes its feature; observed = NULL: point 19 blocks feature 4
    v = LP.search(oracle, P, c, valid=np.ones(len(c["pw"]), np.uint8))
    same(host(ctx, P, c, valid=None), v)
    assert v["assign"][2] == 17 and v["assign"][3] == 18
    ob = LP.search(oracle, P, dict(c, observed=None))
    same(host(ctx, P, c, observed=None), ob)
    assert ob["assign"][4] == 19 and ob["assign"][5] == 20
    off = LP.search(oracle, LP.P(LP.case_of("planted")[0], 1, False, level_mode), c)
    got = host(ctx, dict(P, far_points=False), c)
    same(got, off)
    assert got["reject"][16] == 0 and got["stats"][4] == got["stats"][5] == ref["in_frustum"]


# ---------------------------------------------------------------- 3. other shapes
def test_no_map_points_and_no_features(ctx, oracle):
    P, c, ref = solved(oracle, "main", 6, True, LEVEL_ZERO)
    per_point = ("q", "pw", "normal", "min_dist", "max_dist", "scale_dist", "valid", "observed")
    none = {k: (v[:0] if k in per_point else v) for k, v in c.items()}
    e = host(ctx, P, none)
    assert e["nmatches"] == 0 and len(e["assign"]) == len(c["kpts"]) and (e["assign"] == -1).all()
    assert all(len(e[k]) == 0 for k in LP.KEYS if k != "assign") and list(e["stats"][[0, 1, 3, 4, 5]]) == [0, 0, 0, 0, 0]
    d = dev(ctx, P, none, 16)
    assert (d["assign"] == -1).all() and list(d["stats"][[0, 1, 3, 4, 5]]) == [0, 0, 0, 0, 0] and (d["stats"][6:] == 0).all()
    nof = dict(c, kpts=c["kpts"][:0], kxy=c["kxy"][:0], desc=c["desc"][:0], skip=c["skip"][:0])
    e = host(ctx, P, nof)
    same(e, dict(ref, assign=ref["assign"][:0], best_idx=np.full_like(ref["best_idx"], -1), best_dist=np.full_like(ref["best_dist"], 256),
                 second_dist=np.full_like(ref["second_dist"], 256), nmatches=0))
    assert e["stats"][4] == ref["in_frustum"] and e["stats"][5] == ref["searched"] and e["stats"][1] == 0


def test_every_point_rejected(ctx, oracle):
    P, c, _ = solved(oracle, "main", 6, True, LEVEL_ZERO)
    nobody = dict(c, valid=np.zeros_like(c["valid"]))
    ref = LP.search(oracle, P, nobody)
    assert (ref["reject"] == 1).all() and ref["candidates"] == 0
    h = host(ctx, P, nobody)
    same(h, ref)
    check_stats(h["stats"], ref)
    assert (h["assign"] == -1).all() and (h["proj"] == 0).all() and (h["level"] == -1).all()
    behind = dict(P, rcw=(P["rcw"] * np.array([[-1], [1], [-1]], np.float32)).astype(np.float32))      # half a turn about the camera's y axis
    ref = LP.search(oracle, behind, c)
    assert (ref["reject"] == 2).sum() > 1500
    h = host(ctx, behind, c)
    same(h, ref)
    assert (h["proj"][ref["reject"] == 2] == -1).all()


def test_overflow_is_reported_and_harmless(ctx, oracle):
    P, c, ref = solved(oracle, "main", 6, True, LEVEL_ZERO)
    o = dev(ctx, P, c, ref["candidates"] - 1)                                      # one slot short
    assert list(o["stats"]) == [0, ref["candidates"], o["stats"][2], 1, ref["in_frustum"], ref["searched"], 0, 0]
    assert (o["assign"] == -1).all() and (o["best_idx"] == -1).all() and (o["best_dist"] == 256).all() and (o["second_dist"] == 256).all()
    for k in ("proj", "proj_xr", "depth", "view_cos", "level", "reject"):         # the front does not depend on the slots
        assert np.array_equal(o[k], ref[k]), k
    # only the required outputs
    m = dev(ctx, P, c, ref["candidates"], outputs=("assign",))
    assert np.array_equal(m["assign"], ref["assign"]) and m["stats"][3] == 0 and m["stats"][0] == ref["nmatches"]


def test_one_ctx_across_cases_is_bit_for_bit(oracle):
    from rover_slam_amd import capi
    c0 = capi.Context(0)
    try:
        first = None
        for name, th in (("main", 6), ("planted", 1), ("main", 6)):
            P, c, ref = solved(oracle, name, th, True, LEVEL_ZERO)
            got = host(c0, P, c)
            same(got, ref)
            check_stats(got["stats"], ref)
            if first is None:
                first = got
        for k in LP.KEYS + ("stats",):
            assert np.array_equal(got[k], first[k]), k
    finally:
        c0.close()


def test_host_form_takes_its_second_attempt(oracle):
    """A fresh ctx has ps_cap = 0, so the host form first runs with 16 slots per map point.  At th = 20 the lists of 64 points over 300
    features need more than twice that: the first attempt overflows, the second runs with exactly stats[1] slots.  The second call on
    the same ctx starts from the remembered slot count and gives the same bits in one attempt."""
    from rover_slam_amd import capi
    base, c = LP.make_case(0, W=160, H=120, Nf=300, Np=64)
    P = LP.P(base, 20, True, LEVEL_ZERO)
    ref = LP.search(oracle, P, c)
    Np, Nf = len(c["pw"]), len(c["desc"])
    print(f"candidates {ref['candidates']}, first guess {16 * Np}, ceiling {Np * Nf}, nmatches {ref['nmatches']}")
    assert 16 * Np < ref["candidates"] <= Np * Nf
    c0 = capi.Context(0)
    try:
        first = host(c0, P, c)
        same(first, ref)
        check_stats(first["stats"], ref)
        assert first["stats"][1] == ref["candidates"] and first["stats"][3] == 0 and first["stats"][0] == ref["nmatches"]
        again = host(c0, P, c)
        for k in LP.KEYS + ("stats",):
            assert np.array_equal(again[k], first[k], equal_nan=True), k
        assert again["nmatches"] == first["nmatches"]
    finally:
        c0.close()


# ---------------------------------------------------------------- 4. refusals and profile stages
def test_refusals(ctx, oracle):
    from rover_slam_amd import capi
    P, c, ref = solved(oracle, "planted", 1, True, LEVEL_ZERO)

    def refused(msg, fn):
        with pytest.raises(capi.RfeError) as ex:
            fn()
        assert "error -1" in str(ex.value) and msg in str(ex.value), str(ex.value)
    lv = lambda n, lsf=0.2: dict(P, nlevels=n, scale_factors=np.ones(min(max(n, 1), 16), np.float32), log_scale_factor=np.float32(lsf))   # noqa: E731

    def call(Pm, nlevels=None, th_high=1.4, **kw):
        p = to_capi(Pm)
        if nlevels is not None:
            p.nlevels = nlevels
        a = dict(valid=c["valid"], observed=c["observed"], kpts=c["kpts"], skip=c["skip"])
        a.update(kw)
        return ctx.search_local_points(p, c["q"], c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["desc"], th_high=th_high, **a)
    refused("nlevels", lambda: call(P, nlevels=0))
    refused("nlevels", lambda: call(P, nlevels=17))
    refused("log_scale_factor", lambda: call(lv(2, 0.0)))
    refused("log_scale_factor", lambda: call(lv(2, -0.1)))
    refused("log_scale_factor", lambda: call(lv(2, float("nan"))))
    refused("level_mode", lambda: call(dict(P, level_mode=2)))
    refused("level_mode", lambda: call(dict(P, level_mode=-1)))
    refused("bounds", lambda: call(dict(P, bounds=(0.0, 0.0, 0.0, 480.0))))
    refused("bounds", lambda: call(dict(P, bounds=(0.0, 480.0, 640.0, 480.0))))
    refused("non-finite", lambda: call(dict(P, tcw=np.array([0, np.inf, 0], np.float32))))
    refused("non-finite", lambda: call(dict(P, rcw=np.where(np.eye(3) > 0, np.nan, 0).astype(np.float32))))
    refused("non-finite", lambda: call(dict(P, ow=np.array([np.nan, 0, 0], np.float32))))
    refused("non-finite", lambda: call(dict(P, intrinsics=(256.0, np.inf, 320.0, 240.0))))
    refused("non-finite", lambda: call(dict(P, mbf=np.float32(np.inf))))
    refused("non-finite", lambda: call(dict(P, bounds=(0.0, 0.0, np.inf, 480.0))))
    refused("non-finite", lambda: call(dict(P, th=np.float32(np.nan))))
    refused("non-finite", lambda: call(P, th_high=float("inf")))
    refused("non-finite keypoint", lambda: call(P, kpts=np.where(np.arange(16).reshape(8, 2) == 3, np.nan, c["kpts"]).astype(np.float32)))
    refused("exactly one", lambda: call(P, kxy=c["kxy"]))
    refused("exactly one", lambda: call(P, kpts=None))
    same(call(lv(1, 0.0)), ref)                                                    # one level needs no logarithm
    # the device form validates the same scalars before it touches a pointer
    lib, h = capi.lib, ctx.h
    o = np.zeros((16,), np.float32).ctypes.data

    def raw(p=None, Np=4, Nf=4, q=o, kp=o, kx=None, cap=64, m=o, st=o, sd=o):
        p = to_capi(P) if p is None else p
        return lib.rfe_search_local_points_dev(h, ctypes.byref(p) if p else None, q, o, o, o, o, sd, None, None, Np, o, kp, kx, None, None, Nf, None,
                                               1.4, cap, m, None, None, None, None, None, None, None, None, None, st)
    bad_mode = to_capi(dict(P, level_mode=5))
    for kw, msg in ((dict(Np=-1), "Np"), (dict(Np=16385), "Np"), (dict(Nf=-1), "Nf"), (dict(Nf=4097), "Nf"), (dict(cap=-1), "cand_cap"),
                    (dict(kx=o), "exactly one"), (dict(kp=None), "exactly one"), (dict(q=None), "null"), (dict(sd=None), "null"),
                    (dict(m=None), "null"), (dict(st=None), "null"), (dict(p=bad_mode), "level_mode"), (dict(p=0), "null")):
        assert raw(**kw) == -1 and msg in lib.rfe_last_error(h).decode(), (kw, lib.rfe_last_error(h).decode())
    same(call(P), ref)                                                             # the ctx is still usable


def test_profile_names_every_kernel(ctx, oracle):
    P, c, _ = solved(oracle, "main", 6, True, LEVEL_ZERO)
    ctx.profile(True); ctx.profile_reset()
    try:
        host(ctx, P, c)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False); ctx.profile_reset()
    for name in ("lp_frustum", "ps_grid", "ps_count", "ps_fill", "ps_resolve"):
        assert name in prof and prof[name][1] >= 1 and prof[name][0] > 0, prof


# ---------------------------------------------------------------- 5. the drop-in helper
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_helper(tmp_path, oracle):
    exe = DD.build(tmp_path, "local_points_driver")
    for name, th in (("main", 6), ("planted", 1)):
        P, c, ref = solved(oracle, name, th, True, LEVEL_ZERO)
        Np, Nf = len(c["pw"]), len(c["kpts"])
        before, prior = write_driver_case(str(tmp_path / "case.bin"), P, c)
        DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
        ret, n_to_match, who, got = read_driver_out(str(tmp_path / "out.bin"), Np, Nf)
        assert ret == ref["nmatches"] > 0 and n_to_match == ref["in_frustum"]
        assert np.array_equal(who, np.where(ref["assign"] >= 0, ref["assign"], prior))        # what was there before stays
        want = LP.map_point_fields(ref, before)
        for k in LP.FIELDS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k
        assert (want["proj_x"] == -1).sum() > 2 and (want["in_view"] != before["in_view"]).any()
        # a two-camera frame is refused, nothing is touched
        write_driver_case(str(tmp_path / "rig.bin"), P, c, nleft=500)
        DD.run(exe, str(tmp_path / "rig.bin"), str(tmp_path / "rig_out.bin"))
        ret, n_to_match, who, got = read_driver_out(str(tmp_path / "rig_out.bin"), Np, Nf)
        assert ret == -1 and n_to_match == 0 and np.array_equal(who, prior)
        for k in LP.FIELDS:
            assert np.array_equal(got[k], before[k]), k
