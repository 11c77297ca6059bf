"""GPU: the two Sim3 SearchByProjection overloads of loop closing on the device (rfe_search_by_projection_sim3 / _dev,
SearchByProjectionSim3_rfe) against the contract of DESIGN.md 6e restated in tests/sim3_search_ref.py.  Every comparison is exact
(np.array_equal on every output), in host and device form."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import sim3_search_ref as S3
from sim3_search_ref import MODES, RATIO_HAMMING, solved, to_capi, write_driver_case
from rover_slam_amd import capi

pytestmark = pytest.mark.gpu
OUT = {"matched": np.int32, "best_idx": np.int32, "best_dist": np.float32, "second_dist": np.float32, "proj": np.float32,
       "radius": np.float32, "level": np.int32, "reject": np.int32}
assert tuple(OUT) == S3.KEYS


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def same(got, ref, keys=S3.KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(1))[:8])
    assert got["nmatches"] == ref["nmatches"]


def check_stats(st, ref):
    assert list(st[[0, 1, 3, 4]]) == [ref["nmatches"], ref["candidates"], 0, ref["searched"]] and st[2] >= 1 and (st[5:] == 0).all(), st


def host(ctx, P, c, dist_mode, th_accept=S3.TH_LOW, **kw):
    a = dict(valid=c.get("valid"), kpts=c["kpts"], matched_in=c.get("matched_in"))
    a.update(kw)
    return ctx.search_by_projection_sim3(to_capi(P, dist_mode), c["q"], c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["desc"],
                                         th_accept, **a)


def dev(ctx, P, c, dist_mode, cand_cap, th_accept=S3.TH_LOW, outputs=S3.KEYS):
    """rfe_search_by_projection_sim3_dev on uploaded copies of the host arrays; returns the host form's dict"""
    Np, Nf = len(c["pw"]), len(c["kpts"])
    bufs = []

    def up(a, dt):
        a = np.ascontiguousarray(a, dt)
        bufs.append(ctx.alloc(max(a.nbytes, 4)))
        return bufs[-1].upload(a) if a.nbytes else bufs[-1]
    shape = {k: (Nf,) if k == "matched" else ((Np, 2) if k == "proj" else (Np,)) for k in OUT}
    out = {k: ctx.alloc(max(int(np.prod(shape[k])), 1) * 4) for k in outputs}
    out["stats"] = ctx.alloc(32).upload(np.full((8,), 77, np.int32))               # the call clears the words it adds to
    try:
        ctx.search_by_projection_sim3_dev(to_capi(P, dist_mode), up(c["q"], np.float32), up(c["pw"], np.float32), up(c["normal"], np.float32),
                                          up(c["min_dist"], np.float32), up(c["max_dist"], np.float32), up(c["scale_dist"], np.float32), Np, up(c["desc"], np.float32), Nf,
                                          th_accept, cand_cap, out["matched"], out["stats"], valid=up(c["valid"], np.uint8),
                                          kpts=up(c["kpts"], np.float32), matched_in=up(c["matched_in"], np.uint8),
                                          **{k: out[k] for k in outputs if k != "matched"})
        ctx.synchronize()
        r = {k: out[k].download(shape[k], OUT[k]) if np.prod(shape[k]) else np.zeros(shape[k], OUT[k]) for k in outputs}
        r["stats"] = out["stats"].download((8,), np.int32)
        r["nmatches"] = int(r["stats"][0])
        return r
    finally:
        for b in bufs + list(out.values()):
            b.free()


# ---------------------------------------------------------------- 1. the main case, both projection forms and both distance modes
@pytest.mark.parametrize("proj_mode,dist_mode", MODES)
def test_main_case(ctx, oracle, proj_mode, dist_mode):
    P, c, ref = solved(oracle, "main", proj_mode, dist_mode)
    h = host(ctx, P, c, dist_mode)
    same(h, ref)
    check_stats(h["stats"], ref)
    d = dev(ctx, P, c, dist_mode, ref["candidates"])                               # exactly the slots the lists need
    same(d, ref)
    assert np.array_equal(d["stats"], h["stats"])
    print(f"proj_mode {proj_mode}, dist_mode {dist_mode}: stats {list(h['stats'])}")
    _, _, static = solved(oracle, "main", proj_mode, dist_mode, sequential=False)
    searched = ref["reject"] == 0
    assert (static["best_idx"] != h["best_idx"])[searched].sum() >= 0.2 * searched.sum()   # the sequence matters: not what one bulk scan gives


@pytest.mark.parametrize("proj_mode,dist_mode", MODES)
def test_main_case_with_eight_levels(ctx, oracle, proj_mode, dist_mode):
    P, c, ref = solved(oracle, "main8", proj_mode, dist_mode)
    assert len(np.unique(ref["level"][ref["reject"] == 0])) == 8
    assert not np.array_equal(c["max_dist"], c["scale_dist"])                      # the gate's distance is not PredictScale's
    h = host(ctx, P, c, dist_mode)
    same(h, ref)
    check_stats(h["stats"], ref)
    d = dev(ctx, P, c, dist_mode, ref["candidates"] + 100)
    same(d, ref)
    assert np.array_equal(d["stats"], h["stats"])


# ---------------------------------------------------------------- 2. the planted points
@pytest.mark.parametrize("proj_mode,dist_mode", MODES)
def test_planted_case(ctx, oracle, proj_mode, dist_mode):
    P, c, ref = solved(oracle, "planted", proj_mode, dist_mode)
    h = host(ctx, P, c, dist_mode)
    same(h, ref)
    check_stats(h["stats"], ref)
    assert list(h["reject"]) == [code for _, code in S3.PLANTED_POINTS] and list(h["matched"]) == list(S3.PLANTED_MATCHED)
    d = dev(ctx, P, c, dist_mode, ref["candidates"])
    same(d, ref)
    assert np.array_equal(d["stats"], h["stats"])
    # valid = NULL: every point is valid, and the would-be winner takes its feature
    v = S3.search(oracle, P, c, dist_mode, valid=np.ones(len(c["pw"]), np.uint8))
    same(host(ctx, P, c, dist_mode, valid=None), v)
    assert v["matched"][1] == 4


# ---------------------------------------------------------------- 3. other shapes
def test_no_map_points_and_no_features(ctx, oracle):
    P, c, ref = solved(oracle, "main")
    none = {k: (v[:0] if k in ("q", "pw", "normal", "min_dist", "max_dist", "scale_dist", "valid") else v) for k, v in c.items()}
    e = host(ctx, P, none, S3.DIST_FLOAT)
    assert e["nmatches"] == 0 and len(e["matched"]) == len(c["kpts"]) and (e["matched"] == -1).all()
    assert all(len(e[k]) == 0 for k in S3.KEYS if k != "matched") and list(e["stats"][[0, 1, 3, 4]]) == [0, 0, 0, 0]
    d = dev(ctx, P, none, S3.DIST_TRUNC, 16)
    assert (d["matched"] == -1).all() and list(d["stats"][[0, 1, 3, 4]]) == [0, 0, 0, 0] and (d["stats"][5:] == 0).all()
    nof = dict(c, kpts=c["kpts"][:0], desc=c["desc"][:0], matched_in=c["matched_in"][:0])
    e = host(ctx, P, nof, S3.DIST_FLOAT)
    same(e, dict(ref, matched=ref["matched"][:0], best_idx=np.full_like(ref["best_idx"], -1), best_dist=np.full_like(ref["best_dist"], 256),
                 second_dist=np.full_like(ref["second_dist"], 256), nmatches=0))
    assert e["stats"][4] == ref["searched"] and e["stats"][1] == 0


def test_every_point_rejected(ctx, oracle):
    P, c, _ = solved(oracle, "main")
    for dist_mode in (S3.DIST_FLOAT, S3.DIST_TRUNC):
        nobody = dict(c, valid=np.zeros_like(c["valid"]))
        ref = S3.search(oracle, P, nobody, dist_mode)
        assert (ref["reject"] == 1).all() and ref["candidates"] == 0
        h = host(ctx, P, nobody, dist_mode)
        same(h, ref)
        check_stats(h["stats"], ref)
        assert (h["matched"] == -1).all() and (h["radius"] == 0).all() and (h["level"] == -1).all()
    behind = dict(P, quat=np.array([0, 1, 0, 0], np.float32))                      # half a turn about y: most of the scene is behind the camera
    ref = S3.search(oracle, behind, c)
    assert (ref["reject"] == 2).sum() > 1500
    same(host(ctx, behind, c, S3.DIST_FLOAT), ref)


def test_overflow_is_reported_and_harmless(ctx, oracle):
    P, c, ref = solved(oracle, "main", S3.PROJ_DIV, S3.DIST_TRUNC)
    o = dev(ctx, P, c, S3.DIST_TRUNC, ref["candidates"] - 1)                      # one slot short
    assert list(o["stats"]) == [0, ref["candidates"], o["stats"][2], 1, ref["searched"], 0, 0, 0]
    assert (o["matched"] == -1).all() and (o["best_idx"] == -1).all() and (o["best_dist"] == 256).all() and (o["second_dist"] == 256).all()
    for k in ("proj", "radius", "level", "reject"):                                # the front does not depend on the slots
        assert np.array_equal(o[k], ref[k]), k
    # only the required outputs
    m = dev(ctx, P, c, S3.DIST_TRUNC, ref["candidates"], outputs=("matched",))
    assert np.array_equal(m["matched"], ref["matched"]) and m["stats"][3] == 0


def test_one_ctx_across_cases_is_bit_for_bit(oracle):
    c0 = capi.Context(0)
    try:
        first = None
        for name in ("main", "planted", "main"):
            P, c, ref = solved(oracle, name)
            got = host(c0, P, c, S3.DIST_FLOAT)
            same(got, ref)
            check_stats(got["stats"], ref)
            if first is None:
                first = got
        for k in S3.KEYS + ("stats",):
            assert np.array_equal(got[k], first[k]), k
    finally:
        c0.close()


def test_host_form_takes_its_second_attempt(oracle):
    """A fresh ctx has ps_cap = 0, so the host form first runs with 16 slots per map point.  At th = 40 the lists of 64 points over 300
    features need about three times that: the first attempt overflows, the second runs with exactly stats[1] slots.  The second call on
    the same ctx starts from the remembered slot count and gives the same bits in one attempt."""
    P, c = S3.make_case(0, W=160, H=120, Nf=300, Np=64, th=40)
    ref = S3.search(oracle, P, c, S3.DIST_FLOAT)
    Np, Nf = len(c["pw"]), len(c["kpts"])
    print(f"candidates {ref['candidates']}, first guess {16 * Np}, ceiling {Np * Nf}, nmatches {ref['nmatches']}")
    assert 16 * Np < ref["candidates"] <= Np * Nf
    c0 = capi.Context(0)
    try:
        first = host(c0, P, c, S3.DIST_FLOAT)
        same(first, ref)
        check_stats(first["stats"], ref)
        assert first["stats"][1] == ref["candidates"] and first["stats"][3] == 0 and first["stats"][0] == ref["nmatches"]
        again = host(c0, P, c, S3.DIST_FLOAT)
        for k in S3.KEYS + ("stats",):
            assert np.array_equal(again[k], first[k], equal_nan=True), k
        assert again["nmatches"] == first["nmatches"]
    finally:
        c0.close()


# ---------------------------------------------------------------- 4. refusals and profile stages
def test_refusals(ctx, oracle):
    P, c, ref = solved(oracle, "planted")

    def refused(msg, fn):
        with pytest.raises(capi.RfeError) as ex:
            fn()
        assert "error -1" in str(ex.value) and msg in str(ex.value), str(ex.value)
    lv = lambda n, lsf=0.2: dict(P, nlevels=n, scale_factors=np.ones(min(max(n, 1), 16), np.float32), log_scale_factor=np.float32(lsf))   # noqa: E731

    def call(Pm, dist_mode=S3.DIST_FLOAT, nlevels=None, **kw):
        p = to_capi(Pm, dist_mode)
        if nlevels is not None:
            p.nlevels = nlevels
        a = dict(valid=c["valid"], kpts=c["kpts"], matched_in=c["matched_in"])
        a.update(kw)
        return ctx.search_by_projection_sim3(p, c["q"], c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["desc"], 1.2, **a)
    refused("nlevels", lambda: call(P, nlevels=0))
    refused("nlevels", lambda: call(P, nlevels=17))
    refused("log_scale_factor", lambda: call(lv(2, 0.0)))
    refused("log_scale_factor", lambda: call(lv(2, -0.1)))
    refused("log_scale_factor", lambda: call(lv(2, float("nan"))))
    refused("proj_mode", lambda: call(dict(P, proj_mode=2)))
    refused("dist_mode", lambda: call(P, dist_mode=-1))
    refused("bounds", lambda: call(dict(P, bounds=(0.0, 0.0, 0.0, 480.0))))
    refused("non-finite", lambda: call(dict(P, t=np.array([0, np.inf, 0], np.float32))))
    refused("non-finite", lambda: call(dict(P, quat=np.array([0, 0, np.nan, 1], np.float32))))
    refused("non-finite", lambda: call(dict(P, intrinsics=(256.0, np.inf, 320.0, 240.0))))
    refused("exactly one", lambda: call(P, kxy=c["kpts"].astype(np.int32)))
    refused("exactly one", lambda: call(P, kpts=None))
    same(call(lv(1, 0.0)), ref)                                                    # one level needs no logarithm
    # the device form validates the same scalars before it touches a pointer
    lib, h = capi.lib, ctx.h
    o = np.zeros((16,), np.float32).ctypes.data
    import ctypes

    def raw(p=None, Np=4, Nf=4, q=o, kp=o, kx=None, cap=64, m=o, st=o):
        p = to_capi(P, S3.DIST_FLOAT) if p is None else p
        return lib.rfe_search_by_projection_sim3_dev(h, ctypes.byref(p) if p else None, q, o, o, o, o, o, None, Np, o, kp, kx, None, Nf, None, 1.2,
                                                     cap, m, None, None, None, None, None, None, None, st)
    bad_mode = to_capi(P, 5)
    for kw, msg in ((dict(Np=-1), "Np"), (dict(Np=16385), "Np"), (dict(Nf=4097), "Nf"), (dict(cap=-1), "cand_cap"), (dict(kx=o), "exactly one"),
                    (dict(kp=None), "exactly one"), (dict(q=None), "null"), (dict(m=None), "null"), (dict(st=None), "null"),
                    (dict(p=bad_mode), "dist_mode"), (dict(p=0), "null")):
        assert raw(**kw) == -1 and msg in lib.rfe_last_error(h).decode(), (kw, lib.rfe_last_error(h).decode())
    same(call(P), ref)                                                             # the ctx is still usable


def test_profile_names_every_kernel(ctx, oracle):
    P, c, _ = solved(oracle, "main")
    ctx.profile(True); ctx.profile_reset()
    try:
        host(ctx, P, c, S3.DIST_FLOAT)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False); ctx.profile_reset()
    for name in ("s3_project", "ps_grid", "ps_count", "ps_fill", "ps_resolve"):
        assert name in prof and prof[name][1] >= 1 and prof[name][0] > 0, prof


# ---------------------------------------------------------------- 5. the drop-in helpers
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_helpers(tmp_path, oracle):
    P, c, _ = solved(oracle, "main")
    exe = DD.build(tmp_path, "sim3_search_driver")
    Pd, prior = write_driver_case(str(tmp_path / "case.bin"), P, c)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    Nf = len(c["kpts"])
    out = np.fromfile(str(tmp_path / "out.bin"), np.int32).reshape(2, 1 + 2 * Nf)
    for k, (proj_mode, dist_mode, th_accept) in enumerate(((S3.PROJ_INVZ, S3.DIST_FLOAT, S3.TH_LOW),
                                                           (S3.PROJ_DIV, S3.DIST_TRUNC, np.float32(S3.TH_LOW * RATIO_HAMMING)))):
        ref = S3.search(oracle, dict(Pd, proj_mode=proj_mode), c, dist_mode, th_accept)
        assert ref["nmatches"] > 100
        ret, who, kf = out[k, 0], out[k, 1:1 + Nf], out[k, 1 + Nf:]
        assert ret == ref["nmatches"]
        assert np.array_equal(who, np.where(ref["matched"] >= 0, ref["matched"], prior))      # what was there before stays
        assert np.array_equal(kf, np.where(ref["matched"] >= 0, ref["matched"] % 7, -1) if k == 0 else np.full(Nf, -1))
    assert not np.array_equal(out[0, 1:1 + Nf], out[1, 1:1 + Nf])
    # a two-camera keyframe is refused, nothing is touched
    write_driver_case(str(tmp_path / "rig.bin"), P, c, nleft=500)
    DD.run(exe, str(tmp_path / "rig.bin"), str(tmp_path / "rig_out.bin"))
    out = np.fromfile(str(tmp_path / "rig_out.bin"), np.int32).reshape(2, 1 + 2 * Nf)
    for k in range(2):
        assert out[k, 0] == -1 and np.array_equal(out[k, 1:1 + Nf], prior) and (out[k, 1 + Nf:] == -1).all()
