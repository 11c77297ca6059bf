"""GPU: Optimizer::OptimizeSim3 on the device (rfe_optimize_sim3 / _dev) against the contract of DESIGN.md 6k restated in
tests/optimize_sim3_ref.py.  Every comparison is exact (np.array_equal on s12 in double, s12_f32, keep, chi2, trace and stats), in host
and device form."""
import ctypes

import numpy as np
import pytest

import optimize_sim3_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUT = {"s12": F64, "s12_f32": F32, "keep": np.uint8, "chi2": F64, "trace": F64, "stats": np.int32}
OPTIONAL = ("s12_f32", "chi2", "trace")
SENTINEL, CHI2_SENTINEL = 7, F64(-3.0)
ARRAYS = ("xw1", "xw2", "valid", "kpts1", "octave1", "idx2")


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def batch(cases, N=None, N2=None, poison=True):
    """B cases stacked to [B, N] / [B, N2]: case b keeps its n rows and n2 keypoints in front, the rows behind are padding -- poisoned with
    NaN positions, huge octaves, set valid bytes and wild idx2 when `poison`"""
    B = len(cases)
    N = max([c["P"]["n"] for c in cases] + [0]) if N is None else N
    N2 = max([c["P"]["n2"] for c in cases] + [0]) if N2 is None else N2
    a = {"P": [c["P"] for c in cases], "s12_0": np.stack([c["s12_0"] for c in cases]).astype(F64) if B else np.zeros((0, 8), F64),
         "xw1": np.zeros((B, N, 3), F32), "xw2": np.zeros((B, N, 3), F32), "valid": np.zeros((B, N), np.uint8), "kpts1": np.zeros((B, N, 2), F32),
         "octave1": np.zeros((B, N), np.int32), "idx2": np.full((B, N), -1, np.int32), "kpts2": np.zeros((B, N2, 2), F32),
         "octave2": np.zeros((B, N2), np.int32)}
    if poison:
        a["xw1"][:], a["xw2"][:], a["kpts1"][:], a["kpts2"][:] = np.nan, np.nan, np.nan, np.nan
        a["valid"][:], a["octave1"][:], a["octave2"][:], a["idx2"][:] = 1, 1 << 30, 1 << 30, 5
    for b, c in enumerate(cases):
        n, n2 = c["P"]["n"], c["P"]["n2"]
        for k in ARRAYS:
            a[k][b, :n] = c[k][:n]
        a["kpts2"][b, :n2], a["octave2"][b, :n2] = c["kpts2"][:n2], c["octave2"][:n2]
    return a


def reference(a):
    B, N = a["valid"].shape
    if B == 0:
        return {"s12": np.zeros((0, 8), F64), "s12_f32": np.zeros((0, 8), F32), "keep": np.zeros((0, N), np.uint8),
                "chi2": np.zeros((0, N, 2), F64), "trace": np.zeros((0, 2, 8), F64), "stats": np.zeros((0, 8), np.int32)}
    return R.optimize_sim3_batch(a["P"], a["s12_0"], a["xw1"], a["xw2"], a["valid"], a["kpts1"], a["octave1"], a["idx2"], a["kpts2"], a["octave2"],
                                 np.full((B, N), SENTINEL, np.uint8), np.full((B, N, 2), CHI2_SENTINEL, F64))


def same(got, ref, keys=tuple(OUT)):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.argwhere(got[k] != ref[k])[:8], got[k].ravel()[:8], ref[k].ravel()[:8])


def host(ctx, a, outputs=OPTIONAL, octaves=True):
    B, N = a["valid"].shape
    return ctx.optimize_sim3(a["P"], a["s12_0"], a["xw1"], a["xw2"], a["valid"], a["kpts1"], a["idx2"], a["kpts2"],
                             octave1=a["octave1"] if octaves else None, octave2=a["octave2"] if octaves else None,
                             keep=np.full((B, N), SENTINEL, np.uint8), chi2=np.full((B, N, 2), CHI2_SENTINEL, F64), outputs=outputs)


def dev(ctx, a, outputs=OPTIONAL, octaves=True, calls=1):
    """rfe_optimize_sim3_dev on uploaded copies (`calls` times back to back); returns the host form's dict"""
    B, N = a["valid"].shape
    N2 = a["kpts2"].shape[1]
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(x.nbytes + 64))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    shape = {"s12": (B, 8), "s12_f32": (B, 8), "keep": (B, N), "chi2": (B, N, 2), "trace": (B, 2, 8), "stats": (B, 8)}
    fill = {"s12": 0, "s12_f32": 0, "keep": SENTINEL, "chi2": CHI2_SENTINEL, "trace": 5, "stats": 77}
    # every output sits between two guard words that must survive the call
    guard = {k: np.concatenate([np.full(8, 0x5A, np.uint8), np.full(shape[k], fill[k], OUT[k]).view(np.uint8).ravel(), np.full(8, 0x5A, np.uint8)])
             for k in ("s12", "keep", "stats") + tuple(outputs)}
    out = {k: up(g, np.uint8) for k, g in guard.items()}
    try:
        ins = [up(a["s12_0"], F64), up(a["xw1"], F32), up(a["xw2"], F32), up(a["valid"], np.uint8), up(a["kpts1"], F32), up(a["idx2"], np.int32),
               up(a["kpts2"], F32) if N2 else None]
        o1, o2 = (up(a["octave1"], np.int32), up(a["octave2"], np.int32)) if octaves else (None, None)
        for _ in range(calls):
            ctx.optimize_sim3_dev(a["P"], *ins, B, N, N2, out["s12"].ptr + 8, out["keep"].ptr + 8, out["stats"].ptr + 8, octave1=o1, octave2=o2,
                                  **{k: out[k].ptr + 8 for k in outputs})
        ctx.synchronize()
        res = {}
        for k in out:
            raw = out[k].download(guard[k].shape, np.uint8)
            assert (raw[:8] == 0x5A).all() and (raw[-8:] == 0x5A).all(), k
            res[k] = raw[8:-8].view(OUT[k]).reshape(shape[k]).copy()
        return res
    finally:
        for b in bufs:
            b.free()


def both(ctx, a, ref=None, **kw):
    ref = reference(a) if ref is None else ref
    keys = ("s12", "keep", "stats") + tuple(kw.get("outputs", OPTIONAL))
    h = host(ctx, a, **kw)
    same(h, ref, keys)
    same(dev(ctx, a, **kw), ref, keys)
    return h, ref


# ---------------------------------------------------------------- 1. sizes, one problem
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n", [0, 1, 9, 10, 255, 256, 257, 1100, 4096])
def test_sizes(ctx, n, fix_scale, mixed):
    c = R.scene(500 + n, n, fix_scale=fix_scale, mixed=mixed, pixel=False)
    h, ref = both(ctx, batch([c]))
    st = ref["stats"][0]
    if n >= 255:                                   # the scene is a real one: two rounds, most pairs inliers, some removed
        assert st[3] == 2 and st[0] > n // 2 and 0 < st[2] < n // 2
    if n < 10:
        assert st[7] & R.FLAG_EARLY and st[0] == 0 and np.array_equal(h["s12"][0], c["s12_0"])
    if fix_scale:
        assert h["s12"][0, 7] == c["s12_0"][7]
    print(f"n={n} fix_scale={fix_scale} mixed={mixed}: stats {h['stats'][0].tolist()}")


# ---------------------------------------------------------------- 2. several problems, each with its own n, n2, poses, cameras and flags
def test_batch_of_five(ctx):
    spec = ((600, False, False), (0, True, False), (1100, False, True), (257, True, True), (41, False, False))
    cases = [R.scene(540 + b, n, fix_scale=fs, mixed=mx, pixel=False, all_points=b != 4) for b, (n, fs, mx) in enumerate(spec)]
    a = batch(cases, N=1100, N2=1200)
    assert [P["n"] for P in a["P"]] == [600, 0, 1100, 257, 41] and np.isnan(a["xw1"][0, 600:]).all() and a["valid"][1].all()
    h, ref = both(ctx, a)
    assert (ref["stats"][:, 3] == [2, 0, 2, 2, 2]).all() and len({p.tobytes() for p in ref["s12"]}) == 5
    for b, c in enumerate(cases):                  # the sentinel survives behind n and where no pair was removed
        n = c["P"]["n"]
        assert (h["keep"][b, n:] == SENTINEL).all() and (h["chi2"][b, n:] == CHI2_SENTINEL).all()
        assert set(np.unique(h["keep"][b, :n])) <= {0, SENTINEL}
    assert h["ret"] == ref["stats"][0, 0]
    # nine problems take two launches
    nine = batch([R.scene(560 + b, 40 + b, mixed=bool(b & 1), pixel=False) for b in range(9)])
    both(ctx, nine)


def test_optional_arguments_null(ctx):
    c = R.scene(571, 300, mixed=True, pixel=False)
    a = batch([c])
    ref = reference(a)
    for outputs in ((), ("chi2",), ("s12_f32", "trace")):
        both(ctx, a, ref=ref, outputs=outputs)
    z = dict(a, octave1=np.zeros_like(a["octave1"]), octave2=np.zeros_like(a["octave2"]))
    zref = reference(z)
    assert not np.array_equal(ref["s12"], zref["s12"])
    both(ctx, a, ref=zref, octaves=False)
    # an octave outside the table reads level 0
    both(ctx, dict(a, octave1=np.full_like(a["octave1"], -5), octave2=np.full_like(a["octave2"], 99)), ref=zref)
    # N2 = 0: no keypoint array at all, every row observes the point's normalised coordinates
    e = batch([dict(c, P=dict(c["P"], n2=0))], N2=0)
    _, eref = both(ctx, e)
    assert eref["stats"][0, 7] & R.FLAG_IDX2


# ---------------------------------------------------------------- 3. the forced paths of the CPU tests
@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(ctx, name):
    c = R.forced(name)
    h, ref = both(ctx, batch([c]))
    st = ref["stats"][0]
    if name == "stale":
        assert st[7] & R.FLAG_ENDED_REJECTED
    elif name in ("z_zero", "nan"):
        assert st[7] & R.FLAG_NONFINITE and np.array_equal(h["s12"][0], c["s12_0"])
    elif name == "survivors9":
        assert st[7] & R.FLAG_EARLY and st[2] == 3 and (h["keep"][0, :3] == 0).all() and np.array_equal(h["s12"][0], c["s12_0"])
    elif name == "idx2_range":
        assert st[7] & R.FLAG_IDX2
    elif name == "fix_scale":
        assert h["s12"][0, 7] == 1.0625
    elif name in R.TH2_TARGETS:                    # one ulp either side of (double) th2 in the final classification, and th2 itself
        row, th2 = c["th2_row"], F64(c["P"]["th2"])
        want = th2 if R.TH2_TARGETS[name] is None else np.nextafter(th2, R.TH2_TARGETS[name])
        assert np.array_equal(h["s12"][0], c["s12_0"]) and st[3] == 2 and st[2] == 0
        assert h["chi2"][0, row, 0] == want and h["keep"][0, row] == (0 if name == "th2_above" else SENTINEL)


def test_two_calls_back_to_back(ctx):
    a = batch([R.scene(581, 400, mixed=True, pixel=False), R.scene(582, 300)])
    same(dev(ctx, a, calls=2), reference(a))


# ---------------------------------------------------------------- 4. the chain into the Sim3 projection search, on one ctx
def search_params(S3, s12_f32, cam, bounds):
    """rfe_sim3_params of Tcw = SE3f(S.rotationMatrix(), S.translation() / S.scale()) (SPmatcher.cc:1566) from s12_f32 = qx qy qz qw tx ty tz s"""
    q, t, s = s12_f32[:4].astype(F32), s12_f32[4:7].astype(F32), F32(s12_f32[7])
    q = (q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])).astype(F32)
    return S3.params(q, (t / s).astype(F32), cam, bounds, 10)


def test_chain_into_the_sim3_projection_search(ctx, oracle):
    """optimize_sim3_dev, then search_by_projection_sim3_dev on the same ctx over map points that were resident before either call: KF2's
    points (in camera 2's frame, the search's world) projected through the refined S12 onto KF1's keypoints.  The search takes its
    transform in a host structure, so between the two lies the one 32-byte read of s12_f32 the documents describe.  Compared with the host
    route (rfe_optimize_sim3, rfe_search_by_projection_sim3) and with both restatements."""
    import sim3_search_ref as S3
    c = R.scene(591, 300, noise=0.3)
    a = batch([c])
    n, P = c["P"]["n"], c["P"]
    rng = np.random.default_rng(591)
    pw = R.to_camera(P["rcw2"], P["tcw2"], c["xw2"][:n])                  # float32, as the optimisation forms P3D2c
    desc = rng.standard_normal((n, 256)).astype(F32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(F32)
    q = (desc + F32(0.02) * rng.standard_normal((n, 256)).astype(F32)).astype(F32)
    dist = np.sqrt((pw.astype(F64) ** 2).sum(1))
    bounds = (-160.0, -160.0, 928.0, 640.0)                               # the planted gross outliers lie up to 120 px outside the image
    ref_os = reference(a)
    assert ref_os["stats"][0, 3] == 2 and ref_os["stats"][0, 0] > 200
    Ps = search_params(S3, ref_os["s12_f32"][0], P["cam1"], bounds)
    po = pw.astype(F64) - Ps["ow"].astype(F64)
    d = np.sqrt((po * po).sum(1))
    sc = {"kpts": np.ascontiguousarray(c["kpts1"][:n]), "desc": desc, "q": q, "pw": np.ascontiguousarray(pw),
          "normal": (po / d[:, None]).astype(F32), "min_dist": (0.5 * d).astype(F32), "max_dist": (F32(1.2) * d.astype(F32)).astype(F32),
          "scale_dist": d.astype(F32), "valid": np.ones(n, np.uint8), "matched_in": np.zeros(n, np.uint8)}
    ref = S3.search(oracle, Ps, sc, S3.DIST_FLOAT)
    inl = ~c["planted"][:n]
    # the refined S12 in the layout and convention the search consumes: every inlier point lands on its own keypoint
    assert ref["nmatches"] >= 0.9 * inl.sum() and (ref["best_idx"][inl] == np.flatnonzero(inl)).mean() > 0.9, ref["nmatches"]
    assert dist.min() > 1.0
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)).upload(x))
        return bufs[-1]
    try:
        # everything both calls read goes up first
        sd = {k: up(sc[k], F32) for k in ("q", "pw", "normal", "min_dist", "max_dist", "scale_dist", "desc", "kpts")}
        sd.update({k: up(sc[k], np.uint8) for k in ("valid", "matched_in")})
        od = {k: up(a[k], dt) for k, dt in (("s12_0", F64), ("xw1", F32), ("xw2", F32), ("valid", np.uint8), ("kpts1", F32), ("idx2", np.int32),
                                            ("kpts2", F32), ("octave1", np.int32), ("octave2", np.int32))}
        out = {"s12": up(np.zeros((1, 8), F64), F64), "keep": up(np.full((1, n), SENTINEL, np.uint8), np.uint8), "stats": up(np.zeros((1, 8), np.int32), np.int32),
               "s12_f32": up(np.zeros((1, 8), F32), F32)}
        so = {k: up(np.zeros(n * (2 if k == "proj" else 1), np.int32), np.int32) for k in ("matched", "best_idx", "best_dist", "proj", "reject")}
        so["stats"] = up(np.full(8, 77, np.int32), np.int32)
        ctx.optimize_sim3_dev(a["P"], od["s12_0"], od["xw1"], od["xw2"], od["valid"], od["kpts1"], od["idx2"], od["kpts2"], 1, n, n, out["s12"],
                              out["keep"], out["stats"], octave1=od["octave1"], octave2=od["octave2"], s12_f32=out["s12_f32"])
        s12_f32 = out["s12_f32"].download((8,), F32)                       # the 32-byte read
        assert np.array_equal(s12_f32, ref_os["s12_f32"][0])
        Pd = search_params(S3, s12_f32, P["cam1"], bounds)
        ctx.search_by_projection_sim3_dev(S3.to_capi(Pd, S3.DIST_FLOAT), sd["q"], sd["pw"], sd["normal"], sd["min_dist"], sd["max_dist"],
                                          sd["scale_dist"], n, sd["desc"], n, S3.TH_LOW, ref["candidates"] + 16, so["matched"], so["stats"],
                                          valid=sd["valid"], kpts=sd["kpts"], matched_in=sd["matched_in"], best_idx=so["best_idx"],
                                          best_dist=so["best_dist"], proj=so["proj"], reject=so["reject"])
        ctx.synchronize()
        got = {"matched": so["matched"].download((n,), np.int32), "best_idx": so["best_idx"].download((n,), np.int32),
               "best_dist": so["best_dist"].download((n,), F32), "proj": so["proj"].download((n, 2), F32), "reject": so["reject"].download((n,), np.int32)}
        assert np.array_equal(out["keep"].download((1, n), np.uint8), ref_os["keep"])
    finally:
        for b in bufs:
            b.free()
    # the host route: both host entries, the same composition in between
    ho = host(ctx, a)
    hs = ctx.search_by_projection_sim3(S3.to_capi(search_params(S3, ho["s12_f32"][0], P["cam1"], bounds), S3.DIST_FLOAT), sc["q"], sc["pw"], sc["normal"],
                                       sc["min_dist"], sc["max_dist"], sc["scale_dist"], sc["desc"], S3.TH_LOW, valid=sc["valid"], kpts=sc["kpts"],
                                       matched_in=sc["matched_in"])
    for k in got:
        assert np.array_equal(got[k], hs[k], equal_nan=True) and np.array_equal(got[k], ref[k], equal_nan=True), k
    assert hs["nmatches"] == ref["nmatches"] == int((got["matched"] >= 0).sum())


# ---------------------------------------------------------------- 5. refusals
def test_refusals(ctx):
    from rover_slam_amd import capi
    c = R.scene(595, 20)
    a = batch([c])

    def refused(params=None, B=1, N=20, N2=20, null=(), form="both"):
        p = capi.optimize_sim3_params(a["P"]) if params is None else params
        b1 = max(B, 1)
        s12, sf, tr, st = np.zeros((b1, 8), F64), np.zeros((b1, 8), F32), np.zeros((b1, 16), F64), np.zeros((b1, 8), np.int32)
        keep = np.full((max(B * N, 1),), SENTINEL, np.uint8)
        args = {"params": ctypes.addressof(p), "s12_0": a["s12_0"].ctypes.data, "xw1": a["xw1"].ctypes.data, "xw2": a["xw2"].ctypes.data,
                "valid": a["valid"].ctypes.data, "kpts1": a["kpts1"].ctypes.data, "octave1": a["octave1"].ctypes.data, "idx2": a["idx2"].ctypes.data,
                "kpts2": a["kpts2"].ctypes.data, "octave2": a["octave2"].ctypes.data, "B": B, "N": N, "N2": N2, "s12": s12.ctypes.data,
                "s12_f32": sf.ctypes.data, "keep": keep.ctypes.data, "chi2": None, "trace": tr.ctypes.data, "stats": st.ctypes.data}
        for k in null:
            args[k] = None
        # the _dev form checks its arguments before it touches a pointer, so host addresses do for the refusals
        fns = {"both": (capi.lib.rfe_optimize_sim3, capi.lib.rfe_optimize_sim3_dev), "host": (capi.lib.rfe_optimize_sim3,)}[form]
        for fn in fns:
            assert fn(ctx.h, *args.values()) == -1 and b"optimize_sim3" in capi.lib.rfe_last_error(ctx.h)     # RFE_ERR_INVALID
            assert (keep == SENTINEL).all() and not s12.any() and not st.any()                                # nothing touched
        return True

    assert refused(B=-1) and refused(B=65) and refused(N=-1) and refused(N=4097) and refused(N2=-1) and refused(N2=4097)
    for field in ("nlevels1", "nlevels2"):
        for nl in (0, 17):
            p = capi.optimize_sim3_params(a["P"]); setattr(p[0], field, nl)
            assert refused(params=p)
    p = capi.optimize_sim3_params(a["P"]); p[0].iterations[2] = -1
    assert refused(params=p)
    p = capi.optimize_sim3_params(a["P"]); p[0].max_trials = -1
    assert refused(params=p)
    for k in ("params", "s12_0", "xw1", "xw2", "valid", "kpts1", "idx2", "kpts2", "s12", "keep", "stats"):
        assert refused(null=(k,))
    for field in ("fx1", "cy2", "th2"):            # the host form alone: non-finite params
        p = capi.optimize_sim3_params(a["P"]); setattr(p[0], field, float("nan"))
        assert refused(params=p, form="host")
    p = capi.optimize_sim3_params(a["P"]); p[0].inv_level_sigma2_2[1] = float("inf")
    assert refused(params=p, form="host")
    p = capi.optimize_sim3_params(a["P"]); p[0].rcw1[4] = float("nan")
    assert refused(params=p, form="host")
    both(ctx, a)                                   # and the context still works
