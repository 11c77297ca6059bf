"""GPU: Optimizer::PoseOptimization on the device (rfe_pose_optimization / _dev) against the contract of DESIGN.md 6i restated in
tests/pose_opt_ref.py.  Every comparison is exact (np.array_equal on the pose in double, pose_f32, outlier, chi2, trace and stats), in host
and device form."""
import ctypes

import numpy as np
import pytest

import pose_opt_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUT = {"pose": F64, "pose_f32": F32, "outlier": np.uint8, "chi2": F32, "trace": F64, "stats": np.int32}
KINDS = ("mono", "stereo", "mixed")
SENTINEL, CHI2_SENTINEL = 7, F32(-3.0)


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def to_capi(P):
    from rover_slam_amd import capi
    return capi.pose_params(P["fx"], P["fy"], P["cx"], P["cy"], P["bf"], P["inv_level_sigma2"], P["iterations"], P["max_trials"])


def batch(cases, N=None, poison=True, seed=0):
    """B cases stacked to [B, N]: case b keeps its n = len(kpts) features in front, the rows behind are padding -- poisoned with NaN
    positions, huge octaves and set has_mp when `poison`"""
    rng = np.random.default_rng(seed)
    B = len(cases)
    N = max(len(c["kpts"]) for c in cases) if N is None else N
    a = {"pose0": np.stack([c["pose0"] for c in cases]).astype(F32) if B else np.zeros((0, 7), F32), "kpts": np.zeros((B, N, 2), F32),
         "octave": np.zeros((B, N), np.int32), "uright": np.full((B, N), -1, F32), "xw": np.zeros((B, N, 3), F32),
         "has_mp": np.zeros((B, N), np.uint8), "n": np.array([len(c["kpts"]) for c in cases], np.int32)}
    if poison:
        a["kpts"][:], a["xw"][:], a["octave"][:], a["has_mp"][:] = np.nan, np.nan, 1 << 30, 1
        a["uright"][:] = rng.choice(np.array([-1, np.nan, 50], F32), (B, N))
    for b, c in enumerate(cases):
        n = len(c["kpts"])
        for k in ("kpts", "octave", "uright", "xw", "has_mp"):
            a[k][b, :n] = c[k]
    return a


def reference(P, a, with_n=True):
    B, N = a["has_mp"].shape
    if B == 0:
        return {"pose": np.zeros((0, 7), F64), "pose_f32": np.zeros((0, 7), F32), "outlier": np.zeros((0, N), np.uint8),
                "chi2": np.zeros((0, N), F32), "trace": np.zeros((0, 4, 8), F64), "stats": np.zeros((0, 8), np.int32)}
    rs = [R.pose_optimization(P, a["pose0"][b], a["kpts"][b], a["octave"][b], a["uright"][b], a["xw"][b], a["has_mp"][b],
                              a["n"][b] if with_n else None, np.full(N, SENTINEL, np.uint8), np.full(N, CHI2_SENTINEL, F32)) for b in range(B)]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in OUT}


def same(got, ref, keys=tuple(OUT)):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.argwhere(got[k] != ref[k])[:8], got[k].ravel()[:8], ref[k].ravel()[:8])


def host(ctx, P, a, outputs=("pose_f32", "chi2", "trace"), with_n=True, octave=True, uright=True):
    B, N = a["has_mp"].shape
    return ctx.pose_optimization(to_capi(P), a["pose0"], a["kpts"], a["xw"], a["has_mp"], octave=a["octave"] if octave else None,
                                 uright=a["uright"] if uright else None, n=a["n"] if with_n else None,
                                 outlier=np.full((B, N), SENTINEL, np.uint8), chi2=np.full((B, N), CHI2_SENTINEL, F32), outputs=outputs)


def dev(ctx, P, a, outputs=("pose_f32", "chi2", "trace"), with_n=True, octave=True, uright=True, pose0_buf=None, keep=None):
    """rfe_pose_optimization_dev on uploaded copies; returns the host form's dict.  pose0_buf: a device buffer to read pose0 from; keep:
    a list that receives the pose_f32 buffer instead of it being freed (the chain test)"""
    B, N = a["has_mp"].shape
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    shape = {"pose": (B, 7), "pose_f32": (B, 7), "outlier": (B, N), "chi2": (B, N), "trace": (B, 4, 8), "stats": (B, 8)}
    fill = {"pose": 0, "pose_f32": 0, "outlier": SENTINEL, "chi2": CHI2_SENTINEL, "trace": 5, "stats": 77}
    out = {k: up(np.full(shape[k], fill[k], OUT[k]), OUT[k]) for k in ("pose", "outlier", "stats") + tuple(outputs)}
    try:
        ctx.pose_optimization_dev(to_capi(P), pose0_buf if pose0_buf is not None else up(a["pose0"], F32), up(a["kpts"], F32), up(a["xw"], F32),
                                  up(a["has_mp"], np.uint8), B, N, out["pose"], out["outlier"], out["stats"],
                                  octave=up(a["octave"], np.int32) if octave else None, uright=up(a["uright"], F32) if uright else None,
                                  n=up(a["n"], np.int32) if with_n else None, **{k: out[k] for k in outputs})
        ctx.synchronize()
        return {k: out[k].download(shape[k], OUT[k]) if np.prod(shape[k]) else np.zeros(shape[k], OUT[k]) for k in out}
    finally:
        for b in bufs:
            if keep is not None and b is out.get("pose_f32"):
                keep.append(b)
            else:
                b.free()


def both(ctx, P, a, ref=None, **kw):
    ref = reference(P, a, kw.get("with_n", True)) if ref is None else ref
    h = host(ctx, P, a, **kw)
    same(h, ref)
    same(dev(ctx, P, a, **kw), ref)
    return h, ref


# ---------------------------------------------------------------- 1. sizes and kinds, one problem
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [0, 2, 3, 9, 10, 255, 256, 257, 1100, 4096])
def test_sizes_and_kinds(ctx, N, kind):
    c = R.scene(300 + N, N, kind, has=1.0 if N < 20 else 0.9)
    a = batch([c])
    h, ref = both(ctx, c["P"], a)
    if N >= 255:                                   # the scene is a real one: four rounds, most edges inliers, some outliers
        assert ref["stats"][0, 3] == 4 and ref["stats"][0, 0] > N // 2 and 0 < ref["stats"][0, 2] < N // 2
    print(f"N={N} {kind}: stats {h['stats'][0].tolist()}")


# ---------------------------------------------------------------- 2. several problems, each with its own n and pose0
def test_batch_of_five(ctx):
    P = R.scene(0, 4, "mixed")["P"]
    cases = [R.scene(40 + b, n, "mixed") for b, n in enumerate((600, 0, 257, 1100, 41))]
    a = batch(cases, N=1100)
    assert list(a["n"]) == [600, 0, 257, 1100, 41] and np.isnan(a["xw"][0, 600:]).all() and a["has_mp"][1].all()
    h, ref = both(ctx, P, a)
    assert (ref["stats"][:, 3] == [4, 0, 4, 4, 4]).all() and len({p.tobytes() for p in ref["pose"]}) == 5
    # the sentinel survives wherever has_mp == 0 and behind n
    for b, c in enumerate(cases):
        n = len(c["kpts"])
        assert (h["outlier"][b, n:] == SENTINEL).all() and (h["outlier"][b, :n][c["has_mp"] == 0] == SENTINEL).all()
        assert (h["outlier"][b, :n][c["has_mp"] != 0] <= 1).all() and (h["chi2"][b, n:] == CHI2_SENTINEL).all()
    # the host form returns problem 0's count
    assert h["ret"] == ref["stats"][0, 0]


def test_n_null_is_all_rows_and_optional_inputs(ctx):
    c = R.scene(61, 300, "mono")
    a = batch([c, R.scene(62, 300, "mono")], poison=False)
    both(ctx, c["P"], a, with_n=False)
    # octave = NULL reads level 0, uright = NULL is all mono
    z = dict(a, octave=np.zeros_like(a["octave"]), uright=np.full_like(a["uright"], -1))
    ref = reference(c["P"], z)
    same(host(ctx, c["P"], a, octave=False, uright=False), ref)
    same(dev(ctx, c["P"], a, octave=False, uright=False), ref)
    m = R.scene(63, 300, "mixed")
    am = batch([m])
    assert not np.array_equal(reference(m["P"], am)["pose"], reference(m["P"], dict(am, octave=np.zeros_like(am["octave"])))["pose"])
    both(ctx, m["P"], dict(am, octave=np.full_like(am["octave"], -5)), ref=reference(m["P"], dict(am, octave=np.zeros_like(am["octave"]))))


def test_optional_outputs_null(ctx):
    c = R.scene(64, 300, "mixed")
    a = batch([c])
    ref = reference(c["P"], a)
    for outputs in ((), ("chi2",), ("pose_f32", "trace")):
        keys = ("pose", "outlier", "stats") + outputs
        same(host(ctx, c["P"], a, outputs=outputs), ref, keys)
        same(dev(ctx, c["P"], a, outputs=outputs), ref, keys)


# ---------------------------------------------------------------- 3. the forced paths of the CPU tests
@pytest.mark.parametrize("name", ["rejected", "stale", "one_iteration", "exact", "two", "nine", "comes_back", "behind", "nan", "quadrants", "huge_step"])
def test_forced_paths(ctx, name):
    c = R.forced(name)
    h, ref = both(ctx, c["P"], batch([c]))
    st = ref["stats"][0]
    if name in ("rejected", "stale"):
        assert st[7] & R.FLAG_ENDED_REJECTED
    elif name == "one_iteration":
        assert st[4] == 4
    elif name == "exact":
        assert (ref["trace"][0, :, 0] == 1).all() and st[2] == 0 and st[6] == 4
    elif name == "two":
        assert st.tolist() == [0, 2, 0, 0, 0, 0, 0, 0] and np.array_equal(h["pose_f32"][0], c["pose0"]) and (h["chi2"] == CHI2_SENTINEL).all()
    elif name == "nine":
        assert st[3] == 1
    elif name == "behind":
        assert h["outlier"][0, c["special"]] == 1
    elif name == "nan":
        assert st[7] & R.FLAG_NONFINITE


# ---------------------------------------------------------------- 4. the chain: one call's pose_f32_dev is the next call's pose0_dev
def test_chain_on_the_device(ctx):
    c = R.scene(71, 500, "mixed", rot=0.1, trans=0.3)
    a = batch([c, R.scene(72, 500, "mixed")])
    P = c["P"]
    first = reference(P, a)
    second = reference(P, dict(a, pose0=first["pose_f32"]))
    assert not np.array_equal(first["pose"], second["pose"])
    keep = []
    same(dev(ctx, P, a, keep=keep), first)
    try:
        same(dev(ctx, P, a, pose0_buf=keep[0]), second)
    finally:
        keep[0].free()


# ---------------------------------------------------------------- 5. refusals
def test_refusals(ctx):
    from rover_slam_amd import capi
    c = R.scene(81, 20, "mixed")
    a = batch([c])
    P = c["P"]

    def refused(params=None, B=1, N=20, null=(), form="both", **arrays):
        x = dict(a, **arrays)
        p = to_capi(P) if params is None else params
        pose, pf, tr, st = np.zeros((max(B, 1), 7), F64), np.zeros((max(B, 1), 7), F32), np.zeros((max(B, 1), 32), F64), np.zeros((max(B, 1), 8), np.int32)
        out = np.zeros((max(B * N, 1),), np.uint8)
        args = {"params": ctypes.byref(p), "pose0": x["pose0"].ctypes.data, "kpts": x["kpts"].ctypes.data, "octave": x["octave"].ctypes.data,
                "uright": x["uright"].ctypes.data, "xw": x["xw"].ctypes.data, "has_mp": x["has_mp"].ctypes.data, "n": x["n"].ctypes.data,
                "B": B, "N": N, "pose": pose.ctypes.data, "pose_f32": pf.ctypes.data, "outlier": out.ctypes.data, "chi2": None,
                "trace": tr.ctypes.data, "stats": st.ctypes.data}
        for k in null:
            args[k] = None
        # the _dev form checks its arguments before it touches a pointer, so host addresses do for the refusals
        fns = {"both": (capi.lib.rfe_pose_optimization, capi.lib.rfe_pose_optimization_dev), "host": (capi.lib.rfe_pose_optimization,)}[form]
        for fn in fns:
            assert fn(ctx.h, *args.values()) == -1 and b"pose_optimization" in capi.lib.rfe_last_error(ctx.h)     # RFE_ERR_INVALID
        return True

    assert refused(B=-1) and refused(B=65) and refused(N=-1) and refused(N=4097)
    for nl in (0, 17):
        p = to_capi(P); p.nlevels = nl
        assert refused(params=p)
    p = to_capi(P); p.iterations[2] = -1
    assert refused(params=p)
    p = to_capi(P); p.max_trials = -1
    assert refused(params=p)
    for k in ("params", "pose0", "kpts", "xw", "has_mp", "pose", "outlier", "stats"):
        assert refused(null=(k,))
    # the host form alone: non-finite params or pose0
    for field in ("fx", "fy", "cx", "cy", "bf"):
        p = to_capi(P); setattr(p, field, float("nan"))
        assert refused(params=p, form="host")
    p = to_capi(P); p.inv_level_sigma2[1] = float("inf")
    assert refused(params=p, form="host")
    bad = a["pose0"].copy(); bad[0, 5] = np.nan
    assert refused(form="host", pose0=bad)
    # and the context still works
    both(ctx, P, a)
