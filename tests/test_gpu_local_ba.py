"""GPU: Optimizer::LocalBundleAdjustment on the device (rfe_local_ba / _dev) against the contract of DESIGN.md 6l restated in
tests/local_ba_ref.py.  Every comparison is exact (np.array_equal on pose and point in double, their float casts, erase, chi2, trace and
stats), in host and device form."""
import numpy as np
import pytest

import local_ba_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUT = {"pose": F64, "pose_f32": F32, "point": F64, "point_f32": F32, "erase": np.uint8, "chi2": F64, "trace": F64, "stats": np.int32}
OPTIONAL = ("pose_f32", "point_f32", "chi2", "trace")
REQUIRED = ("pose", "point", "erase", "stats")
PAD = 37                                         # rows of poison behind E, L and the feature arrays


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def lib_params(c, stop=None):
    from rover_slam_amd import capi
    p = c["params"]
    return capi.local_ba_params(p["iterations"], p["max_trials"], p["user_lambda_init"], p["th2_mono"], p["th2_stereo"], stop)


def padded(c):
    """the case's arrays with PAD poisoned rows behind E, L and Nf: wild indices, NaN positions and observations, huge octaves"""
    def pad(a, fill):
        a = np.asarray(a)
        return np.concatenate([a, np.full((PAD,) + a.shape[1:], fill, a.dtype)])
    return {"kpts": pad(c["kpts"], np.nan), "octave": pad(c["octave"], 1 << 30), "uright": pad(c["uright"], np.nan), "xw": pad(c["xw"], np.nan),
            "edge_point": pad(c["edge_point"], 1 << 30), "edge_kf": pad(c["edge_kf"], -5), "edge_feat": pad(c["edge_feat"], 1 << 30)}


def shape_of(c):
    return len(c["xw"]), len(c["edge_point"]), len(c["kpts"])


def same(got, ref, keys):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.argwhere(got[k] != ref[k])[:8], got[k].ravel()[:8], ref[k].ravel()[:8])


def host(ctx, c, outputs=OPTIONAL, stop=None):
    a = padded(c)
    return ctx.local_ba(lib_params(c, stop), c["P"], c["F"], c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"], a["kpts"],
                        a["xw"], a["edge_point"], a["edge_kf"], a["edge_feat"], octave=a["octave"], uright=a["uright"], outputs=outputs,
                        shape=shape_of(c))


def dev(ctx, c, outputs=OPTIONAL, stop=None, expect_error=False):
    """rfe_local_ba_dev on uploaded copies; returns the host form's dict.  Every output sits between two guard words that must survive"""
    a = padded(c)
    L, E, Nf = shape_of(c)
    P, its = c["P"], max(c["params"]["iterations"], 0)
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(x.nbytes + 64))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    shape = {"pose": (P, 7), "pose_f32": (P, 7), "point": (L, 3), "point_f32": (L, 3), "erase": (E,), "chi2": (E,), "trace": (its, 4), "stats": (8,)}
    fill = {"pose": 3, "pose_f32": 3, "point": 3, "point_f32": 3, "erase": 9, "chi2": -3, "trace": 5, "stats": 77}
    guard = {k: np.concatenate([np.full(8, 0x5A, np.uint8), np.full(shape[k], fill[k], OUT[k]).view(np.uint8).ravel(), np.full(8, 0x5A, np.uint8)])
             for k in REQUIRED + tuple(outputs)}
    out = {k: up(g, np.uint8) for k, g in guard.items()}
    try:
        ins = [up(c["kf_pose"], F32), up(c["kf_cam"], F32), up(c["kf_nlevels"], np.int32), up(c["kf_sigma2"], F32), up(c["kf_feat_off"], np.int32),
               up(a["kpts"], F32), up(a["xw"], F32), up(a["edge_point"], np.int32), up(a["edge_kf"], np.int32), up(a["edge_feat"], np.int32)]
        oc, ur = up(a["octave"], np.int32), up(a["uright"], F32)
        ret = ctx.local_ba_dev(lib_params(c, stop), P, c["F"], L, E, Nf, *ins, out["pose"].ptr + 8, out["point"].ptr + 8, out["erase"].ptr + 8,
                               out["stats"].ptr + 8, octave=oc, uright=ur, **{k: out[k].ptr + 8 for k in outputs})
        res = {"ret": ret}
        for k in out:
            raw = out[k].download(guard[k].shape, np.uint8)
            assert (raw[:8] == 0x5A).all() and (raw[-8:] == 0x5A).all(), k
            res[k] = raw[8:-8].view(OUT[k]).reshape(shape[k]).copy()
        return res
    finally:
        for b in bufs:
            b.free()


def both(ctx, c, ref=None, outputs=OPTIONAL, stop=None):
    ref = R.local_ba(c, c["params"]) if ref is None else ref
    keys = REQUIRED + tuple(outputs)
    h = host(ctx, c, outputs, stop)
    same(h, ref, keys)
    assert h["ret"] == ref["ret"]
    d = dev(ctx, c, outputs, stop)
    same(d, ref, keys)
    assert d["ret"] == ref["ret"]
    return h, ref


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 5), (5, 3, 300)])
def test_shapes(ctx, shape, kind):
    c = R.scene(100 + shape[2], *shape, kind=kind, gross=0.1)
    h, ref = both(ctx, c)
    assert ref["stats"][0] >= 1


def test_long_pose_lists(ctx):
    """every point seen by all four keyframes: 4400 edges, per-pose lists and Schur pair lists past 1024"""
    c = R.scene(3, 3, 1, 1100, all_see=True)
    c["params"] = R.params(iterations=3)
    h, ref = both(ctx, c)
    assert len(c["edge_point"]) == 4400 and ref["stats"][6] == 3300 and ref["stats"][7] == 6600


def test_full_factorisation(ctx):
    """64 free poses, four edges per point spread so every pose is used: the full 384-row factorisation"""
    c = R.scene(2, 64, 2, 400)
    c["params"] = R.params(iterations=2)
    assert set(c["edge_kf"].tolist()) == set(range(66))
    both(ctx, c)


def test_no_points(ctx):
    both(ctx, R.scene(5, 1, 1, 0))


def test_no_free_pose(ctx):
    """no free pose: nothing to solve, and the points still move"""
    c = R.scene(6, 0, 2, 10)
    h, ref = both(ctx, c)
    assert h["pose"].shape == (0, 7) and not np.array_equal(h["point_f32"], c["xw"])


# ---------------------------------------------------------------- 2. optional outputs
def test_null_optional_outputs(ctx):
    c = R.scene(7, 3, 2, 50, gross=0.1)
    ref = R.local_ba(c, c["params"])
    both(ctx, c, ref, outputs=())
    both(ctx, c, ref, outputs=("chi2",))
    a = padded(c)
    r = ctx.local_ba(lib_params(c), c["P"], c["F"], c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"], c["kpts"], c["xw"],
                     c["edge_point"], c["edge_kf"], c["edge_feat"], octave=None, uright=None)
    c2 = dict(c, octave=None, uright=None)
    same(r, R.local_ba(c2, c["params"]), REQUIRED + OPTIONAL)
    assert a["kpts"].shape[0] == len(c["kpts"]) + PAD


# ---------------------------------------------------------------- 3. forced paths
@pytest.mark.parametrize("name", ["one_trial", "stale", "exact", "behind", "nan", "fixed_only", "single_edge", "idle_pose", "lambda100",
                                  "zero_iterations"])
def test_forced(ctx, name):
    c = R.forced(name)
    h, ref = both(ctx, c)
    f = int(ref["stats"][5])
    if name == "one_trial":
        assert list(ref["stats"][:3]) == [1, 1, 1] and f & R.FLAG_ENDED_REJECTED
    elif name == "stale":
        assert list(ref["stats"][:3]) == [1, 2, 2] and f & R.FLAG_ENDED_REJECTED
    elif name == "exact":
        assert ref["stats"][0] == 1 and ref["stats"][1] == 1 and ref["erase"].sum() == 0
    elif name == "behind":
        assert ref["erase"][c["edge_point"] == c["special"]].any()
    elif name == "nan":
        assert f & R.FLAG_NONFINITE and np.array_equal(h["pose_f32"], R.local_ba(c, R.params(iterations=0))["pose_f32"])
    elif name == "zero_iterations":
        assert f & R.FLAG_NO_ITERATION and ref["stats"][0] == 0


def test_stop_preset(ctx):
    c = R.forced("stop")
    stop = np.ones(1, np.uint8)
    h, ref = both(ctx, c, stop=stop)
    assert ref["stats"][0] == 0 and int(ref["stats"][5]) & R.FLAG_STOPPED and int(ref["stats"][5]) & R.FLAG_NO_ITERATION
    # a cleared flag behind the pointer changes nothing
    c2 = dict(c, params=R.params())
    both(ctx, c2, stop=np.zeros(1, np.uint8))


def test_threshold_edges(ctx):
    """iterations = 0: one edge planted at the double next below th2, at th2 and next above: kept, kept, erased, for both thresholds"""
    for stereo in (False, True):
        for which, want in (("below", 0), ("at", 0), ("above", 1)):
            c, e = R.threshold_case(stereo, which)
            h, ref = both(ctx, c)
            assert ref["erase"][e] == want and h["erase"][e] == want, (stereo, which)


# ---------------------------------------------------------------- 4. the grow-only workspace
def test_back_to_back(ctx):
    """two calls on one ctx, the second smaller: what the first left in the workspace must not reach the second"""
    big, small = R.scene(8, 6, 2, 200, gross=0.1), R.scene(9, 2, 1, 20)
    rb, rs = R.local_ba(big, big["params"]), R.local_ba(small, small["params"])
    both(ctx, big, rb)
    both(ctx, small, rs)
    both(ctx, big, rb)


# ---------------------------------------------------------------- 5. refusals
def bad_cases():
    base = R.scene(10, 3, 2, 30)
    out = {}
    c = dict(base); ep = base["edge_point"].copy(); ep[[4, 5]] = ep[[5, 4]]; ek = base["edge_kf"].copy(); ek[[4, 5]] = ek[[5, 4]]
    c["edge_point"], c["edge_kf"] = ep, ek
    out["unsorted"] = c
    c = dict(base); ek = base["edge_kf"].copy(); ek[7] = ek[6]; c["edge_kf"] = ek
    out["duplicate"] = c
    c = dict(base); ep = base["edge_point"].copy(); ep[-1] = 30; c["edge_point"] = ep
    out["point_range"] = c
    c = dict(base); ek = base["edge_kf"].copy(); ek[-1] = 5; c["edge_kf"] = ek
    out["kf_range"] = c
    c = dict(base); ef = base["edge_feat"].copy(); ef[3] = 1 << 20; c["edge_feat"] = ef
    out["feat_range"] = c
    c = dict(base); ef = base["edge_feat"].copy(); ef[3] = -1; c["edge_feat"] = ef
    out["feat_negative"] = c
    c = dict(base); off = base["kf_feat_off"].copy(); off[2] = off[1] - 1; c["kf_feat_off"] = off
    out["offsets"] = c
    c = dict(base); nl = base["kf_nlevels"].copy(); nl[1] = 17; c["kf_nlevels"] = nl
    out["nlevels"] = c
    return out


@pytest.mark.parametrize("name", ["unsorted", "duplicate", "point_range", "kf_range", "feat_range", "feat_negative", "offsets", "nlevels"])
def test_refused_tables(ctx, name):
    """the host form checks on the host, the device form in its first kernel; nothing is written"""
    from rover_slam_amd import capi
    c = bad_cases()[name]
    with pytest.raises(R.Invalid):
        R.local_ba(c, c["params"])
    with pytest.raises(capi.RfeError):
        host(ctx, c)
    with pytest.raises(capi.RfeError):
        dev(ctx, c)
    good = R.scene(10, 3, 2, 30)
    both(ctx, good)                              # the ctx is usable afterwards


def test_refused_arguments(ctx):
    from rover_slam_amd import capi
    c = R.scene(11, 2, 1, 10)
    for P in (R.params(iterations=-1), R.params(iterations=65), R.params(max_trials=-1), R.params(th2_mono=np.nan), R.params(user_lambda_init=np.inf)):
        with pytest.raises(capi.RfeError):
            host(ctx, dict(c, params=P))
        with pytest.raises(capi.RfeError):
            dev(ctx, dict(c, params=P))
    lp = lib_params(c)
    z = np.zeros(8, np.int32)
    K = 3
    args = (c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"], c["kpts"], c["xw"], c["edge_point"], c["edge_kf"], c["edge_feat"])
    for Pn, Fn in ((65, 1), (0, 0), (-1, 2), (64, 193)):        # over the caps
        with pytest.raises(capi.RfeError):
            ctx.local_ba(lp, Pn, Fn, *args)
    for shape in ((R.MAX_POINTS + 1, 0, 0), (0, R.MAX_EDGES + 1, 0), (0, 0, -1)):
        with pytest.raises(capi.RfeError):
            ctx.local_ba(lp, 2, 1, *args, shape=shape)
    assert K == c["P"] + c["F"] and z.sum() == 0
