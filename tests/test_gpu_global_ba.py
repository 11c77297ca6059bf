"""GPU: Optimizer::GlobalBundleAdjustemnt on the device (rfe_global_ba / _dev) against the contract of DESIGN.md 6n restated in
tests/global_ba_ref.py.  Every comparison is exact (np.array_equal on pose and point in double, their float casts, included, chi2, trace
and stats), in host and device form, with poisoned padding behind E, L and Nf and guard words round every output of the device form."""
import numpy as np
import pytest

import essential_graph_ref as EG
import global_ba_ref as G
import local_ba_ref as LR

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUT = {"pose": F64, "pose_f32": F32, "point": F64, "point_f32": F32, "included": np.uint8, "chi2": F64, "trace": F64, "stats": np.int32}
OPTIONAL = ("pose_f32", "point_f32", "chi2", "trace")
REQUIRED = ("pose", "point", "included", "stats")
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
    return capi.global_ba_params(p["iterations"], p["max_trials"], p["user_lambda_init"], p["robust"], p["huber2_mono"], p["huber2_stereo"], stop)


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
    return ctx.global_ba(lib_params(c, stop), c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"], c["fixed"], a["kpts"],
                         a["xw"], a["edge_point"], a["edge_kf"], a["edge_feat"], octave=a["octave"], uright=a["uright"], outputs=outputs,
                         shape=shape_of(c))


def dev(ctx, c, outputs=OPTIONAL, stop=None, pose_in=None, xw_in=None):
    """rfe_global_ba_dev on uploaded copies; returns the host form's dict.  Every output sits between two guard words that must survive;
    when the call is refused every output must read back as uploaded, and the refusal is raised again.
    pose_in / xw_in: device addresses to take kf_pose / xw from instead"""
    a = padded(c)
    L, E, Nf = shape_of(c)
    K, its = len(c["fixed"]), max(c["params"]["iterations"], 0)
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(x.nbytes + 64))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    shape = {"pose": (K, 7), "pose_f32": (K, 7), "point": (L, 3), "point_f32": (L, 3), "included": (L,), "chi2": (E,), "trace": (its, 4), "stats": (8,)}
    fill = {"pose": 3, "pose_f32": 3, "point": 3, "point_f32": 3, "included": 9, "chi2": -3, "trace": 5, "stats": 77}
    guard = {k: np.concatenate([np.full(8, 0x5A, np.uint8), np.full(shape[k], fill[k], OUT[k]).view(np.uint8).ravel(), np.full(8, 0x5A, np.uint8)])
             for k in REQUIRED + tuple(outputs)}
    out = {k: up(g, np.uint8) for k, g in guard.items()}
    try:
        kp = up(c["kf_pose"], F32) if pose_in is None else pose_in
        xw = up(a["xw"], F32) if xw_in is None else xw_in
        ins = [kp, up(c["kf_cam"], F32), up(c["kf_nlevels"], np.int32), up(c["kf_sigma2"], F32), up(c["kf_feat_off"], np.int32),
               up(c["fixed"], np.uint8), up(a["kpts"], F32), xw, up(a["edge_point"], np.int32), up(a["edge_kf"], np.int32), up(a["edge_feat"], np.int32)]
        oc, ur = up(a["octave"], np.int32), up(a["uright"], F32)
        from rover_slam_amd import capi
        try:
            ret = ctx.global_ba_dev(lib_params(c, stop), K, L, E, Nf, *ins, out["pose"].ptr + 8, out["point"].ptr + 8, out["included"].ptr + 8,
                                    out["stats"].ptr + 8, octave=oc, uright=ur, **{k: out[k].ptr + 8 for k in outputs})
        except capi.RfeError:
            for k in out:                        # a refusal writes nothing: guard words and fill values are as uploaded
                assert np.array_equal(out[k].download(guard[k].shape, np.uint8), guard[k]), k
            raise
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
    ref = G.global_ba(c, G.run_params(c)) if ref is None else ref
    keys = REQUIRED + tuple(outputs)
    h = host(ctx, c, outputs, stop)
    same(h, ref, keys)
    assert h["ret"] == ref["ret"]
    d = dev(ctx, c, outputs, stop)
    same(d, ref, keys)
    assert d["ret"] == ref["ret"]
    return h, ref


def with_params(c, **kw):
    c = dict(c)
    c["params"] = G.params(**kw)
    return c


# ---------------------------------------------------------------- 1. the number of free poses, round one and two tiles
@pytest.mark.parametrize("P", [0, 1, 3, 4, 5, 8, 9])
def test_free_poses(ctx, P):
    K = P + 1
    c = with_params(G.scene(200 + P, K, [K // 2], G.pattern("dense", K, ppk=6, seed=P), "mixed"), iterations=4)
    h, ref = both(ctx, c)
    assert ref["stats"][5] == P and ref["stats"][7] == ((P + 3) // 4) * ((P + 3) // 4 + 1) // 2


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("P", [65, 70])
def test_past_one_workgroup(ctx, P, robust):
    """more free poses than rfe_local_ba's one-workgroup factorisation takes"""
    K = P + 1
    c = with_params(G.scene(300 + P, K, [0], G.pattern("loop", K, ppk=2), "mixed", ring=True, gross=0.1 if robust else 0.0), iterations=3, robust=robust)
    h, ref = both(ctx, c)
    assert ref["stats"][5] == P > LR.MAX_FREE and ref["stats"][0] >= 1


# ---------------------------------------------------------------- 2. patterns
@pytest.mark.parametrize("name,K,sparse", [("chain", 30, True), ("loop", 30, True), ("star", 30, True), ("hub", 30, False), ("dense", 14, False)])
def test_patterns(ctx, name, K, sparse):
    """a chain, the chain closed by a loop (fill in the last tile row), a star with the hub last, the same with the hub first (the fill is
    dense), a dense pattern"""
    c = with_params(G.scene(400 + K, K, [0] if name != "hub" else [K - 1], G.pattern(name, K, ppk=3, seed=1), "mixed", ring=name == "loop"), iterations=3)
    h, ref = both(ctx, c)
    assert (ref["stats"][6] < ref["stats"][7]) == sparse, ref["stats"]
    if name == "loop":
        chain = G.Structure(G.scene(400 + K, K, [0], G.pattern("chain", K, ppk=3), "mixed"))
        assert ref["stats"][6] > chain.tiles


def test_long_chain(ctx):
    """260 keyframes in a chain with three points per keyframe: past 256 keyframes, 65 tiles a side"""
    K = 260
    c = with_params(G.scene(5, K, [0], G.pattern("chain", K, ppk=3), "mixed"), iterations=2)
    h, ref = both(ctx, c, outputs=("pose_f32", "trace"))
    assert ref["stats"][5] == 259 and ref["stats"][6] < ref["stats"][7] // 8


def test_many_points(ctx):
    """16 400 points with two observations each on five keyframes: past rfe_local_ba's point cap; pose and pair lists of thousands, which
    the ordering kernel merges from sorted runs by rank"""
    c = with_params(G.scene(6, 5, [], G.pattern("pairs5", 5, ppk=16400), "mono", spacing=0.6), iterations=2)
    h, ref = both(ctx, c, outputs=("point_f32",))
    assert len(c["xw"]) == 16400 > LR.MAX_POINTS and len(c["edge_point"]) == 32800


@pytest.mark.parametrize("where", ["first", "middle", "last", "several", "shuffled"])
def test_fixed_roles(ctx, where):
    K = 11
    fixed = {"first": [0], "middle": [5], "last": [10], "several": [0, 4, 5, 10], "shuffled": [1, 3, 4, 8]}[where]
    c = with_params(G.scene(500 + len(fixed) + fixed[0], K, fixed, G.pattern("dense", K, ppk=5, seed=2), "mixed"), iterations=4)
    h, ref = both(ctx, c)
    pose_in = np.asarray(c["kf_pose"], F32).astype(F64)
    for k in fixed:                              # a fixed keyframe's row is its widened, normalised input
        assert np.allclose(h["pose"][k], pose_in[k], atol=1e-6) and np.array_equal(h["pose"][k], ref["pose"][k])
    assert not np.array_equal(h["pose_f32"][2], c["kf_pose"][2])


# ---------------------------------------------------------------- 3. forced paths
@pytest.mark.parametrize("name", [n for n in G.FORCED if n not in ("stop", "stop_after_trial")])
def test_forced(ctx, name):
    c = G.forced(name)
    h, ref = both(ctx, c)
    f = int(ref["stats"][4])
    if name == "ended_rejected":
        assert list(ref["stats"][:3]) == [1, 1, 1] and f & G.FLAG_ENDED_REJECTED
    elif name == "stale":
        assert list(ref["stats"][:3]) == [1, 2, 2] and f & G.FLAG_ENDED_REJECTED
    elif name == "rho_zero":
        assert list(ref["stats"][:2]) == [1, 1]
    elif name == "nan":
        assert f & G.FLAG_NONFINITE and f & G.FLAG_SOLVE_FAILED
    elif name == "iterations0":
        assert f & G.FLAG_NO_ITERATION and ref["stats"][0] == 0
    elif name == "all_fixed":
        assert ref["stats"][5] == 0 and ref["stats"][6] == 0 and not np.array_equal(h["point_f32"], c["xw"])
    elif name == "no_fixed":
        assert ref["stats"][5] == len(c["fixed"])
    elif name == "edgeless":
        assert h["included"][c["special"]] == 0 and h["included"].sum() == len(c["xw"]) - 2
        assert np.array_equal(h["point_f32"][c["special"]], c["xw"][c["special"]])
    elif name == "fixed_only":
        assert h["included"][c["special"]] == 1


def test_stop_preset(ctx):
    c = G.forced("stop")
    h, ref = both(ctx, c, stop=np.ones(1, np.uint8))
    assert ref["stats"][0] == 0 and int(ref["stats"][4]) & G.FLAG_STOPPED and int(ref["stats"][4]) & G.FLAG_NO_ITERATION
    both(ctx, with_params(c), stop=np.zeros(1, np.uint8))      # a cleared flag behind the pointer changes nothing


@pytest.mark.parametrize("name,trials", [("stop_after_trial", 1), ("robust", 3), ("stale", 1)])
def test_stop_seen_after_a_trial(ctx, name, trials):
    """`stop` set while the call runs, at a known trial (rfe_k_global_ba_stop_after: the library writes the caller's flag behind that
    trial, in front of the read that follows it).  After the first trial; after the third, two iterations in; after a rejected first
    trial, whose inner loop would have gone on to a second"""
    from rover_slam_amd import capi
    c = G.forced(name)
    c["params"] = dict(c["params"], stop=("after", trials))
    ref = G.global_ba(c, G.run_params(c))
    assert ref["stats"][1] == trials and int(ref["stats"][4]) & G.FLAG_STOPPED
    unstopped = G.global_ba(c, dict(c["params"], stop=False))
    assert unstopped["stats"][1] > trials and not int(unstopped["stats"][4]) & G.FLAG_STOPPED
    for form in (host, dev):
        flag = np.zeros(1, np.uint8)
        ctx._chk(capi.lib.rfe_k_global_ba_stop_after(ctx.h, trials))
        got = form(ctx, c, stop=flag)
        same(got, ref, REQUIRED + OPTIONAL)
        assert got["ret"] == ref["ret"] and flag[0] == 1
    got = dev(ctx, c, stop=np.zeros(1, np.uint8))     # one shot: the next call runs to its end
    same(got, unstopped, REQUIRED + OPTIONAL)


def test_null_optional_outputs(ctx):
    c = G.forced("robust")
    ref = G.global_ba(c, c["params"])
    both(ctx, c, ref, outputs=())
    both(ctx, c, ref, outputs=("chi2",))
    r = ctx.global_ba(lib_params(c), c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"], c["fixed"], c["kpts"], c["xw"],
                      c["edge_point"], c["edge_kf"], c["edge_feat"], octave=None, uright=None)
    same(r, G.global_ba(dict(c, octave=None, uright=None), c["params"]), REQUIRED + OPTIONAL)


# ---------------------------------------------------------------- 4. the grow-only workspaces
def test_back_to_back(ctx):
    """two calls on one ctx, the second smaller: what the first left in the workspaces (the matrix's tiles among them) must not reach it"""
    big = with_params(G.scene(8, 20, [0], G.pattern("dense", 20, ppk=6, seed=4), "mixed"), iterations=3)
    small = with_params(G.scene(9, 6, [3], G.pattern("chain", 6, ppk=2), "mixed"), iterations=3)
    rb, rs = G.global_ba(big, big["params"]), G.global_ba(small, small["params"])
    both(ctx, big, rb)
    both(ctx, small, rs)
    both(ctx, big, rb)


# ---------------------------------------------------------------- 5. against rfe_local_ba, and behind rfe_essential_graph
@pytest.mark.parametrize("shape", [(5, 3, 120), (64, 2, 400), (7, 0, 60)])
def test_equals_local_ba(ctx, shape):
    """robust with the fixed keyframes last and equal Huber parameters: rfe_local_ba's bits, from the same ctx"""
    from rover_slam_amd import capi
    c = LR.scene(600 + shape[0], *shape, kind="mixed", gross=0.1)
    c["params"] = LR.params(iterations=4)
    p = c["params"]
    l = ctx.local_ba(capi.local_ba_params(p["iterations"], p["max_trials"], p["user_lambda_init"], p["th2_mono"], p["th2_stereo"]), c["P"], c["F"],
                     c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"], c["kpts"], c["xw"], c["edge_point"], c["edge_kf"],
                     c["edge_feat"], octave=c["octave"], uright=c["uright"])
    g = G.from_local(c)
    h, ref = both(ctx, g)
    P = c["P"]
    for k in ("pose", "pose_f32"):
        assert np.array_equal(h[k][:P], l[k])
    for k in ("point", "point_f32", "chi2", "trace"):
        assert np.array_equal(h[k], l[k]), k
    assert np.array_equal(h["stats"][:4], l["stats"][:4])


def test_behind_essential_graph(ctx):
    """rfe_essential_graph_dev's tiw_f32 and xw_out go to rfe_global_ba_dev without leaving the device"""
    from rover_slam_amd import capi
    K = 9
    c = with_params(G.scene(7, K, [0], G.pattern("loop", K, ppk=4), "mixed", ring=True), iterations=3)
    L = len(c["xw"])
    rng = np.random.default_rng(3)
    s_est = np.concatenate([np.asarray(c["kf_pose"], F32).astype(F64), np.ones((K, 1))], 1)
    s_meas = s_est.copy()
    s_meas[:, 4:7] += 1e-3 * rng.standard_normal((K, 3))
    e = {"s_est": s_est, "s_meas": s_meas, "fixed": c["fixed"], "edge_i": np.arange(K - 1, dtype=np.int32), "edge_j": np.arange(1, K, dtype=np.int32),
         "edge_from_est": np.zeros(K - 1, np.uint8), "xw": c["xw"], "point_ref": (np.arange(L) % (K + 1) - 1).astype(np.int32)}
    eref = EG.essential_graph(e, EG.params(iterations=3))
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(x.nbytes + 64))
        return bufs[-1].upload(x)
    try:
        tiw, xwo = ctx.alloc(K * 7 * 4 + 64), ctx.alloc(L * 3 * 4 + 64)
        siw, st = ctx.alloc(K * 64 + 64), ctx.alloc(64)
        bufs += [tiw, xwo, siw, st]
        ctx.essential_graph_dev(capi.essential_graph_params(3), K, K - 1, L, up(e["s_est"], F64), up(e["s_meas"], F64), up(e["fixed"], np.uint8),
                                up(e["edge_i"], np.int32), up(e["edge_j"], np.int32), up(e["edge_from_est"], np.uint8), up(e["xw"], F32),
                                up(e["point_ref"], np.int32), siw, xwo, st, tiw_f32=tiw)
        c2 = dict(c, kf_pose=eref["tiw_f32"], xw=eref["xw_out"])
        ref = G.global_ba(c2, c2["params"])
        d = dev(ctx, c2, pose_in=tiw, xw_in=xwo)
        same(d, ref, REQUIRED + OPTIONAL)
        assert not np.array_equal(eref["tiw_f32"], c["kf_pose"])
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------- 6. refusals
def bad_cases():
    K = 5
    base = G.scene(10, K, [0], G.pattern("dense", K, ppk=6, seed=5))
    out = {}
    c = dict(base); ep = base["edge_point"].copy(); ep[[4, 5]] = ep[[5, 4]]; ek = base["edge_kf"].copy(); ek[[4, 5]] = ek[[5, 4]]
    c["edge_point"], c["edge_kf"] = ep, ek
    out["unsorted"] = c
    c = dict(base); ek = base["edge_kf"].copy(); ek[1] = ek[0]; c["edge_kf"] = ek
    out["duplicate"] = c
    c = dict(base); ep = base["edge_point"].copy(); ep[-1] = len(base["xw"]); c["edge_point"] = ep
    out["point_range"] = c
    c = dict(base); ek = base["edge_kf"].copy(); ek[-1] = K; c["edge_kf"] = ek
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
    """the host form checks on the host, the device form in its first kernel; nothing is written (dev() reads every output back after a
    refusal and compares it with what it uploaded)"""
    from rover_slam_amd import capi
    c = bad_cases()[name]
    with pytest.raises(G.Invalid):
        G.global_ba(c, c["params"])
    with pytest.raises(capi.RfeError):
        host(ctx, c)
    with pytest.raises(capi.RfeError):
        dev(ctx, c)
    both(ctx, with_params(G.scene(10, 5, [0], G.pattern("dense", 5, ppk=6, seed=5)), iterations=2))      # the ctx is usable afterwards


def test_refused_arguments(ctx):
    from rover_slam_amd import capi
    c = G.scene(11, 3, [0], G.pattern("dense", 3, ppk=4, seed=6))
    for P in (dict(iterations=-1), dict(iterations=65), dict(max_trials=-1), dict(huber2_mono=np.nan), dict(huber2_stereo=np.inf),
              dict(user_lambda_init=np.inf)):
        with pytest.raises(capi.RfeError):
            host(ctx, with_params(c, **P))
        with pytest.raises(capi.RfeError):
            dev(ctx, with_params(c, **P))
    lp = lib_params(c)
    args = (c["kf_pose"], c["kf_cam"], c["kf_nlevels"], c["kf_sigma2"], c["kf_feat_off"])
    rest = (c["kpts"], c["xw"], c["edge_point"], c["edge_kf"], c["edge_feat"])
    buf = ctx.alloc(1 << 16)                     # a NULL `fixed`: refused by the argument check, before anything is read or launched
    try:
        with pytest.raises(capi.RfeError, match="null pointer"):
            ctx.global_ba_dev(lp, 3, len(c["xw"]), len(c["edge_point"]), len(c["kpts"]), buf, buf, buf, buf, buf, None, buf, buf, buf, buf, buf,
                              buf, buf, buf, buf)
    finally:
        buf.free()
    with pytest.raises(capi.RfeError):           # K = 0
        ctx.global_ba(lp, *args, np.zeros(0, np.uint8), *rest)
    with pytest.raises(capi.RfeError):           # K over the cap
        ctx.global_ba(lp, *args, np.zeros(G.MAX_KF + 1, np.uint8), *rest)
    for shape in ((G.MAX_POINTS + 1, 0, 0), (0, G.MAX_EDGES + 1, 0), (0, 0, -1)):
        with pytest.raises(capi.RfeError):
            ctx.global_ba(lp, *args, c["fixed"], *rest, shape=shape)


def test_refused_pairs(ctx):
    """more Schur pair entries than the cap: 520 keyframes all seeing 250 points is 250 * 520 * 521 / 2 = 33.9 million; the restatement and
    both forms refuse before any output is written, the device form after its counting kernels"""
    from rover_slam_amd import capi
    big = G.over_pairs_case()
    assert G.schur_pairs(big) > G.MAX_PAIRS and len(big["edge_point"]) <= G.MAX_EDGES and len(big["fixed"]) <= G.MAX_KF
    with pytest.raises(G.Invalid, match="pairs"):
        G.global_ba(big, big["params"])
    with pytest.raises(capi.RfeError, match="pair"):
        host(ctx, big)
    with pytest.raises(capi.RfeError, match="pair"):
        dev(ctx, big)
