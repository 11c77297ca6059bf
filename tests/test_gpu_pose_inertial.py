"""GPU: Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame on the device (rfe_pose_inertial_optimization / _dev) against the
contract of DESIGN.md 6p restated in tests/pose_inertial_ref.py.  Every comparison is exact (np.array_equal on the state in double, its
float cast, outlier, chi2, prior_out, trace and stats), in host and device form, with padded capacity and poisoned padding."""
import ctypes

import numpy as np
import pytest

import pose_inertial_ref as R
import pose_opt_ref as PO

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUT = {"state": F64, "state_f32": F32, "outlier": np.uint8, "chi2": F32, "prior_out": F64, "trace": F64, "stats": np.int32}
OPTIONAL = ("state_f32", "chi2", "prior_out", "trace")
KINDS = ("mono", "stereo", "mixed")
SENTINEL, CHI2_SENTINEL = 7, F32(-3.0)
KF, LF = R.MODE_LAST_KEYFRAME, R.MODE_LAST_FRAME
SMALL = {"mode": np.int32, "rec_init": np.int32, "cam": F32, "state": F32, "prev_state": F32, "preint": F32, "cov_rw": F32}
ROWS = {"kpts": F32, "octave": np.int32, "uright": F32, "xw": F32, "has_mp": np.uint8, "track_depth": F32}


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def to_capi(P):
    from rover_slam_amd import capi
    return capi.pose_inertial_params(P["fx"], P["fy"], P["cx"], P["cy"], P["bf"], P["inv_level_sigma2"])


def batch(cases, N=None, poison=True, seed=0):
    """B cases stacked to [B, N]: case b keeps its n features in front, the rows behind are padding -- poisoned with NaN positions, huge
    octaves, NaN depths and set has_mp when `poison`.  A LastKeyFrame case's prior row is NaN."""
    rng = np.random.default_rng(seed)
    B = len(cases)
    args = [c["args"] for c in cases]
    N = max(len(x["has_mp"]) for x in args) if N is None else N
    a = {k: np.stack([np.asarray(x[k], dt) for x in args]) for k, dt in SMALL.items()}
    a["prior_in"] = np.stack([np.asarray(x["prior_in"], F64) if x["prior_in"] is not None else np.full(R.PRIOR_DOUBLES, np.nan) for x in args])
    a.update({"kpts": np.zeros((B, N, 2), F32), "octave": np.zeros((B, N), np.int32), "uright": np.full((B, N), -1, F32), "xw": np.zeros((B, N, 3), F32),
              "has_mp": np.zeros((B, N), np.uint8), "track_depth": np.zeros((B, N), F32), "n": np.array([len(x["has_mp"]) for x in args], np.int32)})
    if poison:
        a["kpts"][:], a["xw"][:], a["octave"][:], a["has_mp"][:], a["track_depth"][:] = np.nan, np.nan, 1 << 30, 1, np.nan
        a["uright"][:] = rng.choice(np.array([-1, np.nan, 50], F32), (B, N))
    for b, x in enumerate(args):
        n = len(x["has_mp"])
        for k in ROWS:
            a[k][b, :n] = x[k]
    return a


def reference_one(P, a, b, with_n=True):
    N = a["has_mp"].shape[1]
    return R.pose_inertial_optimization(P, a["mode"][b], a["rec_init"][b], a["cam"][b], a["state"][b], a["prev_state"][b], a["preint"][b],
                                        a["cov_rw"][b], a["prior_in"][b], a["kpts"][b], a["octave"][b], a["uright"][b], a["xw"][b], a["has_mp"][b],
                                        a["track_depth"][b], a["n"][b] if with_n else None, np.full(N, SENTINEL, np.uint8),
                                        np.full(N, CHI2_SENTINEL, F32))


def reference(P, a, with_n=True):
    rs = [reference_one(P, a, b, with_n) for b in range(len(a["mode"]))]
    return {k: np.stack([np.asarray(r[k]) for r in rs]) for k in OUT}


def same(got, ref, keys=tuple(OUT)):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.argwhere(got[k] != ref[k])[:8], got[k].ravel()[:8], ref[k].ravel()[:8])


def host(ctx, P, a, outputs=OPTIONAL, with_n=True, octave=True, uright=True, rec_init=True):
    B, N = a["has_mp"].shape
    return ctx.pose_inertial_optimization(to_capi(P), a["mode"], a["cam"], a["state"], a["prev_state"], a["preint"], a["cov_rw"], a["kpts"], a["xw"],
                                          a["has_mp"], a["track_depth"], prior_in=a["prior_in"], rec_init=a["rec_init"] if rec_init else None,
                                          octave=a["octave"] if octave else None, uright=a["uright"] if uright else None,
                                          n=a["n"] if with_n else None, outlier=np.full((B, N), SENTINEL, np.uint8),
                                          chi2=np.full((B, N), CHI2_SENTINEL, F32), outputs=outputs)


def shapes(B, N):
    return {"state": (B, 21), "state_f32": (B, 21), "outlier": (B, N), "chi2": (B, N), "prior_out": (B, 246), "trace": (B, 4, 8), "stats": (B, 16)}


def dev(ctx, P, a, outputs=OPTIONAL, with_n=True, octave=True, uright=True, rec_init=True, prev_buf=None, prior_buf=None, keep=None, prior=True):
    """rfe_pose_inertial_optimization_dev on uploaded copies; returns the host form's dict.  prev_buf / prior_buf: device buffers to read
    prev_state / prior_in from; keep: a dict that receives the state_f32 and prior_out buffers instead of their being freed (the chain)"""
    B, N = a["has_mp"].shape
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    shape = shapes(B, N)
    fill = {"state": 0, "state_f32": 0, "outlier": SENTINEL, "chi2": CHI2_SENTINEL, "prior_out": 3, "trace": 5, "stats": 77}
    out = {k: up(np.full(shape[k], fill[k], OUT[k]), OUT[k]) for k in ("state", "outlier", "stats") + tuple(outputs)}
    try:
        ctx.pose_inertial_optimization_dev(
            to_capi(P), up(a["mode"], np.int32), up(a["cam"], F32), up(a["state"], F32), prev_buf if prev_buf is not None else up(a["prev_state"], F32),
            up(a["preint"], F32), up(a["cov_rw"], F32), up(a["kpts"], F32), up(a["xw"], F32), up(a["has_mp"], np.uint8), up(a["track_depth"], F32),
            B, N, out["state"], out["outlier"], out["stats"], prior_in=(prior_buf if prior_buf is not None else up(a["prior_in"], F64)) if prior else None,
            rec_init=up(a["rec_init"], np.int32) if rec_init else None, octave=up(a["octave"], np.int32) if octave else None,
            uright=up(a["uright"], F32) if uright else None, n=up(a["n"], np.int32) if with_n else None,
            **{k: out[k] for k in outputs})
        ctx.synchronize()
        return {k: out[k].download(shape[k], OUT[k]) if np.prod(shape[k]) else np.zeros(shape[k], OUT[k]) for k in out}
    finally:
        for b in bufs:
            if keep is not None and b is out.get("state_f32"):
                keep["state_f32"] = b
            elif keep is not None and b is out.get("prior_out"):
                keep["prior_out"] = b
            else:
                b.free()


def both(ctx, P, a, ref=None, **kw):
    ref = reference(P, a, kw.get("with_n", True)) if ref is None else ref
    h = host(ctx, P, a, **kw)
    same(h, ref)
    same(dev(ctx, P, a, **kw), ref)
    return h, ref


# ---------------------------------------------------------------- 1. sizes and kinds: both modes in one call
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [0, 1, 5, 6, 7, 255, 256, 257, 1023, 4096])
def test_sizes_and_kinds(ctx, N, kind):
    small = N < 20
    cases = [R.scene(300 + N, N, mode, kind, has=1.0 if small else 0.9, gross=0.0 if small else 0.2) for mode in (KF, LF)]
    a = batch(cases, N=min(N + 3, 4096))
    h, ref = both(ctx, cases[0]["P"], a)
    st = ref["stats"]
    assert (st[:, 5] == [1 if N + 3 < 10 else 4, 1 if N + 4 < 10 else 4]).all()      # the fewer-than-10-edges break counts the 3 / 4 other edges
    if N >= 255:                                   # the scene is a real one: four rounds of ten iterations, most edges inliers, some outliers
        assert (st[:, 6] == 40).all() and (st[:, 0] > N // 2).all() and (0 < st[:, 2]).all() and (st[:, 2] < N // 2).all()
        for b, c in enumerate(cases):
            d0, d1 = R.state_distance(c["args"]["state"], c["truth"]), R.state_distance(h["state"][b], c["truth"])
            assert d1[0] < d0[0] / 5
    print(f"N={N} {kind}: stats {h['stats'][:, :10].tolist()}")


# ---------------------------------------------------------------- 2. several problems, each with its own n and mode
def test_batch_of_three(ctx):
    cases = [R.scene(40, 300, LF), R.scene(41, 0, KF), R.scene(42, 41, LF, dT=0.5)]
    a = batch(cases, N=300)
    assert list(a["n"]) == [300, 0, 41] and np.isnan(a["xw"][2, 41:]).all() and a["has_mp"][1].all()
    h, ref = both(ctx, cases[0]["P"], a)
    assert len({p.tobytes() for p in ref["state"]}) == 3
    for b, c in enumerate(cases):                  # the sentinel survives wherever has_mp == 0 and behind n
        n, hm = len(c["args"]["has_mp"]), c["args"]["has_mp"]
        assert (h["outlier"][b, n:] == SENTINEL).all() and (h["outlier"][b, :n][hm == 0] == SENTINEL).all()
        assert (h["outlier"][b, :n][hm != 0] <= 1).all() and (h["chi2"][b, n:] == CHI2_SENTINEL).all()
    assert h["ret"] == ref["stats"][0, 0]          # the host form returns problem 0's count


def test_batch_of_sixty_four(ctx):
    """eight different problems (both modes, n from 0 to 150), each in eight slots: the restatement runs once per problem"""
    base = [R.scene(50 + k, n, mode, kind) for k, (n, mode, kind) in enumerate(((150, LF, "mixed"), (0, LF, "mono"), (33, KF, "stereo"), (97, KF, "mixed"),
                                                                              (5, LF, "mixed"), (150, KF, "mono"), (64, LF, "stereo"), (7, KF, "mixed")))]
    order = [(3 * s + s // 8) % 8 for s in range(64)]
    a = batch([base[k] for k in order], N=160)
    one = [reference_one(base[0]["P"], a, order.index(k)) for k in range(8)]
    ref = {key: np.stack([np.asarray(one[k][key]) for k in order]) for key in OUT}
    both(ctx, base[0]["P"], a, ref=ref)


def test_n_null_is_all_rows_and_optional_inputs(ctx):
    cases = [R.scene(61, 200, LF, "mono"), R.scene(62, 200, KF, "mono")]
    a = batch(cases, poison=False)
    P = cases[0]["P"]
    both(ctx, P, a, with_n=False)
    # octave = NULL reads level 0, uright = NULL is all mono, rec_init = NULL is 0
    z = dict(a, octave=np.zeros_like(a["octave"]), uright=np.full_like(a["uright"], -1))
    ref = reference(P, z)
    same(host(ctx, P, a, octave=False, uright=False, rec_init=False), ref)
    same(dev(ctx, P, a, octave=False, uright=False, rec_init=False), ref)


def test_optional_outputs_null(ctx):
    cases = [R.scene(64, 120, LF), R.scene(65, 120, KF)]
    a = batch(cases)
    ref = reference(cases[0]["P"], a)
    for outputs in ((), ("chi2",), ("state_f32", "trace"), ("prior_out",)):
        keys = ("state", "outlier", "stats") + outputs
        same(host(ctx, cases[0]["P"], a, outputs=outputs), ref, keys)
        same(dev(ctx, cases[0]["P"], a, outputs=outputs), ref, keys)


def test_back_to_back_calls(ctx):
    """two different calls on one ctx, then the first again: nothing of a call survives into the next"""
    c1, c2 = [R.scene(66, 257, LF)], [R.scene(67, 90, KF), R.scene(68, 90, LF, "stereo")]
    a1, a2 = batch(c1), batch(c2)
    r1, r2 = reference(c1[0]["P"], a1), reference(c1[0]["P"], a2)
    same(dev(ctx, c1[0]["P"], a1), r1)
    same(dev(ctx, c1[0]["P"], a2), r2)
    same(host(ctx, c1[0]["P"], a1), r1)


# ---------------------------------------------------------------- 3. the forced paths of the CPU tests
@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(ctx, name):
    c = R.forced(name)
    h, ref = both(ctx, c["P"], batch([c]))
    st = ref["stats"][0]
    expect = {"failed_solve": R.FLAG_SOLVE_FAILED, "info_clipped": R.FLAG_INFO_CLIPPED, "marg_cut": R.FLAG_MARG_CUT, "huber_above": R.FLAG_PRIOR_HUBER,
              "few_edges_kf": R.FLAG_FEW_EDGES, "few_edges_f": R.FLAG_FEW_EDGES, "recovery": R.FLAG_RECOVERY, "nan": R.FLAG_NONFINITE}
    absent = {"huber_below": R.FLAG_PRIOR_HUBER, "enough_edges_kf": R.FLAG_FEW_EDGES, "enough_edges_f": R.FLAG_FEW_EDGES,
              "recovery_rec_init": R.FLAG_RECOVERY}
    assert st[8] & expect.get(name, 0) == expect.get(name, 0) and not st[8] & absent.get(name, 0)
    assert h["stats"][0, 8] == st[8]


# ---------------------------------------------------------------- 4. the resident chain: four frames through the _dev form only
def test_chain_on_the_device(ctx):
    """LastFrame, LastFrame, LastKeyFrame, LastFrame: each call's prior_out_dev / state_f32_dev is the next call's prior_in_dev /
    prev_state_dev without leaving the device; equal to the restatement run the same way"""
    ref = R.chain(70, 200, [LF, LF, KF, LF])
    assert len({r["prior_out"].tobytes() for _, r in ref}) == 4
    prev = None
    try:
        for c, r in ref:
            a = batch([c])
            keep = {}
            got = dev(ctx, c["P"], a, prev_buf=None if prev is None else prev["state_f32"], prior_buf=None if prev is None else prev["prior_out"], keep=keep)
            same(got, {k: np.asarray(r[k])[None] for k in OUT}, keys=("state", "state_f32", "prior_out", "stats", "trace"))
            hm = c["args"]["has_mp"] != 0
            assert np.array_equal(got["outlier"][0][hm], r["outlier"][hm]) and np.array_equal(got["chi2"][0][hm], r["chi2"][hm])
            if prev is not None:
                for b in prev.values():
                    b.free()
            prev = keep
    finally:
        if prev is not None:
            for b in prev.values():
                b.free()


def test_behind_pose_optimization_on_one_ctx(ctx):
    """rfe_pose_optimization_dev and the inertial entry queued on one ctx without a synchronisation between them"""
    from rover_slam_amd import capi
    pc = PO.scene(75, 300, "mixed")
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)).upload(x))
        return bufs[-1]
    try:
        pose, outl, st = up(np.zeros(7, F64), F64), up(np.zeros(300, np.uint8), np.uint8), up(np.zeros(8, np.int32), np.int32)
        P = pc["P"]
        ctx.pose_optimization_dev(capi.pose_params(P["fx"], P["fy"], P["cx"], P["cy"], P["bf"], P["inv_level_sigma2"]), up(pc["pose0"], F32),
                                  up(pc["kpts"], F32), up(pc["xw"], F32), up(pc["has_mp"], np.uint8), 1, 300, pose, outl, st,
                                  octave=up(pc["octave"], np.int32), uright=up(pc["uright"], F32))
        c = R.scene(76, 300, LF)
        a = batch([c])
        same(dev(ctx, c["P"], a), reference(c["P"], a))
        assert np.array_equal(pose.download((7,), F64), PO.solve(pc)["pose"])
    finally:
        for b in bufs:
            b.free()


def test_dev_form_flags_a_mode_it_cannot_serve(ctx):
    """the _dev form reads mode on the device: LastFrame without prior_in_dev, or an unknown mode, runs as LastKeyFrame and says so in flag 256"""
    c = R.scene(77, 120, LF)
    a = batch([c])
    ref = reference(c["P"], dict(a, prior_in=[None]))
    assert ref["stats"][0, 8] & R.FLAG_MODE and np.array_equal(ref["state"], reference(c["P"], dict(a, mode=np.array([KF], np.int32)))["state"])
    same(dev(ctx, c["P"], a, prior=False), ref)
    a5 = dict(a, mode=np.array([5], np.int32))
    ref5 = reference(c["P"], a5)
    assert ref5["stats"][0, 8] & R.FLAG_MODE
    same(dev(ctx, c["P"], a5), ref5)
    assert not reference(c["P"], a)["stats"][0, 8] & R.FLAG_MODE


# ---------------------------------------------------------------- 5. refusals
def test_refusals(ctx):
    from rover_slam_amd import capi
    c = R.scene(81, 20, LF)
    a = batch([c])
    P = c["P"]

    def refused(params=None, B=1, N=20, null=(), form="both", **arrays):
        x = dict(a, **arrays)
        p = to_capi(P) if params is None else params
        b1 = max(B, 1)
        so, sf, po = np.full((b1, 21), 9.0, F64), np.full((b1, 21), 9.0, F32), np.full((b1, 246), 9.0, F64)
        tr, st, out = np.full((b1, 32), 9.0, F64), np.full((b1, 16), 9, np.int32), np.full((max(B * N, 1),), 9, np.uint8)
        args = {"params": ctypes.byref(p)}
        for k in ("mode", "rec_init", "cam", "state", "prev_state", "preint", "cov_rw", "prior_in", "kpts", "octave", "uright", "xw", "has_mp",
                  "track_depth", "n"):
            args[k] = np.ascontiguousarray(x[k]).ctypes.data
        args.update({"B": B, "N": N, "state_out": so.ctypes.data, "state_f32": sf.ctypes.data, "outlier": out.ctypes.data, "chi2": None,
                     "prior_out": po.ctypes.data, "trace": tr.ctypes.data, "stats": st.ctypes.data})
        for k in null:
            args[k] = None
        # the _dev form checks its arguments before it touches a pointer, so host addresses do for the refusals
        fns = {"both": (capi.lib.rfe_pose_inertial_optimization, capi.lib.rfe_pose_inertial_optimization_dev),
               "host": (capi.lib.rfe_pose_inertial_optimization,)}[form]
        for fn in fns:
            assert fn(ctx.h, *args.values()) == -1 and b"pose_inertial_optimization" in capi.lib.rfe_last_error(ctx.h)     # RFE_ERR_INVALID
            for o in (so, sf, po, tr, st, out):    # nothing was written
                assert (o == 9).all()
        return True

    assert refused(B=-1) and refused(B=65) and refused(N=-1) and refused(N=4097)
    for nl in (0, 17):
        p = to_capi(P); p.nlevels = nl
        assert refused(params=p)
    for k in ("mode", "cam", "state", "prev_state", "preint", "cov_rw", "kpts", "xw", "has_mp", "track_depth", "state_out", "outlier", "stats"):
        assert refused(null=(k,))
    assert refused(form="host", mode=np.array([2], np.int32)) and refused(form="host", mode=np.array([-1], np.int32))
    assert refused(form="host", null=("prior_in",))                                  # LastFrame mode without a prior
    for dT in (0.0, -0.05, np.nan):
        pre = a["preint"].copy(); pre[0, 0] = dT
        assert refused(form="host", preint=pre)
    # B = 0 is not an error and touches nothing
    assert capi.lib.rfe_pose_inertial_optimization(ctx.h, ctypes.byref(to_capi(P)), *([a["mode"].ctypes.data] * 15), 0, 20,
                                                   *([a["prior_in"].ctypes.data] * 7)) == 0


# ---------------------------------------------------------------- 6. one chi2 planted one ulp either side of every threshold
def _planted(values, stereo, close, flagged):
    """edges whose chi2 is exactly values[k]: the identity camera pose, the point (0, 0, 1), fx = fy = 1, cx = cy = bf = 0, the observation
    (1, 0) [and uright 0]: e = (1, 0[, 0]) and chi2 = 1 (isg 1) + 0 (isg 0) = isg, the level's mvInvLevelSigma2 = values[k]"""
    m = len(values)
    P = R.params(1.0, 1.0, 0.0, 0.0, 0.0, tuple(values))
    a = {"kpts": np.tile(np.array([1, 0], F32), (m, 1)), "octave": np.arange(m, dtype=np.int32), "uright": np.full(m, 0.0 if stereo else -1.0, F32),
         "xw": np.tile(np.array([0, 0, 1], F32), (m, 1)), "track_depth": np.full(m, 5.0 if close else 20.0, F32),
         "outlier_in": np.full(m, 1 if flagged else 0, np.uint8)}
    # an edge that is not flagged is compared at the chi2 it is handed; its geometry then says something else (level 0 everywhere)
    a["chi2_in"] = np.asarray(values, F32) if not flagged else np.full(m, 1e9, F32)
    if not flagged:
        a["octave"] = np.zeros(m, np.int32)
    return P, a


def _restated(P, a, lf, rnd):
    f = R.features(P, a["kpts"], a["octave"], a["uright"], a["xw"], np.ones(len(a["octave"]), np.uint8), a["track_depth"], len(a["octave"]))
    cur = {"Rcw": np.eye(3), "tcw": np.zeros(3)}
    if rnd < 4:
        out, c2f = R.classify(P, None, cur, f, lf, rnd, a["outlier_in"] != 0, a["chi2_in"])
        return out.astype(np.uint8), c2f
    good, c2f = R.recovered(P, None, cur, f)
    return np.where(good, 0, (a["outlier_in"] != 0) | 2).astype(np.uint8), c2f


@pytest.mark.parametrize("mode", [KF, LF])
def test_chi2_one_ulp_either_side_of_every_threshold(ctx, mode):
    lf = mode == LF
    view = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    up, dn = (lambda t: np.nextafter(F32(t), F32(np.inf))), (lambda t: np.nextafter(F32(t), F32(-np.inf)))
    checked = 0
    for rnd in range(4):
        tm = (R.CHI2_MONO_F if lf else R.CHI2_MONO_KF)[rnd]
        for thr, stereo, close in ((tm, False, False), (F32(1.5 * float(tm)), False, True), (R.CHI2_STEREO[rnd], True, False)):
            values = [dn(thr), F32(thr), up(thr)]
            for flagged in (False, True):
                P, a = _planted(values, stereo, close, flagged)
                code, c2 = ctx.k_pose_inertial_classify(to_capi(P), mode, rnd, view, a["kpts"], a["xw"], a["track_depth"], a["outlier_in"], a["chi2_in"],
                                                        octave=a["octave"], uright=a["uright"])
                assert np.array_equal(c2, np.asarray(values, F32)), (rnd, thr, flagged, c2)       # the planted chi2 is what was compared
                assert code.tolist() == [0, 0, 1], (rnd, thr, stereo, close, flagged, code)           # chi2 > threshold
                ref_code, ref_c2 = _restated(P, a, lf, rnd)
                assert np.array_equal(code, ref_code) and np.array_equal(c2, ref_c2)
                checked += 1
    # the recovery pass: chi2 < 18 (mono) / 24 (stereo) clears the flag; otherwise it stays as it was and the edge counts as bad
    for thr, stereo in ((R.CHI2_MONO_OUT, False), (R.CHI2_STEREO_OUT, True)):
        values = [dn(thr), F32(thr), up(thr)]
        for flagged in (False, True):
            P, a = _planted(values, stereo, False, True)
            a["outlier_in"][:] = 1 if flagged else 0
            code, c2 = ctx.k_pose_inertial_classify(to_capi(P), mode, 4, view, a["kpts"], a["xw"], a["track_depth"], a["outlier_in"], a["chi2_in"],
                                                    octave=a["octave"], uright=a["uright"])
            assert np.array_equal(c2, np.asarray(values, F32)) and code.tolist() == [0, 2 | int(flagged), 2 | int(flagged)]
            ref_code, ref_c2 = _restated(P, a, lf, 4)
            assert np.array_equal(code, ref_code) and np.array_equal(c2, ref_c2)
            checked += 1
    assert checked == 4 * 3 * 2 + 4
    # a point behind the camera is an outlier whatever its chi2 (mono edges only), and the close rule reads mTrackDepth < 10.f
    P, a = _planted([F32(1.0)] * 4, False, False, True)
    a["xw"][1, 2] = -1.0
    a["track_depth"][:] = [20.0, 20.0, np.nextafter(F32(10), F32(0)), 10.0]
    code, _ = ctx.k_pose_inertial_classify(to_capi(P), mode, 3, view, a["kpts"], a["xw"], a["track_depth"], a["outlier_in"], a["chi2_in"],
                                           octave=a["octave"], uright=a["uright"])
    assert code.tolist() == [0, 1, 0, 0] and np.array_equal(code, _restated(P, a, lf, 3)[0])
    P, a = _planted([F32(7.0)] * 2, False, False, True)          # 5.991 < 7 < 1.5 * 5.991: an outlier when far, an inlier when close
    a["track_depth"][:] = [np.nextafter(F32(10), F32(0)), 10.0]
    code, _ = ctx.k_pose_inertial_classify(to_capi(P), mode, 3, view, a["kpts"], a["xw"], a["track_depth"], a["outlier_in"], a["chi2_in"],
                                           octave=a["octave"], uright=a["uright"])
    assert code.tolist() == [0, 1] and np.array_equal(code, _restated(P, a, lf, 3)[0])
