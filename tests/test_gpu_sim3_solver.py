"""GPU: Sim3Solver's RANSAC on the device (rfe_sim3_ransac / _dev) against the contract of DESIGN.md 6j restated in
tests/sim3_solver_ref.py.  Every comparison is exact (np.array_equal on T12, R, t, s, inliers, best_inliers, counts, hyps and stats), in
host and device form."""
import ctypes

import numpy as np
import pytest

import sim3_solver_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
OUT = R.OUT
OPTIONAL = ("R", "t", "s", "inliers", "best_inliers", "counts", "hyps")
SENT = {"inliers": 7, "best_inliers": 9, "counts": -5, "hyps": F32(-3.0)}


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def batch(cases, N=None, H=None, poison=True):
    """B cases stacked to [B, N] rows and [B, H] draws: case b keeps its n correspondences and its `its` draws in front; what lies behind is
    padding -- NaN positions and sigma2, draws far out of range -- when `poison`"""
    B = len(cases)
    N = max([len(c["xw1"]) for c in cases] + [0]) if N is None else N
    H = max([len(c["draws"]) for c in cases] + [1]) if H is None else H
    a = {"P": [dict(c["P"]) for c in cases], "xw1": np.zeros((B, N, 3), F32), "xw2": np.zeros((B, N, 3), F32), "s1": np.ones((B, N), F32),
         "s2": np.ones((B, N), F32), "draws": np.zeros((B, H, 3), np.int32)}
    if poison:
        a["xw1"][:], a["xw2"][:], a["s1"][:], a["s2"][:], a["draws"][:] = np.nan, np.nan, np.nan, -1.0, 1 << 30
    for b, c in enumerate(cases):
        n, its = len(c["xw1"]), c["P"]["its"]
        assert n == c["P"]["n"] and its <= len(c["draws"])
        for k in ("xw1", "xw2", "s1", "s2"):
            a[k][b, :n] = c[k]
        a["draws"][b, :its] = c["draws"][:its]
    return a


def shapes(a):
    B, N = a["s1"].shape
    H = a["draws"].shape[1]
    return B, N, H, {"T12": (B, 16), "R": (B, 9), "t": (B, 3), "s": (B,), "inliers": (B, N), "best_inliers": (B, N), "counts": (B, H),
                     "hyps": (B, H, 32), "stats": (B, 8)}


def fills(a):
    _, _, _, sh = shapes(a)
    return {k: np.full(sh[k], SENT[k], OUT[k]) for k in SENT}


def reference(a):
    B, N, H, sh = shapes(a)
    if B == 0:
        return {k: np.zeros(sh[k], OUT[k]) for k in OUT}
    f = fills(a)
    rs = [R.sim3_ransac(a["P"][b], a["xw1"][b], a["xw2"][b], a["s1"][b], a["s2"][b], a["draws"][b], N=N, H=H, fill={k: f[k][b] for k in f})
          for b in range(B)]
    return {k: np.stack([np.asarray(r[k], OUT[k]) for r in rs]) for k in OUT}


def same(got, ref, keys=tuple(OUT)):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.argwhere(~((got[k] == ref[k]) | (np.isnan(got[k].astype(np.float64)) &
                                                                     np.isnan(ref[k].astype(np.float64)))))[:8], got[k].ravel()[:8], ref[k].ravel()[:8])


def host(ctx, a, outputs=OPTIONAL):
    f = fills(a)
    return ctx.sim3_ransac(a["P"], a["xw1"], a["xw2"], a["s1"], a["s2"], a["draws"], fill={k: v for k, v in f.items() if k in outputs}, outputs=outputs)


def dev_enqueue(ctx, a, outputs=OPTIONAL):
    """rfe_sim3_ransac_dev on uploaded copies, not waited for; returns finish(), which synchronises, downloads the host form's dict and frees"""
    B, N, H, sh = shapes(a)
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(max(x.nbytes, 4)))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    f = fills(a)
    init = {k: f[k] if k in f else np.full(sh[k], 55, OUT[k]) for k in OUT}
    out = {k: up(init[k], OUT[k]) for k in ("T12", "stats") + tuple(outputs)}
    ctx.sim3_ransac_dev(a["P"], up(a["xw1"], F32), up(a["xw2"], F32), up(a["s1"], F32), up(a["s2"], F32), up(a["draws"], np.int32), B, N, H,
                        out["T12"], out["stats"], **{k: out[k] for k in outputs})

    def finish():
        try:
            ctx.synchronize()
            return {k: out[k].download(sh[k], OUT[k]) if np.prod(sh[k]) else np.zeros(sh[k], OUT[k]) for k in out}
        finally:
            for b in bufs:
                b.free()
    return finish


def dev(ctx, a, outputs=OPTIONAL):
    return dev_enqueue(ctx, a, outputs)()


def both(ctx, a, ref=None):
    ref = reference(a) if ref is None else ref
    h = host(ctx, a)
    same(h, ref)
    same(dev(ctx, a), ref)
    return h, ref


# ---------------------------------------------------------------- 1. sizes, one problem
@pytest.mark.parametrize("n", [0, 2, 3, 63, 64, 65, 257, 1100, 4096])
def test_sizes(ctx, n):
    c = R.scene(300 + n, n, its=5, outliers=0.2, fix_scale=n % 2)
    h, ref = both(ctx, batch([c], N=n + 3 if n < 4096 else n, H=8))
    if n >= 63:
        assert ref["counts"][0, :5].max() >= int(0.8 * n) - 1
    assert (h["inliers"][0, n:] == SENT["inliers"]).all() and (h["counts"][0, 5:] == SENT["counts"]).all() and (h["hyps"][0, 5:] == SENT["hyps"]).all()
    print(f"n={n}: stats {h['stats'][0].tolist()} counts {h['counts'][0, :5].tolist()}")


@pytest.mark.parametrize("its", [1, 3, 4, 5, 300, 1024])
def test_iteration_counts(ctx, its):
    # min_inliers above every count: all `its` hypotheses are the reference's too
    c = R.scene(400 + its, 65, its=its, min_inliers=60)
    h, ref = both(ctx, batch([c], H=its if its in (4, 1024) else its + 2))
    assert ref["stats"][0].tolist()[3:6] == [int(np.flatnonzero(ref["counts"][0, :its] == ref["counts"][0, :its].max())[-1]), its, 1]
    c = R.scene(400 + its, 65, its=its)                               # and with the scene's own min_inliers
    both(ctx, batch([c]))


# ---------------------------------------------------------------- 2. several problems
def test_batch_of_five(ctx):
    spec = [(600, 300, 0, None), (0, 4, 1, None), (257, 5, 1, 257), (1100, 37, 0, None), (41, 1, 0, 3)]
    cases = [R.scene(40 + b, n, its=its, fix_scale=fs, min_inliers=mn) for b, (n, its, fs, mn) in enumerate(spec)]
    a = batch(cases, N=1100, H=300)
    assert [p["n"] for p in a["P"]] == [600, 0, 257, 1100, 41] and np.isnan(a["xw1"][0, 600:]).all() and (a["draws"][3, 37:] == 1 << 30).all()
    h, ref = both(ctx, a)
    assert ref["stats"][:, 0].tolist() == [1, 0, 0, 1, 0] and ref["stats"][1, 7] == R.FLAG_FEW | R.FLAG_BELOW_THREE and len({t.tobytes() for t in ref["T12"]}) == 5
    for b, (n, its, _, _) in enumerate(spec):
        assert (h["best_inliers"][b, n:] == SENT["best_inliers"]).all() and (h["best_inliers"][b, :n] <= 1).all()
        assert (h["counts"][b, its:] == SENT["counts"]).all() and (h["hyps"][b, its:] == SENT["hyps"]).all()
    assert (h["counts"][1] == SENT["counts"]).all()                   # no hypothesis ran
    assert h["ret"] == ref["stats"][0, 0] == 1


def test_more_problems_than_one_front_launch(ctx):
    cases = [R.scene(500 + b, 20 + 3 * b, its=4 + b % 5, fix_scale=b % 2) for b in range(19)]
    both(ctx, batch(cases))


def test_optional_outputs_null(ctx):
    c = R.scene(64, 300, its=40)
    a = batch([c, R.scene(65, 200, its=40)])
    ref = reference(a)
    for outputs in ((), ("counts",), ("inliers", "s"), ("R", "t", "best_inliers", "hyps")):
        keys = ("T12", "stats") + outputs
        same(host(ctx, a, outputs=outputs), ref, keys)
        same(dev(ctx, a, outputs=outputs), ref, keys)


# ---------------------------------------------------------------- 3. the forced paths of the CPU tests
@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(ctx, name):
    c = R.forced(name)
    h, ref = both(ctx, batch([c]))
    st = ref["stats"][0]
    if name == "pure_translation_only":
        assert np.isnan(h["T12"][0, :12]).all() and st[6] == 1
    elif name == "n_lt_min":
        assert st[7] == R.FLAG_FEW and np.array_equal(h["T12"][0].reshape(4, 4), np.eye(4))
    elif name == "out_of_range":
        assert st[7] == R.FLAG_CLAMPED
    elif name == "max_three_times":
        assert st[3] == 4 and st[5] == 1
    elif name == "threshold":
        assert h["best_inliers"][0, :2].tolist() == [0, 1]


def test_below_three_correspondences(ctx):
    c = R.scene(3, 2, outliers=0.0, min_inliers=1, its=2)
    h, ref = both(ctx, batch([c]))
    assert ref["stats"][0].tolist() == [0, 0, 0, -1, 0, 1, 0, R.FLAG_BELOW_THREE]


# ---------------------------------------------------------------- 4. back to back on one ctx: the workspace is reused, grown, reused
def test_back_to_back_calls(ctx):
    a1 = batch([R.scene(71, 1100, its=300), R.scene(72, 900, its=300)])
    a2 = batch([R.scene(73, 65, its=5)])
    a3 = batch([R.scene(74 + b, 2000, its=64) for b in range(3)])
    same(dev(ctx, a1), reference(a1))                                 # sizes the workspace
    f1, f2 = dev_enqueue(ctx, a1, outputs=("inliers", "s")), dev_enqueue(ctx, a2)      # no wait in between; the second keeps its own counts and hyps
    r2, r1 = f2(), f1()
    same(r1, reference(a1), ("T12", "stats", "inliers", "s"))
    same(r2, reference(a2))
    same(dev(ctx, a3), reference(a3))                                 # grows it
    same(dev(ctx, a2), reference(a2))


# ---------------------------------------------------------------- 5. refusals
def test_refusals(ctx):
    from rover_slam_amd import capi
    c = R.scene(81, 20, its=6)
    a = batch([c], H=8)

    def refused(B=1, N=20, H=8, null=(), form="both", params=None, **arrays):
        x = dict(a, **arrays)
        P = capi.sim3_solver_params(x["P"] if params is None else params)
        o = {"T12": np.zeros(16, F32), "R": np.zeros(9, F32), "t": np.zeros(3, F32), "s": np.zeros(1, F32), "inliers": np.zeros(4096, np.uint8),
             "best_inliers": np.zeros(4096, np.uint8), "counts": np.zeros(1024, np.int32), "hyps": np.zeros((1024, 32), F32),
             "stats": np.zeros(8, np.int32)}
        args = {"params": ctypes.addressof(P), "xw1": x["xw1"].ctypes.data, "xw2": x["xw2"].ctypes.data, "s1": x["s1"].ctypes.data,
                "s2": x["s2"].ctypes.data, "draws": x["draws"].ctypes.data, "B": B, "N": N, "H": H}
        args.update({k: v.ctypes.data for k, v in o.items()})
        for k in null:
            args[k] = None
        # the _dev form checks its arguments before it touches a pointer, so host addresses do for the refusals
        fns = {"both": (capi.lib.rfe_sim3_ransac, capi.lib.rfe_sim3_ransac_dev), "host": (capi.lib.rfe_sim3_ransac,)}[form]
        for fn in fns:
            assert fn(ctx.h, *args.values()) == -1 and b"sim3_ransac" in capi.lib.rfe_last_error(ctx.h)     # RFE_ERR_INVALID
        return True

    assert refused(B=-1) and refused(B=65, params=a["P"] * 65) and refused(N=-1) and refused(N=4097) and refused(H=0) and refused(H=1025)
    for field, v in (("its", 0), ("its", 9), ("min_inliers", -1)):
        assert refused(params=[dict(a["P"][0], **{field: v})])
    for k in ("params", "draws", "T12", "stats", "xw1", "xw2", "s1", "s2"):
        assert refused(null=(k,))
    # the host form alone: a non-finite pose or intrinsic, a negative or non-finite sigma2 among the n rows
    for field in ("rcw1", "tcw1", "rcw2", "tcw2", "cam1", "cam2"):
        for bad in (np.nan, np.inf):
            v = np.array(a["P"][0][field], F32).copy()
            v.reshape(-1)[-1] = bad
            assert refused(params=[dict(a["P"][0], **{field: v})], form="host")
    for key in ("s1", "s2"):
        for bad in (-1.0, np.nan, np.inf):
            s = a[key].copy()
            s[0, 19] = bad
            assert refused(form="host", **{key: s})
    # and the context still works
    both(ctx, a)
