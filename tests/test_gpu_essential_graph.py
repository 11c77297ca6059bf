"""GPU: Optimizer::OptimizeEssentialGraph on the device (rfe_essential_graph / _dev) against the contract of DESIGN.md 6m restated in
tests/essential_graph_ref.py.  Every comparison is exact (np.array_equal on the Sim3s, their inverses, the float poses, the corrected
points, chi2, trace and stats), in host and device form; the inputs carry poisoned rows behind N, E and L and the device outputs sit
between guard words."""
import numpy as np
import pytest

import essential_graph_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUT = {"siw": F64, "tiw_f32": F32, "swi": F64, "xw_out": F32, "chi2": F64, "trace": F64, "stats": np.int32}
OPTIONAL = ("tiw_f32", "swi", "chi2", "trace")
REQUIRED = ("siw", "xw_out", "stats")
PAD = 37


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


def lib_params(P):
    from rover_slam_amd import capi
    return capi.essential_graph_params(P["iterations"], P["max_trials"], P["user_lambda_init"], P["fix_scale"])


def padded(c):
    """the case's arrays with PAD poisoned rows behind N, E and L: NaN poses, wild indices"""
    def pad(a, fill):
        a = np.asarray(a)
        return np.concatenate([a, np.full((PAD,) + a.shape[1:], fill, a.dtype)])
    return {"s_est": pad(c["s_est"], np.nan), "s_meas": pad(c["s_meas"], np.nan), "fixed": pad(c["fixed"], 1), "edge_i": pad(c["edge_i"], 1 << 30),
            "edge_j": pad(c["edge_j"], -5), "edge_from_est": pad(c["edge_from_est"], 1), "xw": pad(c["xw"], np.nan),
            "point_ref": pad(c["point_ref"], 1 << 30)}


def shape_of(c):
    return len(c["fixed"]), len(c["edge_i"]), len(c["point_ref"])


def same(got, ref, keys):
    for k in keys:
        assert got[k].dtype == ref[k].dtype == OUT[k] and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, np.argwhere(got[k] != ref[k])[:8], got[k].ravel()[:8], ref[k].ravel()[:8])


def host(ctx, c, P, outputs=OPTIONAL):
    a = padded(c)
    return ctx.essential_graph(lib_params(P), a["s_est"], a["s_meas"], a["fixed"], a["edge_i"], a["edge_j"], a["edge_from_est"], a["xw"],
                               a["point_ref"], outputs=outputs, shape=shape_of(c))


def dev(ctx, c, P, outputs=OPTIONAL):
    """rfe_essential_graph_dev on uploaded copies; returns the host form's dict.  Every output sits between two guard words"""
    a = padded(c)
    N, E, L = shape_of(c)
    its = max(P["iterations"], 0)
    bufs = []

    def up(x, dt):
        x = np.ascontiguousarray(x, dt)
        bufs.append(ctx.alloc(x.nbytes + 64))
        return bufs[-1].upload(x) if x.nbytes else bufs[-1]
    shape = {"siw": (N, 8), "tiw_f32": (N, 7), "swi": (N, 8), "xw_out": (L, 3), "chi2": (E,), "trace": (its, 4), "stats": (8,)}
    fill = {"siw": 3, "tiw_f32": 3, "swi": 3, "xw_out": 3, "chi2": -3, "trace": 5, "stats": 77}
    guard = {k: np.concatenate([np.full(8, 0x5A, np.uint8), np.full(shape[k], fill[k], OUT[k]).view(np.uint8).ravel(), np.full(8, 0x5A, np.uint8)])
             for k in REQUIRED + tuple(outputs)}
    out = {k: up(g, np.uint8) for k, g in guard.items()}
    try:
        ins = [up(a["s_est"], F64), up(a["s_meas"], F64), up(a["fixed"], np.uint8), up(a["edge_i"], np.int32), up(a["edge_j"], np.int32),
               up(a["edge_from_est"], np.uint8), up(a["xw"], F32), up(a["point_ref"], np.int32)]
        ret = ctx.essential_graph_dev(lib_params(P), N, E, L, *ins, out["siw"].ptr + 8, out["xw_out"].ptr + 8, out["stats"].ptr + 8,
                                      **{k: out[k].ptr + 8 for k in outputs})
        res = {"ret": ret}
        for k in out:
            raw = out[k].download(guard[k].shape, np.uint8)
            assert (raw[:8] == 0x5A).all() and (raw[-8:] == 0x5A).all(), k
            res[k] = raw[8:-8].view(OUT[k]).reshape(shape[k]).copy()
        return res
    finally:
        for b in bufs:
            b.free()


def both(ctx, c, P, ref=None, outputs=OPTIONAL):
    ref = R.essential_graph(c, P) if ref is None else ref
    keys = REQUIRED + tuple(outputs)
    h = host(ctx, c, P, outputs)
    same(h, ref, keys)
    assert h["ret"] == ref["ret"]
    d = dev(ctx, c, P, outputs)
    same(d, ref, keys)
    assert d["ret"] == ref["ret"]
    return h, ref


SHORT = dict(iterations=3)


# ---------------------------------------------------------------- 1. sizes at the edges of the kernel
@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("N", [1, 2, 3, R.TILE_V, R.TILE_V + 1, R.TILE_V + 2, 3 * R.TILE_V + 3])
def test_vertex_counts(ctx, N, fix_scale):
    """one fixed vertex, so N - 1 free ones: 0, 1, 2, one tile less a vertex, one tile exactly, one tile and a vertex, three tile
    columns and a remainder"""
    c = R.graph(20 + N, N, loops=min(2, N // 2), corrected=min(2, N // 2), L=5, drift=0.02)
    h, ref = both(ctx, c, R.params(fix_scale=fix_scale, **SHORT))
    assert ref["stats"][5] == N - 1


@pytest.mark.parametrize("E", [255, 257, 1023, 1025])
def test_edge_counts(ctx, E):
    c = R.graph(30, 24, band=6, loops=3, corrected=3, edges_total=E, drift=0.01)
    assert len(c["edge_i"]) == E
    both(ctx, c, R.params(iterations=2))


@pytest.mark.parametrize("L", [0, 1, 257, 70000])
def test_point_counts(ctx, L):
    c = R.graph(31, 9, loops=2, corrected=2, L=L, drift=0.02)
    h, ref = both(ctx, c, R.params(**SHORT))
    if L > 3:
        assert np.array_equal(h["xw_out"][1], c["xw"][1]) and not np.array_equal(h["xw_out"][0], c["xw"][0])


# ---------------------------------------------------------------- 2. structures
@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("kind", ["chain", "star", "arrowhead"])
def test_structures(ctx, kind, fix_scale):
    """40 keyframes, ten tile columns.  The arrowhead fills only the band and the last rows: fewer tiles than the dense triangle are
    processed, and the result still equals the dense restatement"""
    c = R.graph(40, 40, kind=kind, corrected=3 if kind != "star" else 0, drift=0.01, dscale=0.0 if fix_scale else 0.005, L=12)
    h, ref = both(ctx, c, R.params(fix_scale=fix_scale, **SHORT))
    if kind == "arrowhead":
        assert 0 < h["stats"][6] < h["stats"][7]
    if kind == "star":
        assert h["stats"][6] == 10                    # the hub is fixed: the free vertices do not touch each other


def test_shuffled(ctx):
    """keyframe indices permuted, the fixed one in the middle: the elimination order is the index order, whatever the graph"""
    c = R.graph(41, 23, band=3, loops=3, corrected=3, shuffle=True, fixed=11, L=9, drift=0.01)
    assert c["fixed"][0] == 0 and c["fixed"].sum() == 1
    both(ctx, c, R.params(**SHORT))


# ---------------------------------------------------------------- 3. forced paths
@pytest.mark.parametrize("name", R.FORCED)
def test_forced(ctx, name):
    c, P = R.forced(name)
    h, ref = both(ctx, c, P)
    R.check_forced(name, ref)


def test_null_optional_outputs(ctx):
    c, P = R.forced("duplicates")
    ref = R.essential_graph(c, P)
    both(ctx, c, P, ref, outputs=())
    both(ctx, c, P, ref, outputs=("chi2",))


# ---------------------------------------------------------------- 4. the grow-only workspaces
def test_back_to_back(ctx):
    """calls on one ctx at growing and shrinking N: what one call left in the workspaces must not reach the next"""
    cases = [R.graph(50 + n, n, band=2, loops=2, corrected=2, L=7, drift=0.01) for n in (6, 30, 11)]
    P = R.params(**SHORT)
    refs = [R.essential_graph(c, P) for c in cases]
    for k in (0, 1, 2, 1, 0):
        both(ctx, cases[k], P, refs[k])


# ---------------------------------------------------------------- 5. refusals
def bad_cases():
    base = R.graph(60, 8, band=2, loops=2, corrected=2, L=6)
    out = {}
    c = dict(base); e = base["edge_i"].copy(); e[3] = 8; c["edge_i"] = e
    out["i_range"] = c
    c = dict(base); e = base["edge_j"].copy(); e[3] = -1; c["edge_j"] = e
    out["j_negative"] = c
    c = dict(base); e = base["edge_j"].copy(); e[4] = base["edge_i"][4]; c["edge_j"] = e
    out["self_edge"] = c
    c = dict(base); ei, ej = base["edge_i"].copy(), base["edge_j"].copy(); ei[[2, 9]] = ei[[9, 2]]; ej[[2, 9]] = ej[[9, 2]]; c["edge_i"], c["edge_j"] = ei, ej
    out["unsorted"] = c
    c = dict(base); r = base["point_ref"].copy(); r[2] = 8; c["point_ref"] = r
    out["ref_range"] = c
    c = dict(base); r = base["point_ref"].copy(); r[2] = -2; c["point_ref"] = r
    out["ref_negative"] = c
    return out


@pytest.mark.parametrize("name", ["i_range", "j_negative", "self_edge", "unsorted", "ref_range", "ref_negative"])
def test_refused_tables(ctx, name):
    """the host form checks on the host, the device form in its first kernels; nothing is written (dev() checks the fill survives)"""
    from rover_slam_amd import capi
    c = bad_cases()[name]
    P = R.params(**SHORT)
    with pytest.raises(R.Invalid):
        R.essential_graph(c, P)
    with pytest.raises(capi.RfeError):
        host(ctx, c, P)
    with pytest.raises(capi.RfeError):
        dev(ctx, c, P)
    both(ctx, R.graph(60, 8, band=2, loops=2, corrected=2, L=6), P)      # the ctx is usable afterwards


def test_refused_arguments(ctx):
    from rover_slam_amd import capi
    c = R.graph(61, 5, L=3)
    for P in (R.params(iterations=-1), R.params(iterations=65), R.params(max_trials=-1), R.params(user_lambda_init=np.inf)):
        with pytest.raises(capi.RfeError):
            host(ctx, c, P)
        with pytest.raises(capi.RfeError):
            dev(ctx, c, P)
    lp = lib_params(R.params())
    args = (c["s_est"], c["s_meas"], c["fixed"], c["edge_i"], c["edge_j"], c["edge_from_est"], c["xw"], c["point_ref"])
    for shape in ((0, 0, 0), (R.MAX_KF + 1, 0, 0), (5, R.MAX_EDGES + 1, 0), (5, -1, 0), (5, 0, R.MAX_POINTS + 1), (5, 0, -1)):
        with pytest.raises(capi.RfeError):
            ctx.essential_graph(lp, *args, shape=shape)


# ---------------------------------------------------------------- 6. the chain from OptimizeSim3
def test_chain_from_optimize_sim3(ctx):
    """rfe_optimize_sim3 and this entry back to back on one ctx: the refined S12 corrects the current keyframe (Scw' = S21 Slw as
    CorrectLoop forms it, on the host), which becomes the loop edge's end; both results equal their restatements"""
    import optimize_sim3_ref as OS
    sc = OS.scene(5, 120)
    ref12 = OS.solve(sc)
    got = ctx.optimize_sim3([sc["P"]], sc["s12_0"][None], sc["xw1"][None], sc["xw2"][None], sc["valid"][None], sc["kpts1"][None], sc["idx2"][None],
                            sc["kpts2"][None], octave1=sc["octave1"][None], octave2=sc["octave2"][None])
    assert np.array_equal(got["s12"][0], ref12["s12"])
    c = R.graph(62, 14, loops=0, corrected=0, L=8, drift=0.01)
    s21 = np.array(OS.sim3_inverse([F64(v) for v in got["s12"][0]]), F64)
    c["s_est"][13] = np.array(R.sim3_mul([F64(v) for v in s21], [F64(v) for v in c["s_est"][0]]), F64)
    e = sorted([(int(i), int(j), int(f)) for i, j, f in zip(c["edge_i"], c["edge_j"], c["edge_from_est"])] + [(13, 0, 1)])
    e = np.array(e)
    c["edge_i"], c["edge_j"], c["edge_from_est"] = e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), e[:, 2].astype(np.uint8)
    both(ctx, c, R.params(**SHORT))
