"""The sparse descriptor head (calls of more than four frames: convDa, convDb and the L2 norm only on the cells that keypoints sample, as GEMM rows)
against the dense head (up to four frames: the whole map), against the oracle, and stage by stage through rfe_k_sparse_desc.

Everything is compared bit for bit: the canonical arithmetic (bias, then the kappa-ascending fmaf chain, padding multiplied) does not depend on the
matrix row a cell sits in.  The only tolerance of this file is on the hook's sampled descriptors for hand-placed keypoints, which have no bit-exact
numpy counterpart (fmaf chains): a float64 bilinear sample of the dense map, 2e-6 absolute on unit-norm vectors (about ten fp32 roundings of values
<= 1 at 2^-24 each, then one division by a norm that carries the same error)."""
import numpy as np
import pytest

from rover_slam_amd import weights as Wt, synth

pytestmark = pytest.mark.gpu

SP_SEED = 7


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi
    c = capi.Context(0)
    c.set_weights(capi.KIND_SUPERPOINT, Wt.make_superpoint(seed=SP_SEED))
    yield c
    c.close()


def _extract_dev(ctx, frames, kmax, thr=0.0005):
    """rfe_extract_u8_bin_dev on frames [B,H,W] in ONE call (B > 4: sparse head, B <= 4: dense head); fresh output buffers every time"""
    from rover_slam_amd import capi
    frames = np.ascontiguousarray(frames, np.uint8)
    B, H, W = frames.shape
    dimg = ctx.alloc(frames.nbytes).upload(frames)
    spec = [("n", np.int32, (B,)), ("kxy", np.int32, (B, kmax, 2)), ("score", np.float32, (B, kmax)), ("desc", np.float32, (B, kmax, 256)),
            ("desc_bin", np.uint8, (B, kmax, 256))]
    bufs = {k: ctx.alloc(int(np.prod(s)) * np.dtype(t).itemsize) for k, t, s in spec}
    for k, t, s in spec:   # a word no kernel writes: an element the call skipped would show
        bufs[k].upload(np.full(bufs[k].nbytes, 0x5A, np.uint8))
    ctx._chk(capi.lib.rfe_extract_u8_bin_dev(ctx.h, dimg.ptr, H, W, W, B, kmax, thr, bufs["n"].ptr, bufs["kxy"].ptr, bufs["score"].ptr,
                                             bufs["desc"].ptr, bufs["desc_bin"].ptr))
    ctx.synchronize()
    out = {k: bufs[k].download(s, t) for k, t, s in spec}
    for d in [dimg] + list(bufs.values()):
        d.free()
    return out


def _one_by_one(ctx, frames, kmax, thr=0.0005):
    outs = [_extract_dev(ctx, frames[i:i + 1], kmax, thr) for i in range(len(frames))]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_paths_agree(sparse, dense, frames, kmax, thr, oracle):
    for k in ("n", "kxy", "score", "desc", "desc_bin"):
        assert _same_bits(sparse[k], dense[k]), k            # desc compared as bytes: -0.0 and NaN payloads count
    w = Wt.make_superpoint(seed=SP_SEED)
    for i in range(len(frames)):
        r = oracle.superpoint(w, frames[i], kmax=kmax, thr=thr)
        n = r["n"]
        assert sparse["n"][i] == n
        assert np.array_equal(sparse["kxy"][i, :n], r["kxy"][:n]) and _same_bits(sparse["score"][i, :n], r["score"][:n])
        assert _same_bits(sparse["desc"][i, :n], r["desc"][:n])
        assert np.array_equal(sparse["desc_bin"][i, :n], (r["desc"][:n] > 0).astype(np.uint8))
        assert not sparse["desc"][i, n:].any() and not sparse["desc_bin"][i, n:].any()


def _footprint_cells(kxy, n, H, W, Hc, Wc):
    """desc_footprint (sp_post.hip) in numpy float32, operation by operation: the [Hc,Wc] mask of in-range corner cells of keypoints kxy[:n]"""
    f = np.float32
    x, y = kxy[:n, 0].astype(f), kxy[:n, 1].astype(f)
    gx = ((x - f(3.5)) / (f(W) - f(4.5))) * f(2.0) - f(1.0)
    gy = ((y - f(3.5)) / (f(H) - f(4.5))) * f(2.0) - f(1.0)
    ix = ((gx + f(1.0)) * f(0.5)) * f(Wc - 1)
    iy = ((gy + f(1.0)) * f(0.5)) * f(Hc - 1)
    assert ix.dtype == np.float32 and iy.dtype == np.float32
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    m = np.zeros((Hc, Wc), bool)
    outside = 0
    for dx in (0, 1):
        for dy in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < Wc) & (yy >= 0) & (yy < Hc)
            m[yy[ok], xx[ok]] = True
            outside += int((~ok).sum())
    return m, outside, (ix, iy, x0, y0)


def _expected_cell_row(mask):
    flat = mask.reshape(-1)
    return np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32), int(flat.sum())


def _sparse_hook(ctx, frames, kmax, n, kxy, poison=0):
    from rover_slam_amd import capi
    frames = np.ascontiguousarray(frames, np.uint8)
    B, H, W = frames.shape
    Hc, Wc = H // 8, W // 8
    cap = min(4 * kmax, Hc * Wc)
    dimg = ctx.alloc(frames.nbytes).upload(frames)
    dn = ctx.alloc(B * 4).upload(np.ascontiguousarray(n, np.int32))
    dk = ctx.alloc(B * kmax * 8).upload(np.ascontiguousarray(kxy, np.int32))
    dcr, dcnt, drows, ddesc = ctx.alloc(B * Hc * Wc * 4), ctx.alloc(B * 4), ctx.alloc(B * cap * 1024), ctx.alloc(B * kmax * 1024)
    ctx._chk(capi.lib.rfe_k_sparse_desc(ctx.h, dimg.ptr, H, W, W, B, kmax, dn.ptr, dk.ptr, poison, dcr.ptr, dcnt.ptr, drows.ptr, ddesc.ptr))
    out = dict(cell_row=dcr.download((B, Hc * Wc), np.int32), count=dcnt.download((B,), np.int32), rows=drows.download((B * cap, 256), np.float32),
               desc=ddesc.download((B, kmax, 256), np.float32))
    out["base"] = np.concatenate([[0], np.cumsum(out["count"])])      # the frames' rows lie back to back: frame b's are rows base[b] .. base[b + 1]
    assert (out["count"] >= 0).all() and (out["count"] <= cap).all()
    for d in (dimg, dn, dk, dcr, dcnt, drows, ddesc):
        d.free()
    return out


def _dense_descmap(ctx, frames):
    from rover_slam_amd import capi
    frames = np.ascontiguousarray(frames, np.uint8)
    B, H, W = frames.shape
    dimg = ctx.alloc(frames.nbytes).upload(frames)
    dd = ctx.alloc(B * (H // 8) * (W // 8) * 1024)
    ctx._chk(capi.lib.rfe_k_scoremap(ctx.h, dimg.ptr, H, W, W, B, None, None, dd.ptr))
    dmap = dd.download((B, (H // 8) * (W // 8), 256), np.float32)
    dimg.free(); dd.free()
    return dmap


# ------------------------------------------------------------------ cross-path: B = 5 in one call (sparse) against the same frames one by one (dense)
@pytest.mark.parametrize("H,W,constant", [(120, 160, True), (101, 151, False)])
def test_sparse_equals_dense_and_oracle(ctx, oracle, H, W, constant):
    """120 x 160 with one constant frame (a constant region keeps every pixel of it through simple_nms's equality mask, so that frame saturates Kmax
    with tied scores), and 101 x 151: floor pooling, 12 x 18 cells, the score frame 96 x 144 smaller than the image"""
    kmax = 100
    frames, _ = synth.make_frames(5, H, W, seed=H + W)
    if constant:
        frames[2] = 128
    sparse, dense = _extract_dev(ctx, frames, kmax), _one_by_one(ctx, frames, kmax)
    _assert_paths_agree(sparse, dense, frames, kmax, 0.0005, oracle)


@pytest.mark.parametrize("kmax,thr,every_cell", [(4096, -0.5, True), (12, 0.0005, False)])
def test_every_cell_and_keypoint_bound_capacity(ctx, oracle, kmax, thr, every_cell):
    """64 x 64 frames = 8 x 8 cells.  (a) thr = -0.5 with Kmax = 4096 selects every pixel inside the border (3136 keypoints, suppressed ones with score 0
    included): all 64 cells are needed, count == capacity == Hc Wc, and the rows ARE the dense map, row for row.  (b) Kmax = 12: capacity 4 Kmax = 48 < 64
    cells, the keypoint bound."""
    H = W = 64
    frames, _ = synth.make_frames(5, H, W, seed=4)
    sparse, dense = _extract_dev(ctx, frames, kmax, thr), _one_by_one(ctx, frames, kmax, thr)
    _assert_paths_agree(sparse, dense, frames, kmax, thr, oracle)
    h = _sparse_hook(ctx, frames, kmax, sparse["n"], sparse["kxy"])
    dmap = _dense_descmap(ctx, frames)
    for b in range(5):
        mask, _, _ = _footprint_cells(sparse["kxy"][b], int(sparse["n"][b]), H, W, 8, 8)
        exp_row, cnt = _expected_cell_row(mask)
        assert h["count"][b] == cnt and np.array_equal(h["cell_row"][b], exp_row)
        if every_cell:
            assert cnt == 64 and _same_bits(h["rows"][64 * b:64 * b + 64], dmap[b])
        else:
            assert 4 * kmax < 64 and 0 < cnt <= 4 * kmax
            assert _same_bits(h["rows"][h["base"][b]:h["base"][b + 1]], dmap[b][mask.reshape(-1)])


# ------------------------------------------------------------------ hook level: hand-placed keypoints, edges, poison, repeatability
def _edge_case_keypoints(frames, kmax, ctx):
    """n [5], kxy [5,kmax,2] for five 120 x 160 frames: frame 0 the extraction's own keypoints; frame 1 the four image corners, points along all four image
    edges (x1 / y1 = Wc / Hc or x0 / y0 = -1: a corner outside the map) and points whose cell lies on each map edge (3 x 3 taps outside the map);
    frame 2 none at all (zero rows: the GEMMs see m_valid = 0); frame 3 kmax random pixels with repeats; frame 4 one keypoint"""
    B, H, W = frames.shape
    ex = _extract_dev(ctx, frames, kmax)
    n, kxy = np.zeros((B,), np.int32), np.zeros((B, kmax, 2), np.int32)
    n[0], kxy[0] = ex["n"][0], ex["kxy"][0]
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    pts += [(x, 0) for x in range(5, W, 17)] + [(x, H - 1) for x in range(3, W, 19)] + [(0, y) for y in range(2, H, 13)] + [(W - 1, y) for y in range(7, H, 11)]
    pts += [(4, 60), (W - 5, 61), (80, 4), (81, H - 5), (W - 2, H - 2), (1, 1)]
    assert len(pts) <= kmax
    n[1] = len(pts); kxy[1, :len(pts)] = np.array(pts, np.int32)
    rng = np.random.default_rng(11)
    n[3] = kmax
    kxy[3, :, 0], kxy[3, :, 1] = rng.integers(0, W, kmax), rng.integers(0, H, kmax)
    kxy[3, 1::7] = kxy[3, 0::7][:len(kxy[3, 1::7])]      # repeated keypoints: several writers of one mark
    n[4] = 1; kxy[4, 0] = (77, 58)
    return n, kxy


@pytest.fixture(scope="module")
def hook_case(ctx):
    H, W, kmax = 120, 160, 100
    frames, _ = synth.make_frames(5, H, W, seed=21)
    n, kxy = _edge_case_keypoints(frames, kmax, ctx)
    return dict(H=H, W=W, kmax=kmax, frames=frames, n=n, kxy=kxy, plain=_sparse_hook(ctx, frames, kmax, n, kxy), dmap=_dense_descmap(ctx, frames))


def test_hook_cell_list_and_rows_against_dense_map(hook_case):
    c = hook_case
    H, W, Hc, Wc = c["H"], c["W"], c["H"] // 8, c["W"] // 8
    h = c["plain"]
    outside_seen, edge_cells = 0, np.zeros((Hc, Wc), bool)
    for b in range(5):
        mask, outside, _ = _footprint_cells(c["kxy"][b], int(c["n"][b]), H, W, Hc, Wc)
        exp_row, cnt = _expected_cell_row(mask)
        assert h["count"][b] == cnt, b
        assert np.array_equal(h["cell_row"][b], exp_row), b
        assert _same_bits(h["rows"][h["base"][b]:h["base"][b + 1]], c["dmap"][b][mask.reshape(-1)]), b
        outside_seen += outside if b == 1 else 0
        edge_cells |= mask
    assert h["count"][2] == 0 and (h["cell_row"][2] == -1).all()
    assert outside_seen > 0                                                                   # corners outside the map were asked for
    assert edge_cells[0].any() and edge_cells[-1].any() and edge_cells[:, 0].any() and edge_cells[:, -1].any()   # cells on all four map edges
    assert edge_cells[0, 0] and edge_cells[0, -1] and edge_cells[-1, 0] and edge_cells[-1, -1]


def test_hook_sampling_through_cell_row(hook_case):
    """descriptors sampled through cell_row against a float64 bilinear sample of the DENSE map (zero outside), L2-normalised: 2e-6 (module docstring)"""
    c = hook_case
    H, W, Hc, Wc = c["H"], c["W"], c["H"] // 8, c["W"] // 8
    for b in range(5):
        n = int(c["n"][b])
        assert not c["plain"]["desc"][b, n:].any()
        if n == 0:
            continue
        _, _, (ix, iy, x0, y0) = _footprint_cells(c["kxy"][b], n, H, W, Hc, Wc)
        ix, iy = ix.astype(np.float64), iy.astype(np.float64)
        dm = np.zeros((Hc + 2, Wc + 2, 256))
        dm[1:-1, 1:-1] = c["dmap"][b].reshape(Hc, Wc, 256)
        wx1, wy1 = ix - x0, iy - y0
        v = (dm[y0 + 1, x0 + 1] * ((1 - wx1) * (1 - wy1))[:, None] + dm[y0 + 1, x0 + 2] * (wx1 * (1 - wy1))[:, None]
             + dm[y0 + 2, x0 + 1] * ((1 - wx1) * wy1)[:, None] + dm[y0 + 2, x0 + 2] * (wx1 * wy1)[:, None])
        v /= np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12)
        err = np.abs(c["plain"]["desc"][b, :n] - v).max()
        print(f"frame {b}: max |desc - float64 sample| = {err:.3e}")
        assert err <= 2e-6, (b, err)


def test_hook_poisoned_workspace_and_repeatability(ctx, hook_case):
    """NaN in the patch buffer, both activation buffers and the row tables beyond (and under) the live rows changes nothing; neither does a second run"""
    c = hook_case
    for poison in (1, 0):
        h = _sparse_hook(ctx, c["frames"], c["kmax"], c["n"], c["kxy"], poison=poison)
        assert np.array_equal(h["count"], c["plain"]["count"]) and np.array_equal(h["cell_row"], c["plain"]["cell_row"])
        assert _same_bits(h["desc"], c["plain"]["desc"])
        k = int(h["base"][-1])
        assert k > 0 and _same_bits(h["rows"][:k], c["plain"]["rows"][:k]) and not np.isnan(h["rows"][:k]).any()


def test_extract_repeatable(ctx):
    frames, _ = synth.make_frames(6, 120, 160, seed=33)
    a, b = _extract_dev(ctx, frames, 128), _extract_dev(ctx, frames, 128)
    for k in a:
        assert _same_bits(a[k], b[k]), k
    assert a["n"].min() > 0
