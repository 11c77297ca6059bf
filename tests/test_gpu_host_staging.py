"""Every host-pointer entry stages its arrays through ONE device block (ws_io) and, for the per-frame entries, its pinned
mirror (h_pin); both only ever grow, and each entry lays its arrays out in them anew on every call.  The per-entry tests
run one entry on one context and cannot see what that sharing can break: an entry reading what another one left behind, a
layout that goes wrong once the block has been regrown, arrays whose padding differs from their neighbours'.

So: on ONE context every entry is called at a small shape, then at a larger one that makes ws_io grow (the large shapes
ascend in size from entry to entry, and the growth is asserted), then at the small shape again; every single call is
repeated on a fresh context, and every output of the shared context must equal the fresh one's byte for byte.

Bit stability: every output compared here is the same from run to run (fresh context against fresh context, checked on
an MI355X for each call of this file), the LightGlue match scores included -- there is no float atomic on any of these
paths --, so nothing is compared at a tolerance.

Small shapes: two 64 x 96 images at stride 112, Kmax = 48, N = 37 -- array sizes that are no multiple of the 256-byte
granule, so the padding between neighbours differs from array to array."""
import numpy as np
import pytest

from rover_slam_amd import weights as Wt, synth

H0, W0, PAD, K0, N0 = 64, 96, 16, 48, 37
MB, MBF = 0.11, 0.11 * 435.0
LEVELS, SF = 3, 1.2


def _unit(rng, n):
    d = rng.standard_normal((n, 256)).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _stereo_case(rng, H, W, n, nr, disp=6):
    """a shifted view pair with keypoints that do match: right(x) = left(x + disp), right keypoint i = left keypoint i shifted"""
    scene = synth.make_scene(rng, H, W + disp, margin=0)
    left = np.clip(scene[:, :W] + rng.integers(0, 8, (H, W)), 0, 255).astype(np.uint8)
    right = np.clip(scene[:, disp:disp + W] + rng.integers(0, 8, (H, W)), 0, 255).astype(np.uint8)
    kl = np.stack([rng.integers(24, W - 16, n), rng.integers(14, H - 14, n)], axis=1).astype(np.float32)
    dl = _unit(rng, n)
    pick = rng.permutation(n)[:nr] if nr <= n else rng.integers(0, n, nr)
    kr = kl[pick] - np.array([disp, 0], np.float32)
    dr = dl[pick]
    return np.ascontiguousarray(left), np.ascontiguousarray(right), kl, kr, dl, np.ascontiguousarray(dr)


def _csr(rng, rows, nf, per):
    counts = rng.integers(0, per + 1, rows)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cand = rng.integers(0, max(nf, 1), int(off[-1])).astype(np.int32)
    return off, cand


def _calls(capi):
    """name -> (weights it needs, small call, large call or None); a call takes a context and returns a tuple of arrays"""
    rng = np.random.default_rng(20250117)
    small_img = synth.make_frames(2, H0, W0, seed=3)[0]
    large_img = synth.make_frames(3, 96, 128, seed=4)[0]
    calls = {}

    def raw(fn_name, outs, *args):      # entries without a Context method; the closure keeps the arrays alive
        def run(ctx):
            ctx._chk(getattr(capi.lib, fn_name)(ctx.h, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]))
            return tuple(o.copy() for o in outs)
        return run

    # ---- descriptor helpers, ascending ws_io need of the large shapes: 2, 3, 4, 5, 6 MiB
    def binarize(rows):
        d, bits = _unit(rng, rows), np.zeros((rows, 256), np.uint8)
        return raw("rfe_binarize_descriptors", [bits], d, rows, bits)
    calls["binarize"] = ("", binarize(N0), binarize(900))

    def distinctive(npts, per):
        off, _ = _csr(rng, npts, 1, per)
        d = _unit(rng, int(off[-1]))
        return lambda ctx: ctx.distinctive_descriptors(d, off)
    calls["distinctive"] = ("", distinctive(N0, 5), distinctive(460, 10))

    def l2(m, n):
        a, b, out = _unit(rng, m), _unit(rng, n), np.zeros((m, n), np.float32)
        return raw("rfe_l2_distance_matrix", [out], a, m, b, n, out)
    calls["l2"] = ("", l2(N0, 29), l2(700, 800))

    def candidates(nq, nf, skip):
        q, f = _unit(rng, nq), _unit(rng, nf)
        off, cand = _csr(rng, nq, nf, 6 if nf else 0)
        sk = (rng.random(nf) < 0.2).astype(np.uint8) if skip else None
        return lambda ctx: ctx.search_candidates(q, f, off, cand, sk)
    calls["candidates"] = ("", candidates(N0, 53, True), candidates(2000, 2400, True))
    calls["candidates_nf0"] = ("", candidates(N0, 0, False), None)
    calls["candidates_noskip"] = ("", candidates(N0, 53, False), None)

    def projection(nq, nf, optional):
        W, H = 640.0, 480.0
        kpts = np.stack([rng.uniform(0, W, nf), rng.uniform(0, H, nf)], axis=1).astype(np.float32)
        f = _unit(rng, nf)
        src = rng.integers(0, max(nf, 1), nq)
        q = _unit(rng, nq) if nf == 0 else (f[src] + 0.02 * rng.standard_normal((nq, 256))).astype(np.float32)
        proj = (rng.uniform(0, [W, H], (nq, 2)) if nf == 0 else kpts[src] + rng.uniform(-3, 3, (nq, 2))).astype(np.float32)
        radius = rng.uniform(4, 12, nq).astype(np.float32)
        kw = {}
        if optional:
            kw = dict(pred_level=rng.integers(0, 3, nq), observed=(rng.random(nq) < 0.1).astype(np.uint8),
                      octave=rng.integers(0, 3, nf), skip=(rng.random(nf) < 0.1).astype(np.uint8))

        def run(ctx):
            r = ctx.search_by_projection(q, proj, radius, f, (0.0, 0.0, W, H), kpts=kpts, **kw)
            return r["assign"], r["best_idx"], r["best_dist"], r["second_dist"], r["stats"], np.array([r["nmatches"]])
        return run
    calls["projection"] = ("", projection(N0, 61, True), projection(3000, 2700, True))
    calls["projection_nf0"] = ("", projection(N0, 0, False), None)
    calls["projection_noskip_nooctave"] = ("", projection(N0, 61, False), None)

    # ---- stereo matchers: 7, 8 MiB
    def stereo(H, W, n, nr):
        il, ir, kl, kr, dl, dr = _stereo_case(rng, H, W, n, nr)
        return lambda ctx: ctx.stereo_match(il, ir, kl, kr, dl, dr, MB, MBF)
    calls["stereo"] = ("", stereo(H0, W0, N0, 31), stereo(96, 128, 3300, 3300))
    calls["stereo_nr0"] = ("", stereo(H0, W0, N0, 0), None)

    def stereo_pyr(H, W, n, nr):
        il, ir, kl, kr, dl, dr = _stereo_case(rng, H, W, n, nr)
        lh, lw, _ = capi.pyramid_geometry(H, W, LEVELS, SF)
        # any level images serve (the kernels only read them): nearest-neighbour shrunken views
        lv = [[np.ascontiguousarray(im[(np.arange(h) * H // h)][:, (np.arange(w) * W // w)]) for h, w in zip(lh, lw)] for im in (il, ir)]
        ol = rng.integers(0, LEVELS, n); orr = rng.integers(0, LEVELS, nr)
        return lambda ctx: ctx.stereo_match_pyramid(lv[0], lv[1], H, W, LEVELS, SF, kl, ol, kr, orr, dl, dr, MB, MBF)
    calls["stereo_pyramid"] = ("", stereo_pyr(H0, W0, N0, 31), stereo_pyr(96, 128, 3900, 3900))

    # ---- extractors (pinned transport): 9, 11, 13, 17+ MiB
    calls["extract_u8"] = ("s", lambda ctx: ctx.extract(small_img, kmax=K0, pad_cols=PAD), lambda ctx: ctx.extract(large_img[:2], kmax=4096))
    calls["extract_u8_bin"] = ("s", lambda ctx: ctx.extract(small_img, kmax=K0, pad_cols=PAD, binarized=True),
                               lambda ctx: ctx.extract(large_img[:2], kmax=4096, binarized=True))
    f32 = lambda im: im.astype(np.float32) / 255.0   # noqa: E731
    calls["extract_f32"] = ("s", lambda ctx: ctx.extract_f32(f32(small_img), kmax=K0), lambda ctx: ctx.extract_f32(f32(large_img), kmax=4096))

    def pyramid(img, kmax, pad):
        def run(ctx):
            r = ctx.extract_pyramid(img, nlevels=2, scale_factor=SF, kmax=kmax, with_levels=True, pad_cols=pad)
            return (r["n"], r["level_n"], r["kpts"], r["octave"], r["score"], r["desc"]) + tuple(r["levels"])
        return run
    calls["extract_pyramid"] = ("s", pyramid(small_img, K0, PAD), pyramid(large_img[:2], 4096, 0))

    # ---- matcher (pinned transport, two DMAs in): 21 MiB
    def match(P, M, N):
        k0, k1 = rng.uniform(-1, 1, (P, M, 2)).astype(np.float32), rng.uniform(-1, 1, (P, N, 2)).astype(np.float32)
        d0, d1 = _unit(rng, P * M).reshape(P, M, 256), _unit(rng, P * N).reshape(P, N, 256)
        m, n = rng.integers(M // 2, M + 1, P), rng.integers(N // 2, N + 1, P)

        def run(ctx):       # pairs / ms are defined up to S[p] matches per pair: what lies behind them is whatever the staging block held
            S, pairs, ms = ctx.match(k0, k1, d0, d1, m, n)
            for p in range(P):
                pairs[p, S[p]:] = 0; ms[p, S[p]:] = 0
            return S, pairs, ms
        return run
    calls["match"] = ("l", match(2, N0, K0), match(10, 1024, 1024))

    def fused(M, N):
        kp0, kp1 = rng.uniform(0, [W0, H0], (M, 2)).astype(np.float32), rng.uniform(0, [W0, H0], (N, 2)).astype(np.float32)
        d0, d1 = _unit(rng, M), _unit(rng, N)

        def run(ctx):
            size, vn = ctx.match_fused(kp0, kp1, d0, d1, H0, W0)
            return np.array([size]), vn
        return run
    calls["match_fused"] = ("l", fused(N0, K0), None)   # rfe_match underneath: no shape of one pair outgrows the call above
    return calls


@pytest.mark.gpu
def test_host_entries_share_staging():
    from rover_slam_amd import capi
    blobs = {"s": (capi.KIND_SUPERPOINT, Wt.make_superpoint(seed=7)), "l": (capi.KIND_LIGHTGLUE, Wt.make_lightglue(seed=11))}

    def context(needs):
        ctx = capi.Context(0)
        for k in needs:
            ctx.set_weights(*blobs[k])      # the shared context holds both: a fresh one finds the device copy
        return ctx

    def same(name, got, want):
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{name}: output {i} differs from a fresh context's"

    calls = _calls(capi)
    shared = context("sl")
    try:
        fresh = {}
        for name, (needs, small, large) in calls.items():
            for tag, call in (("small", small), ("large", large)):
                if call is not None:
                    ctx = context(needs)
                    fresh[name, tag] = call(ctx)
                    ctx.close()
        for name, (_, small, _) in calls.items():
            same(name + " (small, first)", small(shared), fresh[name, "small"])
        for name, (_, _, large) in calls.items():
            if large is None:
                continue
            before = shared.workspace_bytes()
            same(name + " (large)", large(shared), fresh[name, "large"])
            assert shared.workspace_bytes() > before, f"{name}: the large shape did not make the staging block grow"
        for name, (_, small, _) in calls.items():
            same(name + " (small, after the growth)", small(shared), fresh[name, "small"])
    finally:
        shared.close()
