"""GPU: SuperPoint on a scale pyramid (rfe_extract_pyramid_u8 / _dev, SPextractor with RFE_SP_PYRAMID=1) against the contract of
DESIGN.md 6b restated in tests/pyramid_ref.py: level images bit for bit, the merged output against the oracle composed per level,
GPU-vs-GPU agreement with rfe_extract_u8 per level, the refusals, and the drop-in class.  Comparisons are exact unless a tolerance is named."""
import os
import shutil
import struct

import numpy as np
import pytest

import dropin_driver as DD
import pyramid_ref as P
from tolerances import LG_SCORE_TOL
from rover_slam_amd import capi, weights as Wt, synth

pytestmark = pytest.mark.gpu
FPL_1000 = [217, 181, 151, 126, 105, 87, 73, 60]


@pytest.fixture(scope="module")
def wsp():
    return Wt.make_superpoint(seed=7)


@pytest.fixture(scope="module")
def ctx(wsp):
    c = capi.Context(0)
    c.set_weights(capi.KIND_SUPERPOINT, wsp)
    yield c
    c.close()


def textured(B, H, W, seed):
    if H >= 64 and W >= 64:
        return synth.make_frames(B, H, W, seed=seed)[0]
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (B, H, W)).astype(np.uint8)


def assert_same(got, ref, B, L):
    assert np.array_equal(got["n"], ref["n"])
    assert np.array_equal(got["level_n"], ref["level_n"])
    assert np.array_equal(got["kpts"], ref["kpts"])
    assert np.array_equal(got["octave"], ref["octave"])
    assert np.array_equal(got["score"], ref["score"])
    assert np.array_equal(got["desc"], ref["desc"])


# ---------------------------------------------------------------- 1. level images
@pytest.mark.parametrize("B,H,W,L,sf,pad", [(1, 480, 640, 8, 1.2, 0), (2, 480, 752, 8, 1.2, 0), (1, 376, 1241, 8, 1.2, 0),
                                            (1, 105, 73, 8, 1.5, 0), (1, 64, 64, 5, 2.0, 0), (2, 120, 160, 4, 1.2, 13)])
def test_level_images_match_reference(ctx, B, H, W, L, sf, pad):
    frames = textured(B, H, W, seed=H + W)
    out = ctx.extract_pyramid(frames, nlevels=L, scale_factor=sf, kmax=64, with_levels=True, pad_cols=pad)
    ref = P.build(frames, L, sf)
    lh, lw, _ = P.geometry(H, W, L, sf)
    assert len(out["levels"]) == L
    for l in range(L):
        assert out["levels"][l].shape == (B, lh[l], lw[l])
        assert np.array_equal(out["levels"][l], ref[l]), l
    if (H, W) == (105, 73):
        assert lh[6] < 8 or lw[6] < 8
        assert (out["level_n"][:, 6:] == 0).all()
    if (H, W) == (64, 64):
        assert out["levels"][4].shape[1:] == (4, 4)


# ---------------------------------------------------------------- 2. whole output against the oracle
@pytest.mark.parametrize("B,H,W,L,sf,kmax", [(1, 240, 320, 8, 1.2, FPL_1000), (1, 480, 640, 8, 1.2, FPL_1000),
                                             (3, 120, 160, 4, 2.0, [128, 96, 64, 32]),     # B <= 4: fused detector tail
                                             (5, 120, 160, 4, 2.0, [128, 96, 64, 32])])    # B > 4: separate launches
def test_output_matches_oracle(ctx, wsp, oracle, B, H, W, L, sf, kmax):
    frames = textured(B, H, W, seed=B * 100 + H)
    got = ctx.extract_pyramid(frames, nlevels=L, scale_factor=sf, kmax=kmax)
    ref = P.extract(oracle, wsp, frames, L, sf, kmax)
    assert_same(got, ref, B, L)
    assert (got["n"] > 0).all()


def test_black_and_half_constant_frames(ctx, wsp, oracle):
    H, W = 240, 320
    f = textured(2, H, W, seed=5)
    f[0] = 0
    f[1, :, : W // 2] = 128
    got = ctx.extract_pyramid(f, nlevels=8, scale_factor=1.2, kmax=FPL_1000)
    ref = P.extract(oracle, wsp, f, 8, 1.2, FPL_1000)
    assert_same(got, ref, 2, 8)


def test_other_hyper_parameters(wsp, oracle):
    c = capi.Context(0)
    try:
        c.set_weights(capi.KIND_SUPERPOINT, wsp)
        c.set_hparams(sp_nms_radius=3, sp_remove_borders=8, sp_topk_always=1)
        f = textured(2, 240, 320, seed=9)
        got = c.extract_pyramid(f, nlevels=6, scale_factor=1.2, kmax=[100, 80, 60, 50, 40, 30])
        ref = P.extract(oracle, wsp, f, 6, 1.2, [100, 80, 60, 50, 40, 30], nms_radius=3, border=8, topk_always=True)
        assert_same(got, ref, 2, 6)
    finally:
        c.close()


# ---------------------------------------------------------------- 3. / 4. against rfe_extract_u8
def test_one_level_is_plain_extract(ctx):
    f = textured(2, 240, 320, seed=11)
    got = ctx.extract_pyramid(f, nlevels=1, scale_factor=1.2, kmax=300)
    n, kxy, score, desc = ctx.extract(f, kmax=300)
    assert np.array_equal(got["n"], n) and np.array_equal(got["level_n"][:, 0], n)
    assert np.array_equal(got["kpts"], kxy.astype(np.float32))
    assert (got["octave"] == 0).all()
    assert np.array_equal(got["score"], score) and np.array_equal(got["desc"], desc)


def test_every_level_is_plain_extract_of_its_image(ctx):
    f = textured(1, 480, 640, seed=12)
    got = ctx.extract_pyramid(f, nlevels=8, scale_factor=1.2, kmax=FPL_1000, with_levels=True)
    _, _, s = P.geometry(480, 640, 8, 1.2)
    row = 0
    for l in range(8):
        n, kxy, score, desc = ctx.extract(got["levels"][l], kmax=FPL_1000[l])
        k = int(n[0])
        assert got["level_n"][0, l] == k
        seg = slice(row, row + k)
        assert np.array_equal(got["kpts"][0, seg], kxy[0, :k].astype(np.float32) * s[l])
        assert (got["octave"][0, seg] == l).all()
        assert np.array_equal(got["score"][0, seg], score[0, :k]) and np.array_equal(got["desc"][0, seg], desc[0, :k])
        row += k
    assert got["n"][0] == row
    assert not got["kpts"][0, row:].any() and not got["desc"][0, row:].any() and not got["score"][0, row:].any()


# ---------------------------------------------------------------- 5. device form, repeatability, no effect on other entries
def run_dev(ctx, frames, L, sf, kmax, with_levels):
    B, H, W = frames.shape
    km = np.ascontiguousarray(kmax, np.int32)
    K = int(km.sum())
    lh, lw, _ = P.geometry(H, W, L, sf)
    tot = int((lh.astype(np.int64) * lw).sum())
    img = ctx.alloc(frames.nbytes).upload(frames)
    bufs = {k: ctx.alloc(max(nb, 4)) for k, nb in (("n", B * 4), ("ln", B * L * 4), ("kp", B * K * 8), ("oc", B * K * 4), ("sc", B * K * 4),
                                                   ("de", B * K * 1024), ("lv", B * tot))}
    try:
        ctx._chk(capi.lib.rfe_extract_pyramid_u8_dev(ctx.h, img.ptr, H, W, W, B, L, sf, km.ctypes.data, 0.0005, bufs["n"].ptr, bufs["ln"].ptr,
                                                     bufs["kp"].ptr, bufs["oc"].ptr, bufs["sc"].ptr, bufs["de"].ptr,
                                                     bufs["lv"].ptr if with_levels else None))
        ctx.synchronize()
        out = {"n": bufs["n"].download((B,), np.int32), "level_n": bufs["ln"].download((B, L), np.int32),
               "kpts": bufs["kp"].download((B, K, 2), np.float32), "octave": bufs["oc"].download((B, K), np.int32),
               "score": bufs["sc"].download((B, K), np.float32), "desc": bufs["de"].download((B, K, 256), np.float32)}
        if with_levels:
            out["levels"] = capi.split_levels(bufs["lv"].download((B, tot), np.uint8), lh, lw)
        return out
    finally:
        img.free()
        for b in bufs.values():
            b.free()


def test_dev_form_matches_host_and_repeats(ctx):
    f = textured(2, 240, 320, seed=13)
    host = ctx.extract_pyramid(f, nlevels=8, scale_factor=1.2, kmax=FPL_1000, with_levels=True)
    dev_lv = run_dev(ctx, f, 8, 1.2, FPL_1000, True)
    dev = run_dev(ctx, f, 8, 1.2, FPL_1000, False)
    again = ctx.extract_pyramid(f, nlevels=8, scale_factor=1.2, kmax=FPL_1000)
    for other in (dev_lv, dev, again):
        assert_same(other, host, 2, 8)
    for a, b in zip(dev_lv["levels"], host["levels"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("host_graph", [0, 1])
def test_plain_extract_unchanged_around_pyramid_calls(wsp, host_graph):
    c = capi.Context(0)
    try:
        c.set_weights(capi.KIND_SUPERPOINT, wsp)
        c.set_option(capi.OPT_HOST_GRAPH, host_graph)
        f = textured(1, 240, 320, seed=14)
        before = [c.extract(f, kmax=512) for _ in range(4)]     # enough repeats for a captured graph
        c.extract_pyramid(textured(2, 480, 640, seed=15), nlevels=8, scale_factor=1.2, kmax=FPL_1000)
        after = [c.extract(f, kmax=512) for _ in range(4)]
        for r in before[1:] + after:
            for x, y in zip(r, before[0]):
                assert np.array_equal(x, y)
    finally:
        c.close()


# ---------------------------------------------------------------- 6. end to end: merged device output into LightGlue
def test_merged_output_feeds_lightglue(ctx, oracle):
    wlg = Wt.make_lightglue(seed=11)
    ctx.set_weights(capi.KIND_LIGHTGLUE, wlg)
    H, W, L = 240, 320, 8
    f = synth.make_frames(2, H, W, seed=16, max_shift=16, shift_step=8)[0]
    km = np.array(FPL_1000, np.int32)
    K = int(km.sum())
    img = ctx.alloc(f.nbytes).upload(f)
    names = (("n", 8), ("kp", 2 * K * 8), ("oc", 2 * K * 4), ("sc", 2 * K * 4), ("de", 2 * K * 1024), ("kn", 2 * K * 8), ("S", 4),
             ("pairs", K * 8), ("ms", K * 4))
    b = {k: ctx.alloc(nb) for k, nb in names}
    try:
        ctx._chk(capi.lib.rfe_extract_pyramid_u8_dev(ctx.h, img.ptr, H, W, W, 2, L, 1.2, km.ctypes.data, 0.0005, b["n"].ptr, None, b["kp"].ptr,
                                                     b["oc"].ptr, b["sc"].ptr, b["de"].ptr, None))
        n = b["n"].download((2,), np.int32)
        kp = b["kp"].download((2, K, 2), np.float32)
        kn = np.stack([oracle.normalize_keypoints(kp[i], H, W) for i in range(2)])
        b["kn"].upload(kn)
        ctx._chk(capi.lib.rfe_match_dev(ctx.h, b["kn"].ptr, b["kn"].ptr + K * 8, b["de"].ptr, b["de"].ptr + K * 1024, b["n"].ptr, b["n"].ptr + 4,
                                        1, K, K, 0.1, b["S"].ptr, b["pairs"].ptr, b["ms"].ptr))
        S = int(b["S"].download((1,), np.int32)[0])
        pairs = b["pairs"].download((K, 2), np.int32)[:S]
        ms = b["ms"].download((K,), np.float32)[:S]
        desc = b["de"].download((2, K, 256), np.float32)
        r = oracle.lightglue(wlg, kn[0, :n[0]], kn[1, :n[1]], desc[0, :n[0]], desc[1, :n[1]])
        assert S == r["S"] and S > 0 and np.array_equal(pairs, r["pairs"])
        assert np.abs(ms - r["ms"]).max() <= LG_SCORE_TOL
    finally:
        img.free()
        for v in b.values():
            v.free()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(ctx):
    f = np.zeros((1, 64, 64), np.uint8)
    bad = [dict(nlevels=0, kmax=[8]), dict(nlevels=17, kmax=[8] * 17), dict(nlevels=4, scale_factor=1.0, kmax=[8] * 4),
           dict(nlevels=4, scale_factor=4.5, kmax=[8] * 4), dict(nlevels=2, kmax=[8, 4097]), dict(nlevels=2, kmax=[8, -1]),
           dict(nlevels=2, kmax=[0, 0])]
    msgs = ["nlevels", "nlevels", "scale_factor", "scale_factor", "kmax", "kmax", "kmax"]
    for kw, m in zip(bad, msgs):
        with pytest.raises(capi.RfeError) as e:
            ctx.extract_pyramid(f, scale_factor=kw.pop("scale_factor", 1.2), **kw)
        assert "error -1" in str(e.value) and m in str(e.value), (kw, str(e.value))
    with pytest.raises(capi.RfeError) as e:      # 16 x 16 at 4.0: level 2 is 1 x 1, level 3 rounds to zero pixels
        ctx.extract_pyramid(np.zeros((1, 16, 16), np.uint8), nlevels=4, scale_factor=4.0, kmax=8)
    assert "error -1" in str(e.value) and "zero pixels" in str(e.value)
    km = np.array([8, 8], np.int32)
    o = np.zeros((4096,), np.float32)
    lib, h = capi.lib, ctx.h
    args = lambda img=f.ctypes.data, H=64, W=64, stride=64, B=1, kmp=km.ctypes.data, nn=o.ctypes.data: (  # noqa: E731
        h, img, H, W, stride, B, 2, 2.0, kmp, 0.0005, nn, None, o.ctypes.data, o.ctypes.data, o.ctypes.data, o.ctypes.data, None)
    for a, m in ((args(H=7), "at least 8"), (args(W=7), "at least 8"), (args(B=0), "B > 0"), (args(stride=63), "stride"),
                 (args(img=None), "null"), (args(kmp=None), "null"), (args(nn=None), "null")):
        assert lib.rfe_extract_pyramid_u8(*a) == -1
        assert m in lib.rfe_last_error(h).decode()
        assert lib.rfe_extract_pyramid_u8_dev(*a) == -1
    c = capi.Context(0)
    try:
        assert lib.rfe_extract_pyramid_u8(c.h, *args()[1:]) == -5
        assert "weights" in lib.rfe_last_error(c.h).decode()
    finally:
        c.close()
    ctx.extract_pyramid(f, nlevels=2, scale_factor=2.0, kmax=8)     # the ctx is still usable


# ---------------------------------------------------------------- 8. the drop-in class
def read_driver(path):
    buf = open(path, "rb").read()
    off = 0
    n = struct.unpack_from("<i", buf, off)[0]; off += 4
    kp = np.frombuffer(buf, np.float32, n * 4, off).reshape(n, 4); off += 16 * n
    octave = np.frombuffer(buf, np.int32, n, off); off += 4 * n
    desc = np.frombuffer(buf, np.float32, n * 256, off).reshape(n, 256); off += 1024 * n
    L = struct.unpack_from("<i", buf, off)[0]; off += 4
    levels = []
    for _ in range(L):
        r, c = struct.unpack_from("<ii", buf, off); off += 8
        levels.append(np.frombuffer(buf, np.uint8, r * c, off).reshape(r, c)); off += r * c
    st, unset = struct.unpack_from("<ii", buf, off)
    return n, kp, octave, desc, levels, st, unset


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_spextractor_pyramid_opt_in(tmp_path, ctx, wsp, oracle):
    H, W, cap = 480, 640, 200
    Wt.save(str(tmp_path / "sp.rfew"), wsp, 1, {"max_keypoints": cap})
    f = textured(1, H, W, seed=17)
    f.tofile(str(tmp_path / "frame.u8"))
    env = dict(os.environ, RFE_SP_WEIGHTS=str(tmp_path / "sp.rfew"))
    kmax = [min(k, cap) for k in P.features_per_level(1000, 1.2, 8)]
    assert kmax == [200, 181, 151, 126, 105, 87, 73, 60]
    api = ctx.extract_pyramid(f, nlevels=8, scale_factor=1.2, kmax=kmax, with_levels=True)
    ref = P.extract(oracle, wsp, f, 8, 1.2, kmax)
    assert_same(api, ref, 1, 8)
    results = {}
    for macro in (True, False):
        exe = DD.build(tmp_path, "pyramid_driver", ("RFE_SP_PYRAMID=1",) if macro else ())
        out = str(tmp_path / ("out_on.bin" if macro else "out_off.bin"))
        DD.run(exe, str(tmp_path / "frame.u8"), H, W, out, env=env)
        results[macro] = read_driver(out)
    n, kp, octave, desc, levels, st, unset = results[True]
    N = int(api["n"][0])
    assert n == N > 0
    assert np.array_equal(kp[:, :2], api["kpts"][0, :N]) and np.array_equal(kp[:, 2], api["score"][0, :N]) and (kp[:, 3] == 10).all()
    assert np.array_equal(octave, api["octave"][0, :N]) and (octave > 0).any()
    assert np.array_equal(desc, api["desc"][0, :N])
    assert len(levels) == 8 and all(np.array_equal(levels[l], api["levels"][l][0]) for l in range(8))
    assert st == -1 and unset == 1          # ComputeStereoMatches_rfe refuses octave > 0 keypoints
    n0, _, _, _, levels0, st0, _ = results[False]
    assert n0 == 0 and st0 == 0             # without the macro: the reference's no-op
    assert all(lv.size == 0 for lv in levels0)
