"""GPU: octave-aware stereo matching (rfe_stereo_match_pyramid / _dev, rfe_stereo_frame_pyramid_dev, ComputeStereoMatchesPyramid_rfe)
against the contract of DESIGN.md 6c restated in tests/stereo_pyramid_ref.py.  Comparisons are exact unless a tolerance is named."""
import os
import shutil
import struct

import numpy as np
import pytest

import dropin_driver as DD
import pyramid_ref as PR
import stereo_pyramid_ref as SR
from test_stereo_pyramid_ref import MB, MBF, check_constructed, constructed_case, shifted_pair
from tolerances import LG_SCORE_TOL
from rover_slam_amd import capi, weights as Wt, synth

pytestmark = pytest.mark.gpu
FPL_1000 = [217, 181, 151, 126, 105, 87, 73, 60]


@pytest.fixture(scope="module")
def wsp():
    return Wt.make_superpoint(seed=7)


@pytest.fixture(scope="module")
def wlg():
    return Wt.make_lightglue(seed=11)


@pytest.fixture(scope="module")
def ctx(wsp, wlg):
    c = capi.Context(0)
    c.set_weights(capi.KIND_SUPERPOINT, wsp)
    c.set_weights(capi.KIND_LIGHTGLUE, wlg)
    yield c
    c.close()


def views(ex):
    """per-view features of an extract_pyramid result on [left, right]: (k, octave, desc, levels) twice"""
    out = []
    for v in range(2):
        n = int(ex["n"][v])
        out.append((ex["kpts"][v, :n], ex["octave"][v, :n], ex["desc"][v, :n], [lv[v] for lv in ex["levels"]]))
    return out


def both(ctx, H, W, L, sf, vl, vr, mode, mb=MB, mbf=MBF):
    _, _, s = capi.pyramid_geometry(H, W, L, sf)
    got = ctx.stereo_match_pyramid(vl[3], vr[3], H, W, L, sf, vl[0], vl[1], vr[0], vr[1], vl[2], vr[2], mb, mbf, mode)
    ref = SR.stereo_match(vl[3], vr[3], s, vl[0], vl[1], vr[0], vr[1], vl[2], vr[2], mb, mbf, mode)
    return got, ref


# ---------------------------------------------------------------- 1. host entry against the restatement on extracted features
@pytest.mark.parametrize("H,W,L,kmax,disp", [(240, 320, 4, 300, 17), (480, 752, 8, FPL_1000, 13)])
def test_match_vs_restatement(ctx, H, W, L, kmax, disp):
    if L == 8:
        assert PR.features_per_level(1000, 1.2, 8) == FPL_1000
    left, right = shifted_pair(H, W, disp, seed=disp)
    ex = ctx.extract_pyramid(np.stack([left, right]), nlevels=L, scale_factor=1.2, kmax=kmax, with_levels=True)
    vl, vr = views(ex)
    out = {}
    for mode in (capi.STEREO_SAD_LEVEL, capi.STEREO_SAD_LEVEL0):
        (u, z), (u_ref, z_ref) = both(ctx, H, W, L, 1.2, vl, vr, mode)
        per = [int(((u_ref >= 0) & (vl[1] == l)).sum()) for l in range(L)]
        err = np.abs((vl[0][u_ref >= 0, 0] - u_ref[u_ref >= 0]) - disp)
        print(f"{H}x{W} L={L} mode={mode}: accepted {int((u_ref >= 0).sum())} of {len(u_ref)}, per octave {per}, median error {np.median(err):.3f}")
        assert np.array_equal(u, u_ref) and np.array_equal(z, z_ref)
        out[mode] = (u, per, err)
    u, per, err = out[capi.STEREO_SAD_LEVEL]
    assert all(p > 10 for p in per), per                     # not vacuous: matches on EVERY octave
    assert np.median(err) < 0.5                              # recovered disparity against the true shift
    assert not np.array_equal(u, out[capi.STEREO_SAD_LEVEL0][0])


# ---------------------------------------------------------------- 2. one level: the single-level entry and the oracle
def test_one_level_is_rfe_stereo_match(ctx, oracle):
    H, W, disp = 120, 160, 9
    left, right = shifted_pair(H, W, disp, seed=disp)
    n, kxy, score, desc = ctx.extract(np.stack([left, right]), kmax=400)
    kl, kr = kxy[0, :n[0]].astype(np.float32), kxy[1, :n[1]].astype(np.float32)
    dl, dr = desc[0, :n[0]], desc[1, :n[1]]
    u1, z1 = ctx.stereo_match(left, right, kl, kr, dl, dr, MB, MBF)
    u_ref, z_ref = oracle.stereo_match(left, right, kl, kr, dl, dr, MB, MBF)
    assert (u_ref >= 0).sum() > 10
    for mode in (capi.STEREO_SAD_LEVEL, capi.STEREO_SAD_LEVEL0):
        u, z = ctx.stereo_match_pyramid([left], [right], H, W, 1, 1.2, kl, np.zeros(n[0], np.int32), kr, np.zeros(n[1], np.int32), dl, dr,
                                        MB, MBF, mode)
        assert np.array_equal(u, u1) and np.array_equal(z, z1)
        assert np.array_equal(u, u_ref) and np.array_equal(z, z_ref)


# ---------------------------------------------------------------- 3. device-resident entry
def dev_match(ctx, lev_l, lev_r, H, W, L, sf, kl, ol, kr, orr, dl, dr, mb, mbf, mode):
    """rfe_stereo_match_pyramid_dev on uploaded copies of host arrays"""
    up = lambda a, dt: ctx.alloc(max(np.asarray(a).size, 1) * np.dtype(dt).itemsize).upload(np.ascontiguousarray(a, dt))   # noqa: E731
    flat = lambda lv: np.concatenate([np.ascontiguousarray(a, np.uint8).reshape(-1) for a in lv])                            # noqa: E731
    N, Nr = len(kl), len(kr)
    bufs = [up(flat(lev_l), np.uint8), up(flat(lev_r), np.uint8), up(kl, np.float32), up(ol, np.int32), up(kr, np.float32), up(orr, np.int32),
            up(dl, np.float32), up(dr, np.float32), ctx.alloc(max(N, 1) * 4), ctx.alloc(max(N, 1) * 4)]
    try:
        b = [x.ptr for x in bufs]
        ctx._chk(capi.lib.rfe_stereo_match_pyramid_dev(ctx.h, b[0], b[1], H, W, L, sf, b[2], b[3], N, b[4], b[5], Nr, b[6], b[7], mb, mbf, mode,
                                                       b[8], b[9]))
        ctx.synchronize()
        return bufs[8].download((N,), np.float32), bufs[9].download((N,), np.float32)
    finally:
        for x in bufs:
            x.free()


def test_dev_entry_on_extractor_buffers(ctx):
    H, W, L, disp = 240, 320, 4, 17
    km = np.full((L,), 300, np.int32)
    K = int(km.sum())
    left, right = shifted_pair(H, W, disp, seed=disp)
    f = np.stack([left, right])
    lh, lw, _ = capi.pyramid_geometry(H, W, L, 1.2)
    frame = int((lh.astype(np.int64) * lw).sum())
    img = ctx.alloc(f.nbytes).upload(f)
    names = (("n", 8), ("kp", 2 * K * 8), ("oc", 2 * K * 4), ("sc", 2 * K * 4), ("de", 2 * K * 1024), ("lv", 2 * frame), ("u", K * 4), ("z", K * 4))
    b = {k: ctx.alloc(nb) for k, nb in names}
    try:
        ctx._chk(capi.lib.rfe_extract_pyramid_u8_dev(ctx.h, img.ptr, H, W, W, 2, L, 1.2, km.ctypes.data, 0.0005, b["n"].ptr, None, b["kp"].ptr,
                                                     b["oc"].ptr, b["sc"].ptr, b["de"].ptr, b["lv"].ptr))
        n = b["n"].download((2,), np.int32)
        nl, nr = int(n[0]), int(n[1])
        host = ctx.extract_pyramid(f, nlevels=L, scale_factor=1.2, kmax=km, with_levels=True)
        assert nl == host["n"][0] and nr == host["n"][1] and nl > 100
        vl, vr = views(host)
        for mode in (capi.STEREO_SAD_LEVEL, capi.STEREO_SAD_LEVEL0):
            ctx._chk(capi.lib.rfe_stereo_match_pyramid_dev(ctx.h, b["lv"].ptr, b["lv"].ptr + frame, H, W, L, 1.2, b["kp"].ptr, b["oc"].ptr, nl,
                                                           b["kp"].ptr + K * 8, b["oc"].ptr + K * 4, nr, b["de"].ptr, b["de"].ptr + K * 1024,
                                                           MB, MBF, mode, b["u"].ptr, b["z"].ptr))
            ctx.synchronize()
            u, z = b["u"].download((nl,), np.float32), b["z"].download((nl,), np.float32)
            uh, zh = ctx.stereo_match_pyramid(vl[3], vr[3], H, W, L, 1.2, vl[0], vl[1], vr[0], vr[1], vl[2], vr[2], MB, MBF, mode)
            assert np.array_equal(u, uh) and np.array_equal(z, zh) and (u >= 0).sum() > 100
    finally:
        img.free()
        for v in b.values():
            v.free()


def test_constructed_case_and_bad_octaves_dev(ctx):
    """the hand-built case of the CPU test through the _dev entry (which, unlike the host entry, accepts an octave outside [0, nlevels) and
    treats it as no match / not a candidate), each run equal to the restatement"""
    def run(c, octr, mb, mbf, mode):
        got = dev_match(ctx, c["lev_l"], c["lev_r"], c["H"], c["W"], c["L"], c["sf"], c["kl"], c["ol"], c["kr"], octr, c["dl"], c["dr"], mb, mbf, mode)
        ref = SR.stereo_match(c["lev_l"], c["lev_r"], c["s"], c["kl"], c["ol"], c["kr"], octr, c["dl"], c["dr"], mb, mbf, mode)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        return got
    check_constructed(run)


# ---------------------------------------------------------------- 4. the fused per-frame entry
def frame_pair(scene, rng, H, W, x0, disp):
    left = np.clip(scene[:, x0:x0 + W] + rng.integers(0, 8, (H, W)), 0, 255).astype(np.uint8)
    right = np.clip(scene[:, x0 + disp:x0 + disp + W] + rng.integers(0, 8, (H, W)), 0, 255).astype(np.uint8)
    return left, right


def push_padded(ctx, st, left, right, pad, reset=False):
    H, W = left.shape
    wide = np.full((2, H, W + pad), 255, np.uint8)          # device images with a row pitch > W, like a cv::Mat ROI
    wide[0, :, :W], wide[1, :, :W] = left, right
    dimg = ctx.alloc(wide.nbytes).upload(wide)
    try:
        st.push(dimg.ptr, dimg.ptr + H * (W + pad), stride=W + pad, reset=reset)
        return st.results()
    finally:
        dimg.free()


@pytest.mark.parametrize("H,W,L,kmax", [(240, 320, 4, [150, 120, 100, 80]), (480, 752, 8, FPL_1000)])
def test_stereo_frame_pyramid_stream_vs_oracle(ctx, wsp, wlg, oracle, H, W, L, kmax):
    rng = np.random.default_rng(H)
    disp, T = 13, 3
    scene = synth.make_scene(rng, H, W + disp + 8 * T, margin=0)
    _, _, s = capi.pyramid_geometry(H, W, L, 1.2)
    st = capi.StereoPyramidStream(ctx, H, W, L, 1.2, kmax, mb=MB, mbf=MBF)
    K = st.K
    prev = None
    for t in range(T):
        left, right = frame_pair(scene, rng, H, W, 6 * t, disp)
        got = push_padded(ctx, st, left, right, 24)
        ref = PR.extract(oracle, wsp, np.stack([left, right]), L, 1.2, kmax)
        for k in ("n", "level_n", "kpts", "octave", "score", "desc"):
            assert np.array_equal(got[k], ref[k]), k
        nl, nr = int(ref["n"][0]), int(ref["n"][1])
        lev = [[lv[v] for lv in ref["levels"]] for v in range(2)]
        u_ref, z_ref = SR.stereo_match(lev[0], lev[1], s, ref["kpts"][0, :nl], ref["octave"][0, :nl], ref["kpts"][1, :nr], ref["octave"][1, :nr],
                                       ref["desc"][0, :nl], ref["desc"][1, :nr], MB, MBF, SR.SAD_LEVEL)
        assert np.array_equal(got["u_right"][:nl], u_ref) and np.array_equal(got["depth"][:nl], z_ref)
        assert (got["u_right"][nl:] == -1).all() and (got["depth"][nl:] == -1).all()
        assert (u_ref >= 0).sum() > 10
        cur = (ref["kpts"][0, :nl].copy(), ref["desc"][0, :nl].copy())
        if prev is None:
            assert got["S"] == 0
        else:
            lg = oracle.lightglue(wlg, oracle.normalize_keypoints(cur[0], H, W), oracle.normalize_keypoints(prev[0], H, W), cur[1], prev[1])
            assert got["S"] == lg["S"] and lg["S"] > 0 and np.array_equal(got["pairs"][:lg["S"]], lg["pairs"])
            assert np.abs(got["ms"][:lg["S"]] - lg["ms"]).max() < LG_SCORE_TOL       # the stated fp32 tolerance (tests/tolerances.py)
        prev = cur
    # a new sequence starts (S = 0) after reset, ...
    assert push_padded(ctx, st, left, right, 0, reset=True)["S"] == 0
    again = push_padded(ctx, st, left, right, 0)
    assert again["S"] > 0                                    # (the sequence then continues: same view against itself)
    # ... after a change of kmax (no reset flag), ...
    km2 = list(kmax); km2[0] -= 1; km2[-1] += 1             # same total, another split
    st2 = capi.StereoPyramidStream(ctx, H, W, L, 1.2, km2, mb=MB, mbf=MBF)
    st2.first = False
    assert push_padded(ctx, st2, left, right, 0)["S"] == 0
    assert push_padded(ctx, st2, left, right, 0)["S"] > 0
    # ... and after an rfe_stereo_frame_dev call on the same ctx, in both directions
    single = capi.StereoStream(ctx, H, W, K, mb=MB, mbf=MBF)
    single.first = False
    wide = np.ascontiguousarray(np.stack([left, right]))
    dimg = ctx.alloc(wide.nbytes).upload(wide)
    single.push(dimg.ptr, dimg.ptr + H * W)
    assert single.results()["S"] == 0
    assert push_padded(ctx, st2, left, right, 0)["S"] == 0
    single.push(dimg.ptr, dimg.ptr + H * W)
    assert single.results()["S"] == 0
    dimg.free()
    # the other SAD source through the fused entry (last frame; the stereo outputs do not depend on the sequence)
    st0 = capi.StereoPyramidStream(ctx, H, W, L, 1.2, kmax, mb=MB, mbf=MBF, sad_source=capi.STEREO_SAD_LEVEL0)
    got = push_padded(ctx, st0, left, right, 24)
    u0, z0 = SR.stereo_match(lev[0], lev[1], s, ref["kpts"][0, :nl], ref["octave"][0, :nl], ref["kpts"][1, :nr], ref["octave"][1, :nr],
                             ref["desc"][0, :nl], ref["desc"][1, :nr], MB, MBF, SR.SAD_LEVEL0)
    assert got["S"] == 0 and np.array_equal(got["u_right"][:nl], u0) and np.array_equal(got["depth"][:nl], z0)
    assert not np.array_equal(u0, u_ref)
    for x in (st, st2, single, st0):
        x.close()


# ---------------------------------------------------------------- 5. degenerate shapes
def test_small_and_empty_levels_and_empty_sets(ctx, wsp, oracle):
    H, W, L, sf, disp = 64, 64, 5, 2.0, 5                   # levels 64, 32, 16, 8, 4: the last one is too small to run
    kmax = [64, 0, 32, 16, 16]                              # and level 1 has no budget
    left, right = shifted_pair(H, W, disp, seed=3)
    ex = ctx.extract_pyramid(np.stack([left, right]), nlevels=L, scale_factor=sf, kmax=kmax, with_levels=True)
    assert ex["level_n"][0, 1] == 0 and ex["level_n"][0, 4] == 0 and ex["level_n"][0, 0] > 0 and ex["level_n"][0, 2] > 0 and ex["n"][0] < sum(kmax)
    vl, vr = views(ex)
    for mode in (capi.STEREO_SAD_LEVEL, capi.STEREO_SAD_LEVEL0):
        (u, z), (u_ref, z_ref) = both(ctx, H, W, L, sf, vl, vr, mode)
        assert np.array_equal(u, u_ref) and np.array_equal(z, z_ref)
    # Nr = 0
    u, z = ctx.stereo_match_pyramid(vl[3], vr[3], H, W, L, sf, vl[0], vl[1], vr[0][:0], vr[1][:0], vl[2], vr[2][:0], MB, MBF)
    assert len(u) == len(vl[0]) and (u == -1).all() and (z == -1).all()
    # N = 0
    u, z = ctx.stereo_match_pyramid(vl[3], vr[3], H, W, L, sf, vl[0][:0], vl[1][:0], vr[0], vr[1], vl[2][:0], vr[2], MB, MBF)
    assert len(u) == 0 and len(z) == 0
    # the fused entry on the same degenerate level set; then with views that have no keypoints (a threshold no score reaches)
    st = capi.StereoPyramidStream(ctx, H, W, L, sf, kmax, mb=MB, mbf=MBF)
    got = push_padded(ctx, st, left, right, 8)
    ref = PR.extract(oracle, wsp, np.stack([left, right]), L, sf, kmax)
    for k in ("n", "level_n", "kpts", "octave", "score", "desc"):
        assert np.array_equal(got[k], ref[k]), k
    nl = int(got["n"][0])
    (_, _), (u_ref, z_ref) = both(ctx, H, W, L, sf, vl, vr, capi.STEREO_SAD_LEVEL)
    assert np.array_equal(got["u_right"][:nl], u_ref) and np.array_equal(got["depth"][:nl], z_ref) and (got["u_right"][nl:] == -1).all()
    st.close()
    st = capi.StereoPyramidStream(ctx, H, W, L, sf, kmax, mb=MB, mbf=MBF, thr=2.0)
    for _ in range(2):                                      # the second call matches an empty view against an empty previous view
        got = push_padded(ctx, st, left, right, 8)
        assert got["n"].tolist() == [0, 0] and got["S"] == 0
        assert (got["u_right"] == -1).all() and (got["depth"] == -1).all()
    st.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(ctx):
    c = constructed_case()
    a = (c["lev_l"], c["lev_r"], c["H"], c["W"], c["L"], c["sf"], c["kl"], c["ol"], c["kr"], c["orr"], c["dl"], c["dr"])
    def refused(msg, *args, **kw):
        with pytest.raises(capi.RfeError) as e:
            ctx.stereo_match_pyramid(*args, **kw)
        assert "error -1" in str(e.value) and msg in str(e.value), str(e.value)
    refused("sad_source", *a, MB, MBF, 2)
    refused("mb", *a, 0.0, MBF)
    big = 4097
    kb, ob, db = np.zeros((big, 2), np.float32), np.zeros((big,), np.int32), np.zeros((big, 256), np.float32)
    refused("4096", *a[:6], kb, ob, c["kr"], c["orr"], db, c["dr"], MB, MBF)
    refused("4096", *a[:6], c["kl"], c["ol"], kb, ob, c["dl"], db, MB, MBF)
    bad = c["orr"].copy(); bad[1] = c["L"]
    refused("octave", *a[:9], bad, c["dl"], c["dr"], MB, MBF)
    badl = c["ol"].copy(); badl[0] = -1
    refused("octave", *a[:7], badl, c["kr"], c["orr"], c["dl"], c["dr"], MB, MBF)
    with pytest.raises(capi.RfeError):                       # geometry rfe_pyramid_geometry refuses
        ctx.stereo_match_pyramid(c["lev_l"], c["lev_r"], c["H"], c["W"], c["L"], 1.0, *a[6:], MB, MBF)
    # the _dev entry validates the same scalars before touching a pointer
    lib, h = capi.lib, ctx.h
    o = np.zeros((16,), np.float32).ctypes.data
    dev = lambda L=3, sf=1.5, N=4, Nr=4, mb=MB, mode=0: lib.rfe_stereo_match_pyramid_dev(   # noqa: E731
        h, o, o, 96, 240, L, sf, o, o, N, o, o, Nr, o, o, mb, MBF, mode, o, o)
    for kw, m in ((dict(mode=2), "sad_source"), (dict(mode=-1), "sad_source"), (dict(N=4097), "4096"), (dict(Nr=4097), "4096"), (dict(N=-1), "4096"),
                  (dict(mb=0.0), "mb"), (dict(L=17), "nlevels"), (dict(L=0), "nlevels"), (dict(sf=1.0), "scale_factor")):
        assert dev(**kw) == -1 and m in lib.rfe_last_error(h).decode(), (kw, lib.rfe_last_error(h).decode())
    assert lib.rfe_stereo_match_pyramid_dev(h, None, o, 96, 240, 3, 1.5, o, o, 4, o, o, 4, o, o, MB, MBF, 0, o, o) == -1
    assert "null" in lib.rfe_last_error(h).decode()
    # the fused entry: Ktot above 4096, a bad sad_source, mb = 0
    km = np.array([2048, 2048, 1], np.int32)
    fr = lambda kmp=km.ctypes.data, mode=0, mb=MB: lib.rfe_stereo_frame_pyramid_dev(   # noqa: E731
        h, o, o, 96, 240, 240, 3, 1.5, kmp, 0.0005, 0.1, mb, MBF, mode, 0, o, None, o, o, o, o, o, o, o, o, o)
    assert fr() == -1 and "4096" in lib.rfe_last_error(h).decode()
    ok = np.array([8, 8, 8], np.int32)
    assert fr(kmp=ok.ctypes.data, mode=2) == -1 and "sad_source" in lib.rfe_last_error(h).decode()
    assert fr(kmp=ok.ctypes.data, mb=0.0) == -1 and "mb" in lib.rfe_last_error(h).decode()
    u, _ = ctx.stereo_match_pyramid(*a, MB, MBF)             # the ctx is still usable
    assert (u >= 0).sum() >= 3


# ---------------------------------------------------------------- 7. the drop-in helper
def read_driver(path):
    buf = open(path, "rb").read()
    L = struct.unpack_from("<i", buf, 0)[0]; off = 4
    vs = []
    for _ in range(2):
        n = struct.unpack_from("<i", buf, off)[0]; off += 4
        k = np.frombuffer(buf, np.float32, n * 2, off).reshape(n, 2); off += 8 * n
        o = np.frombuffer(buf, np.int32, n, off); off += 4 * n
        d = np.frombuffer(buf, np.float32, n * 256, off).reshape(n, 256); off += 1024 * n
        lv = []
        for _ in range(L):
            r, c = struct.unpack_from("<ii", buf, off); off += 8
            lv.append(np.frombuffer(buf, np.uint8, r * c, off).reshape(r, c)); off += r * c
        vs.append((k, o, d, lv))
    n = len(vs[0][0])
    res = []
    for _ in range(3):
        st = struct.unpack_from("<i", buf, off)[0]; off += 4
        u = np.frombuffer(buf, np.float32, n, off); off += 4 * n
        z = np.frombuffer(buf, np.float32, n, off); off += 4 * n
        res.append((st, u, z))
    assert off == len(buf)
    return L, vs, res


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_helper(tmp_path, ctx, wsp):
    H, W, disp = 480, 752, 13
    Wt.save(str(tmp_path / "sp.rfew"), wsp, 1, {"max_keypoints": 400})
    left, right = shifted_pair(H, W, disp, seed=disp)
    left.tofile(str(tmp_path / "left.u8")); right.tofile(str(tmp_path / "right.u8"))
    env = dict(os.environ, RFE_SP_WEIGHTS=str(tmp_path / "sp.rfew"))
    exe = DD.build(tmp_path, "stereo_pyramid_driver", ("RFE_SP_PYRAMID=1",))
    for L in (8, 1):
        out = str(tmp_path / f"out{L}.bin")
        DD.run(exe, str(tmp_path / "left.u8"), str(tmp_path / "right.u8"), H, W, L, out, env=env)
        Ld, (vl, vr), res = read_driver(out)
        assert Ld == L and len(vl[0]) > 100 and len(vr[0]) > 100
        assert np.array_equal(vl[3][0], left) and np.array_equal(vr[3][0], right)
        for mode in (capi.STEREO_SAD_LEVEL, capi.STEREO_SAD_LEVEL0):
            u, z = ctx.stereo_match_pyramid(vl[3], vr[3], H, W, L, 1.2, vl[0], vl[1], vr[0], vr[1], vl[2], vr[2], MB, MBF, mode)
            st, ud, zd = res[mode]
            assert st == 0 and np.array_equal(ud, u) and np.array_equal(zd, z) and (u >= 0).sum() > 50
        st1, u1, z1 = res[2]                                 # ComputeStereoMatches_rfe on the same frame
        if L == 1:
            assert (vl[1] == 0).all() and st1 == 0 and np.array_equal(u1, res[0][1]) and np.array_equal(z1, res[0][2])
            us, zs = ctx.stereo_match(left, right, vl[0], vr[0], vl[2], vr[2], MB, MBF)
            assert np.array_equal(u1, us) and np.array_equal(z1, zs)
        else:
            assert (vl[1] > 0).any() and st1 == -1 and (u1 == -1).all() and (z1 == -1).all()
            assert not np.array_equal(res[0][1], res[1][1])
