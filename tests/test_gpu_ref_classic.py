"""GPU: the HIP stereo and map-point helpers against what Rover-SLAM's own C++ computed (tests/golden/ref_*.npz, recorded by
tools/gen_ref_golden.py through oracle/ref_classic; tests/test_ref_classic.py holds the CPU checkers to the same recordings).  Reads
fixtures only.  Stereo outputs are compared as uint32 views: bit for bit, -1 and NaN included.  The last test is against the oracle, not
the reference (whose N x N stack array stops near 512 observations): rfe_distinctive_descriptors at its documented bound."""
import numpy as np
import pytest

import ref_classic_cases as RC
from rover_slam_amd import capi
from test_ref_classic import check_distance

pytestmark = pytest.mark.gpu
SINGLE = [n for n in RC.STEREO_FIXTURES if n[0] in "abc"]
PYRAMID = [n for n in RC.STEREO_FIXTURES if n[0] == "d"]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def up(ctx, a, dt):
    a = np.ascontiguousarray(a, dt)
    return ctx.alloc(max(a.nbytes, 16)).upload(a)


def padded(img, pad, fill=255):
    wide = np.full((img.shape[0], img.shape[1] + pad), fill, np.uint8)
    wide[:, :img.shape[1]] = img
    return wide


def flat_levels(case, fill):
    ll, lr = RC.levels_of(case, fill)
    return np.concatenate([a.reshape(-1) for a in ll]), np.concatenate([a.reshape(-1) for a in lr])


def same(got, u_ref, z_ref, what):
    u, z = got
    bad = np.nonzero(np.ascontiguousarray(u).view(np.uint32) != u_ref.view(np.uint32))[0]
    assert RC.same_bits(u, u_ref) and RC.same_bits(z, z_ref), f"{what}: differs from the reference at left keypoints {bad[:10].tolist()}"


# ---------------------------------------------------------------- single level: families (a), (b), (c)
@pytest.mark.parametrize("name", SINGLE)
def test_stereo_match_equals_reference(ctx, name):
    c, u_ref, z_ref, cen = RC.load_stereo(name)
    assert c["nlevels"] == 1 and cen["survivors"] >= 1
    H, W = c["img_l"].shape
    N, Nr = len(c["k_l"]), len(c["k_r"])
    same(ctx.stereo_match(c["img_l"], c["img_r"], c["k_l"], c["k_r"], c["d_l"], c["d_r"], c["mb"], c["mbf"]), u_ref, z_ref, "rfe_stereo_match")
    # the device entry, images with a row pitch above W (like a cv::Mat ROI)
    pad = 24
    bufs = [up(ctx, padded(c["img_l"], pad), np.uint8), up(ctx, padded(c["img_r"], pad, 0), np.uint8), up(ctx, c["k_l"], np.float32),
            up(ctx, c["k_r"], np.float32), up(ctx, c["d_l"], np.float32), up(ctx, c["d_r"], np.float32), ctx.alloc(max(N, 4) * 4), ctx.alloc(max(N, 4) * 4)]
    try:
        b = [x.ptr for x in bufs]
        ctx._chk(capi.lib.rfe_stereo_match_dev(ctx.h, b[0], b[1], H, W, W + pad, b[2], N, b[3], Nr, b[4], b[5], c["mb"], c["mbf"], b[6], b[7]))
        ctx.synchronize()
        same((bufs[6].download((N,), np.float32), bufs[7].download((N,), np.float32)), u_ref, z_ref, "rfe_stereo_match_dev")
    finally:
        for x in bufs:
            x.free()
    # the pyramid entry with one level, both patch sources (they coincide at one level)
    for mode in (capi.STEREO_SAD_LEVEL, capi.STEREO_SAD_LEVEL0):
        got = ctx.stereo_match_pyramid([c["img_l"]], [c["img_r"]], H, W, 1, 1.2, c["k_l"], c["o_l"], c["k_r"], c["o_r"], c["d_l"], c["d_r"],
                                       c["mb"], c["mbf"], mode)
        same(got, u_ref, z_ref, f"rfe_stereo_match_pyramid(nlevels=1, sad_source={mode})")


# ---------------------------------------------------------------- the pyramid as written: family (d)
@pytest.mark.parametrize("name", PYRAMID)
def test_stereo_match_pyramid_level0_equals_reference(ctx, name):
    c, u_ref, z_ref, cen = RC.load_stereo(name)
    H, W = c["img_l"].shape
    L, sf = c["nlevels"], c["scale_factor"]
    N, Nr = len(c["k_l"]), len(c["k_r"])
    assert L > 1 and len(cen["survivor_octaves"]) >= 3
    for fill in (0, 200):                    # levels >= 1 hold a constant: with RFE_STEREO_SAD_LEVEL0 nothing but level 0 may be read
        fl, fr = flat_levels(c, fill)
        got = ctx.stereo_match_pyramid(fl, fr, H, W, L, sf, c["k_l"], c["o_l"], c["k_r"], c["o_r"], c["d_l"], c["d_r"], c["mb"], c["mbf"],
                                       capi.STEREO_SAD_LEVEL0)
        same(got, u_ref, z_ref, f"rfe_stereo_match_pyramid(fill={fill})")
    bufs = [up(ctx, fl, np.uint8), up(ctx, fr, np.uint8), up(ctx, c["k_l"], np.float32), up(ctx, c["o_l"], np.int32), up(ctx, c["k_r"], np.float32),
            up(ctx, c["o_r"], np.int32), up(ctx, c["d_l"], np.float32), up(ctx, c["d_r"], np.float32), ctx.alloc(max(N, 4) * 4), ctx.alloc(max(N, 4) * 4)]
    try:
        b = [x.ptr for x in bufs]
        ctx._chk(capi.lib.rfe_stereo_match_pyramid_dev(ctx.h, b[0], b[1], H, W, L, sf, b[2], b[3], N, b[4], b[5], Nr, b[6], b[7], c["mb"], c["mbf"],
                                                       capi.STEREO_SAD_LEVEL0, b[8], b[9]))
        ctx.synchronize()
        same((bufs[8].download((N,), np.float32), bufs[9].download((N,), np.float32)), u_ref, z_ref, "rfe_stereo_match_pyramid_dev")
    finally:
        for x in bufs:
            x.free()


# ---------------------------------------------------------------- descriptor helpers
def test_distinctive_index_equals_reference(ctx):
    z = RC.load("distinctive")
    desc, off = RC.dequantize(z["desc_q7"]), z["offsets"]
    best, med = ctx.distinctive_descriptors(desc, off)
    assert np.array_equal(best, z["ref_best"])
    assert int(np.diff(off).max()) == 512 and (med[np.diff(off) > 0] >= 0).all()


def test_distance_matrix_against_reference(ctx):
    z = RC.load("distance")
    a, b = np.ascontiguousarray(z["a"]), np.ascontiguousarray(z["b"])
    out = np.empty((37, 101), np.float32)
    ctx._chk(capi.lib.rfe_l2_distance_matrix(ctx.h, a.ctypes.data, 37, b.ctypes.data, 101, out.ctypes.data))
    check_distance(out, z["ref_dist"], "rfe_l2_distance_matrix")


def test_binarize_signed_zeros_and_denormals(ctx):
    z = RC.load("binarize")
    d = np.ascontiguousarray(z["desc"])
    bits = np.full(d.shape, 7, np.uint8)
    ctx._chk(capi.lib.rfe_binarize_descriptors(ctx.h, d.ctypes.data, d.shape[0], bits.ctypes.data))
    assert np.array_equal(bits, z["ref_bits"])
    dd, db = up(ctx, d, np.float32), ctx.alloc(d.size)
    try:
        ctx._chk(capi.lib.rfe_binarize_descriptors_dev(ctx.h, dd.ptr, d.shape[0], db.ptr))
        ctx.synchronize()
        assert np.array_equal(db.download(d.shape, np.uint8), z["ref_bits"])
    finally:
        dd.free(); db.free()


# ---------------------------------------------------------------- the documented bound, against the oracle
def test_distinctive_at_4096_and_8192_observations(ctx, oracle):
    """one map point of 4096 observations and one of 8192 (the bound rover_fe.h documents; the one-workgroup sort's whole LDS row) among
    small points, host and device form, bit for bit against rfo_distinctive_descriptors"""
    rng = np.random.default_rng(77)
    lens = np.array([3, 4096, 17, 0, 8192, 1, 40, 64, 65], np.int32)
    off = np.zeros(len(lens) + 1, np.int32); off[1:] = np.cumsum(lens)
    centers = rng.standard_normal((len(lens), 256)).astype(np.float32)
    desc = np.repeat(centers, lens, axis=0) + 0.3 * rng.standard_normal((off[-1], 256)).astype(np.float32)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(np.float32)
    desc[off[4] + 5000] = desc[off[4] + 17]                    # a duplicated observation inside the largest point
    rbest, rmed = oracle.distinctive_descriptors(desc, off)
    best, med = ctx.distinctive_descriptors(desc, off)
    assert np.array_equal(best, rbest) and RC.same_bits(med, rmed)
    assert rbest[3] == -1 and rbest[1] > 0 and rbest[4] > 0
    dd, do = up(ctx, desc, np.float32), up(ctx, off, np.int32)
    db, dm = ctx.alloc(len(lens) * 4), ctx.alloc(len(lens) * 4)
    try:
        ctx._chk(capi.lib.rfe_distinctive_descriptors_dev(ctx.h, dd.ptr, do.ptr, len(lens), int(off[-1]), 8192, db.ptr, dm.ptr))
        ctx.synchronize()
        assert np.array_equal(db.download((len(lens),), np.int32), rbest) and RC.same_bits(dm.download((len(lens),), np.float32), rmed)
        with pytest.raises(capi.RfeError):                     # one more than the bound is refused, not computed
            ctx._chk(capi.lib.rfe_distinctive_descriptors_dev(ctx.h, dd.ptr, do.ptr, len(lens), int(off[-1]), 8193, db.ptr, dm.ptr))
    finally:
        for x in (dd, do, db, dm):
            x.free()
