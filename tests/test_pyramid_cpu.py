"""CPU: the scale-pyramid contract -- known answers of the numpy restatement (tests/pyramid_ref.py), the library's
rfe_pyramid_geometry against it (a pure function: no device needed), its refusals, and the drop-in headers with the RFE_SP_PYRAMID opt-in."""
import os
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import pyramid_ref as P


def test_constant_image_stays_constant():
    for v in (0, 1, 77, 254, 255):
        img = np.full((2, 97, 131), v, np.uint8)
        for lv in P.build(img, 8, 1.2):
            assert (lv == v).all()


def test_scale_two_is_rounded_block_mean():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 64, 96)).astype(np.uint8)
    l1 = P.build(img, 2, 2.0)[1]
    want = (img.reshape(2, 32, 2, 48, 2).astype(np.int64).sum((2, 4)) + 2) >> 2
    assert np.array_equal(l1, want.astype(np.uint8))


def test_geometry_table_640x480():
    lh, lw, s = P.geometry(480, 640, 8, 1.2)
    assert list(zip(lh.tolist(), lw.tolist())) == [(480, 640), (400, 533), (333, 444), (278, 370), (231, 309), (193, 257), (161, 214), (134, 179)]
    assert np.allclose(s, [1, 1.2000000477, 1.4400000572, 1.7280001640, 2.0736002922, 2.4883203506, 2.9859845638, 3.5831816196], rtol=0, atol=1e-9)
    assert round(float((lh.astype(np.int64) * lw).sum()) / (480 * 640), 2) == 3.09
    assert P.features_per_level(1000, 1.2, 8) == [217, 181, 151, 126, 105, 87, 73, 60]


def test_library_geometry_matches_reference():
    from rover_slam_amd import capi
    for sf in (1.2, 1.25, 1.5, 2.0, 3.7):
        for L in range(1, 17):
            for v in range(8, 2001):
                H, W = v, 2008 - v
                lh, lw, s = P.geometry(H, W, L, sf)
                h = np.zeros((L,), np.int32); w = np.zeros((L,), np.int32); sc = np.zeros((L,), np.float32)
                rc = capi.lib.rfe_pyramid_geometry(H, W, L, np.float32(sf), h.ctypes.data, w.ctypes.data, sc.ctypes.data)
                assert rc == (0 if (lh.min() >= 1 and lw.min() >= 1) else -1), (H, W, L, sf)
                assert np.array_equal(h, lh) and np.array_equal(w, lw) and np.array_equal(sc, s), (H, W, L, sf)


def test_library_geometry_refusals():
    from rover_slam_amd import capi
    h = np.zeros((16,), np.int32); w = np.zeros((16,), np.int32); s = np.zeros((16,), np.float32)
    call = lambda H, W, L, sf, hp=h.ctypes.data: capi.lib.rfe_pyramid_geometry(H, W, L, sf, hp, w.ctypes.data, s.ctypes.data)  # noqa: E731
    assert call(480, 640, 8, 1.2) == 0
    for args in ((480, 640, 0, 1.2), (480, 640, 17, 1.2), (480, 640, 8, 1.0), (480, 640, 8, 0.5), (480, 640, 8, 4.5), (7, 640, 8, 1.2),
                 (480, 7, 8, 1.2), (16, 16, 16, 4.0)):
        assert call(*args) == -1, args
    assert call(480, 640, 1, 0.5) == 0          # one level: the scale factor plays no part
    assert call(480, 640, 8, 1.2, None) == -1
    with pytest.raises(capi.RfeError):
        capi.pyramid_geometry(480, 640, 8, 1.0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("macro", [None, "1"])
def test_shim_headers_build_with_pyramid_opt_in(tmp_path, macro):
    assert os.path.exists(DD.build(tmp_path, "pyramid_driver", ("RFE_SP_PYRAMID=" + macro,) if macro else ()))
