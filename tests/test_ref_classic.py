"""CPU: the checkers themselves held against Rover-SLAM's OWN C++ for the classic (model-free) stages.  tests/golden/ref_*.npz record
what the reference's function bodies compute (oracle/ref_classic cuts them out of a checkout and compiles them behind a stand-in for the
few OpenCV names; tools/gen_ref_golden.py records).  Here the numpy restatement (tests/stereo_pyramid_ref.py, tests/pyramid_ref.py), the
C oracle and the library's pure geometry function are compared with those recordings; tests/test_gpu_ref_classic.py does the HIP kernels.
Stereo outputs are compared as uint32 views.  The live tests re-run the harness when oracle/_ref/ exists (it needs the checkout).

Not reachable, so not in any fixture (profiles/ref_classic.md has the argument): a NaN or |deltaR| > 1 out of the parabola fit.  The first
STRICT minimum at an interior offset has d1 > d2 <= d3, so the denominator 2 * (d1 + d3 - 2 * d2) is positive and |deltaR| <= 0.5; a flat
patch (all SADs equal) puts that first minimum on the rim (-5) and is dropped there.  The census asserts both counts are zero."""
import ctypes as C
import time

import numpy as np
import pytest

import pyramid_ref as PR
import ref_classic_cases as RC
import stereo_pyramid_ref as SR
from oracle.ref_classic import client as R

f32 = np.float32
live = pytest.mark.skipif(not R.usable(), reason="oracle/_ref/ref_classic is not built, or its Rover-SLAM checkout is absent "
                                                 "(__graft_entry__.build() builds it when the checkout is there)")
# every branch family (b) is built for (issue list; the two unreachable ones are asserted to be zero instead, see the docstring)
B_BRANCHES = ("subpixel_left", "round_half", "band_edge_frac_y", "band_edge", "band_one_row_out", "descriptor_tie", "uR_eq_minU", "uR_eq_maxU",
              "best_in_1.3_1.4", "best_ge_1.4", "window_at_left_edge_kept", "window_at_right_edge_kept", "window_past_left_edge",
              "window_past_right_edge", "sad_best_at_minus5", "sad_best_at_plus5", "disparity_clamped", "disparity_just_under_maxD",
              "disparity_eq_maxD", "disparity_negative", "cut_removed", "cut_removed_eq_thDist")


def check_stereo_case(case, u_ref, z_ref, oracle, census=None):
    """restatement (and, at one level, the C oracle) == the reference's output, bit for bit; returns the census of the restatement"""
    cs = {} if census is None else census
    u, z = RC.restatement(case, cs)
    bad = np.nonzero(u.view(np.uint32) != u_ref.view(np.uint32))[0]
    assert RC.same_bits(u, u_ref) and RC.same_bits(z, z_ref), f"restatement differs from the reference at left keypoints {bad[:10].tolist()}"
    if case["nlevels"] == 1:
        uo, zo = oracle.stereo_match(case["img_l"], case["img_r"], case["k_l"], case["k_r"], case["d_l"], case["d_r"], case["mb"], case["mbf"])
        assert RC.same_bits(uo, u_ref) and RC.same_bits(zo, z_ref), "oracle.stereo_match differs from the reference"
    return cs


# ---------------------------------------------------------------- stereo fixtures
@pytest.mark.parametrize("name", RC.STEREO_FIXTURES)
def test_stereo_fixture(oracle, name):
    case, u_ref, z_ref, recorded = RC.load_stereo(name)
    kl, kr = RC.in_domain(case)
    assert kl.all() and kr.all()                               # every recorded keypoint is inside the domain: none is left out below
    assert len(u_ref) == len(case["k_l"])
    cs = check_stereo_case(case, u_ref, z_ref, oracle)
    assert cs == recorded, "the census changed: regenerate the fixtures (tools/gen_ref_golden.py)"
    assert cs["survivors"] == int((u_ref != -1).sum()) and cs["survivors"] >= 1
    assert cs["flat_patch_nan"] == 0 and cs["delta_outside_1"] == 0      # unreachable (module docstring)
    print(f"{name}: N={len(u_ref)} Nr={len(case['k_r'])} " + " ".join(f"{k}={v}" for k, v in cs.items() if v))


def test_stereo_fixtures_are_not_vacuous():
    cen = {n: RC.load_stereo(n)[3] for n in RC.STEREO_FIXTURES}
    for key in B_BRANCHES:
        assert cen["b_constructed"][key] >= 1, f"family (b) never takes {key}"
    names = RC.load_stereo("b_constructed")[0]["names"]
    assert "flat_patch" in names and "delta_half" in names
    for fam in "acd":
        mine = [c for n, c in cen.items() if n[0] == fam]
        assert sum(c["survivors"] for c in mine) > 10 and sum(c["cut_removed"] for c in mine) >= 1, fam
        assert any(c["survivors"] > 10 and c["cut_removed"] >= 1 for c in mine), fam
    for n in ("d_4lev_240x320", "d_8lev_480x752", "d_constructed"):
        assert len(cen[n]["survivor_octaves"]) >= 3, n
    d = cen["d_constructed"]
    assert d["octave_delta0"] and d["octave_delta1"] and d["octave_delta2_rejected"] >= 2 and d["band_right_octave_decides"] >= 1
    sizes = {n: (len(RC.load_stereo(n)[0]["k_l"]), len(RC.load_stereo(n)[0]["k_r"])) for n in ("c_4096", "c_1025_63", "c_1_63")}
    assert sizes == {"c_4096": (4096, 4096), "c_1025_63": (1025, 63), "c_1_63": (1, 63)}
    # the disparity clamp writes uL - 0.01 computed in DOUBLE (bestuR = uL-0.01); recorded value of the constructed keypoint
    case, u_ref, z_ref, _ = RC.load_stereo("b_constructed")
    i = case["names"].index("zero_disparity_clamp")
    assert u_ref[i] == f32(float(case["k_l"][i, 0]) - 0.01) and z_ref[i] == f32(case["mbf"]) / f32(0.01)


# ---------------------------------------------------------------- geometry, features per level
def test_geometry_and_features_per_level():
    from rover_slam_amd import capi
    import test_gpu_pyramid
    import test_gpu_stereo_pyramid
    z = RC.load("geometry")
    assert len(z["division_differs"]) >= 10 and int(z["n_division_differs_found"][0]) >= 10
    differing = 0
    for i, ((H, W, L), sf) in enumerate(zip(z["args"].tolist(), z["sf"].tolist())):
        rs, rinv, rw, rh, rfpl = (z[k][i, :L] for k in ("scale", "inv", "level_w", "level_h", "fpl"))
        for geo in (PR.geometry, SR.geometry):                 # the two numpy restatements
            lh, lw, s = geo(H, W, L, sf)
            assert np.array_equal(lh, rh) and np.array_equal(lw, rw) and RC.same_bits(s, rs), (H, W, L, sf)
        assert RC.same_bits((f32(1.0) / rs).astype(np.float32), rinv)
        h, w, s = np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.float32)
        rc = capi.lib.rfe_pyramid_geometry(H, W, L, C.c_float(sf), h.ctypes.data, w.ctypes.data, s.ctypes.data)
        assert (rc == 0) == bool(rh.min() > 0 and rw.min() > 0), (H, W, L, sf, rc)   # refused only for a level of zero pixels
        assert np.array_equal(h[:L], rh) and np.array_equal(w[:L], rw) and RC.same_bits(s[:L], rs), (H, W, L, sf)
        assert PR.features_per_level(1000, sf, L) == rfpl.tolist(), (L, sf)
        if i in z["division_differs"]:
            with np.errstate(all="ignore"):
                differing += int((np.rint(f32(W) / rs) != rw).any())
        if (L, round(sf, 4)) == (8, 1.2):
            assert rfpl.tolist() == test_gpu_pyramid.FPL_1000 == test_gpu_stereo_pyramid.FPL_1000
    assert differing == len(z["division_differs"])             # the recorded sizes really tell X * (1 / s) from X / s


# ---------------------------------------------------------------- descriptor helpers
def test_oracle_distinctive_index(oracle):
    z = RC.load("distinctive")
    desc, off = RC.dequantize(z["desc_q7"]), z["offsets"]
    lens = np.diff(off)
    assert {1, 2, 3, 4, 5, 64, 65, 130, 512} <= set(lens.tolist()) and 0 in lens
    best, _ = oracle.distinctive_descriptors(desc, off)
    assert np.array_equal(best, z["ref_best"])
    assert (z["ref_best"][lens == 0] == -1).all() and (z["ref_best"][lens > 0] >= 0).all()
    assert (z["ref_best"][lens > 2] > 0).any()                 # not every answer is index 0


def test_oracle_normalize_keypoints(oracle):
    z = RC.load("normkp")
    for h, w in ((300, 400), (480, 640), (376, 1241), (480, 752)):
        assert RC.same_bits(oracle.normalize_keypoints(z[f"k_{h}x{w}"], h, w), z[f"ref_{h}x{w}"]), (h, w)


def ulp_apart(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_distance(got, ref, what):
    """at most 1 ulp from the reference (the summation orders differ), the TH_LOW / TH_HIGH decisions identical"""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape and (got >= 0).all() and (ref >= 0).all()
    d = ulp_apart(got, ref)
    print(f"{what}: {int((d != 0).sum())} of {d.size} entries differ from the reference, at most {int(d.max())} ulp")
    assert d.max() <= 1
    for th in (f32(1.2), f32(1.4), (f32(1.4) + f32(1.2)) / f32(2)):
        assert np.array_equal(got < th, ref < th) and np.array_equal(got <= th, ref <= th)


def test_oracle_distance(oracle):
    z = RC.load("distance")
    a, b, ref = z["a"], z["b"], z["ref_dist"]
    assert ref.shape == (37, 101) and (ref < 1.2).sum() > 20 and (ref >= 1.4).sum() > 100 and ((ref >= 1.2) & (ref < 1.4)).sum() > 100
    got = np.stack([SR.desc_dist(a[i], b) for i in range(37)])
    check_distance(got, ref, "numpy desc_dist")
    # the C oracle's distance: best_dist of one-candidate lists, every b for every a
    _, bd, _ = oracle.search_candidates(np.repeat(a, 101, axis=0), b, np.arange(37 * 101 + 1, dtype=np.int32),
                                        np.tile(np.arange(101, dtype=np.int32), 37))
    assert bd.size == 37 * 101
    check_distance(bd.reshape(37, 101), ref, "oracle rfo_desc_dist")


def test_binarize_fixture_holds_the_edges():
    z = RC.load("binarize")
    d, bits = z["desc"], z["ref_bits"]
    assert np.array_equal(bits, (d > 0).astype(np.uint8))      # numpy compares denormals exactly
    neg0 = (d == 0) & np.signbit(d)
    den = (d != 0) & (np.abs(d) < np.finfo(np.float32).tiny)
    assert neg0.any() and ((d == 0) & ~np.signbit(d)).any() and (den & (d > 0)).any() and (den & (d < 0)).any()
    assert (bits[den & (d > 0)] == 1).all() and (bits[neg0] == 0).all()


# ---------------------------------------------------------------- live: the harness itself
@live
def test_live_harness_reproduces_every_recording():
    """fixtures cannot go stale: the compiled reference gives today what was recorded"""
    for name in RC.STEREO_FIXTURES:
        c, u_ref, z_ref, _ = RC.load_stereo(name)
        u, z = R.stereo(c["img_l"], c["img_r"], c["k_l"], c["o_l"], c["k_r"], c["o_r"], c["d_l"], c["d_r"], c["mb"], c["mbf"], c["nlevels"], c["scale_factor"])
        assert RC.same_bits(u, u_ref) and RC.same_bits(z, z_ref), name
    z = RC.load("geometry")
    for i, ((H, W, L), sf) in enumerate(zip(z["args"].tolist(), z["sf"].tolist())):
        g = R.geometry(H, W, L, sf, 1000)
        assert all(np.array_equal(g[k].view(np.uint32), z[k][i, :L].view(np.uint32)) for k in ("scale", "inv", "level_w", "level_h", "fpl")), (H, W, L, sf)
    z = RC.load("distinctive")
    assert np.array_equal(R.distinctive(RC.dequantize(z["desc_q7"]), z["offsets"]), z["ref_best"])
    z = RC.load("distance")
    assert RC.same_bits(R.distance(z["a"], z["b"]), z["ref_dist"])
    z = RC.load("normkp")
    for h, w in ((300, 400), (480, 640), (376, 1241), (480, 752)):
        assert RC.same_bits(R.normalize_keypoints(z[f"k_{h}x{w}"], h, w), z[f"ref_{h}x{w}"])
    z = RC.load("binarize")
    assert np.array_equal(R.binarize(z["desc"]), z["ref_bits"])


@live
def test_live_sweep(oracle):
    """fresh cases of families (a), (b) and (d), fixed seeds: reference == restatement (== oracle at one level), bit for bit"""
    from rover_slam_amd import weights as Wt
    wsp = Wt.make_superpoint(seed=7)
    t0 = time.time()
    cases = [("a", RC.extracted_case(oracle, wsp, 240, 320, 9 + 2 * s, seed=100 + s, kmax=400)) for s in range(6)]
    cases += [("b", RC.constructed_single(seed=200 + s, jitter=3)) for s in range(8)]
    cases += [("d", RC.extracted_case(oracle, wsp, 240, 320, 13 + 2 * s, seed=300 + s, nlevels=4, kmax=200)) for s in range(3)]
    cases += [("d", RC.constructed_pyramid(seed=400 + s)) for s in range(6)]
    for fam, c in cases:
        u, z = R.stereo(c["img_l"], c["img_r"], c["k_l"], c["o_l"], c["k_r"], c["o_r"], c["d_l"], c["d_r"], c["mb"], c["mbf"], c["nlevels"], c["scale_factor"])
        cs = check_stereo_case(c, u, z, oracle)
        assert cs["survivors"] >= 1
        print(f"sweep ({fam}): N={len(u)} survivors={cs['survivors']} cut={cs['cut_removed']} octaves={cs['survivor_octaves']}")
    print(f"sweep: {len(cases)} cases in {time.time() - t0:.1f} s")


@live
def test_live_extractor_fails_on_drift(tmp_path):
    """a checkout whose lines moved is refused, not compiled: the ranges must be the ones include/rover_fe.h cites"""
    import shutil
    from oracle.ref_classic import build_ref
    ref = tmp_path / "ref"
    for name, (fname, *_r) in build_ref._spec().items():
        dst = ref / fname
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(build_ref.ref_dir() + "/" + fname, dst)
    assert len(build_ref.extract(str(ref), str(tmp_path / "out"))) == 9          # the copy as it is: accepted
    frame = ref / "src" / "Frame.cc"
    frame.write_bytes(b"// one more line\n" + frame.read_bytes())
    with pytest.raises(build_ref.Drift, match="Frame.cc"):
        build_ref.extract(str(ref), str(tmp_path / "out2"))
