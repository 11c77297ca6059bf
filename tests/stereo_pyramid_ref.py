"""numpy restatement of the octave-aware stereo match, the checker of rfe_stereo_match_pyramid[_dev] and
rfe_stereo_frame_pyramid_dev.  Every fp32 product and sum is a separate rounding (explicit np.float32 casts); with one level it equals
oracle.stereo_match bit for bit (tests/test_stereo_pyramid_ref.py).  With SAD_LEVEL0 it is held, bit for bit, to what the reference's own
Frame::ComputeStereoMatches computes (tests/test_ref_classic.py on tests/golden/ref_*.npz)."""
import numpy as np

f32 = np.float32
SAD_LEVEL, SAD_LEVEL0 = 0, 1
TH_HIGH, TH_LOW = f32(1.4), f32(1.2)
_IDX = np.arange(64)
CENSUS_KEYS = ("candidates", "band_edge", "band_edge_frac_y", "band_one_row_out", "band_right_octave_decides", "octave_delta0", "octave_delta1",
               "octave_delta2_rejected", "uR_eq_minU", "uR_eq_maxU", "descriptor_tie", "best_in_1.3_1.4", "best_ge_1.4", "coarse_matches",
               "subpixel_left", "round_half", "window_at_left_edge_kept", "window_at_right_edge_kept", "window_past_left_edge",
               "window_past_right_edge", "sad_best_at_minus5", "sad_best_at_plus5", "flat_patch_nan", "delta_outside_1", "disparity_eq_maxD",
               "disparity_just_under_maxD", "disparity_negative", "disparity_clamped", "cut_removed", "cut_removed_eq_thDist", "survivors")


def geometry(H, W, nlevels, scale_factor):
    """(H_l, W_l, s_l) as rfe_pyramid_geometry: s_l = (float)((double)s_{l-1} * scale_factor), sizes lrintf(X * (1.0f / s_l))."""
    h, w, s = np.zeros(nlevels, np.int32), np.zeros(nlevels, np.int32), np.zeros(nlevels, np.float32)
    sc = f32(1.0)
    for l in range(nlevels):
        if l > 0:
            sc = f32(float(sc) * float(f32(scale_factor)))
        inv = f32(1.0) / sc
        s[l] = sc
        h[l] = int(np.rint(f32(f32(H) * inv)))
        w[l] = int(np.rint(f32(f32(W) * inv)))
    return h, w, s


def desc_dist(a, b):
    """DescriptorDistance_sp in the canonical order: a [256], b [C,256] -> [C] f32.  Float differences, double accumulation over a
    lane's 4 elements, then the xor butterfly 32..1 over the 64 lanes (lane 0's value)."""
    b = np.asarray(b, np.float32).reshape(-1, 256)
    d = (np.asarray(a, np.float32)[None, :] - b).astype(np.float32).reshape(-1, 64, 4).astype(np.float64)
    p = np.zeros(d.shape[:2], np.float64)
    for e in range(4):
        p = p + d[:, :, e] * d[:, :, e]
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, _IDX ^ off]
    return np.sqrt(p[:, 0]).astype(np.float32)


def roundf(x):
    """C roundf: half away from zero."""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def stereo_match(levels_l, levels_r, scale, k_l, oct_l, k_r, oct_r, d_l, d_r, mb, mbf, sad_source=SAD_LEVEL, census=None):
    """levels_*: list of [H_l,W_l] u8 arrays (level 0 first) of one view; scale: [L] f32 level scale factors; k_*: [N,2] f32 level-0
    pixels; oct_*: [N] i32; d_*: [N,256].  Returns (uRight [N], depth [N]).  A keypoint whose octave is outside [0, L) is handled as the
    device entry does: left -> no match, right -> never a candidate.
    census: an optional dict that receives how often each branch was taken (CENSUS_KEYS; tests/test_ref_classic.py uses it to show that a
    fixture reaches the branches it was built for).  It never changes the result."""
    cs = None
    if census is not None:
        cs = census
        for key in CENSUS_KEYS:
            cs.setdefault(key, 0)
        cs.setdefault("survivor_octaves", [])
        cs.setdefault("median_sad", -1)
    assert sad_source in (SAD_LEVEL, SAD_LEVEL0)
    scale = np.asarray(scale, np.float32)
    L = len(scale)
    kL = np.asarray(k_l, np.float32).reshape(-1, 2); kR = np.asarray(k_r, np.float32).reshape(-1, 2)
    oL = np.asarray(oct_l, np.int64).reshape(-1); oR = np.asarray(oct_r, np.int64).reshape(-1)
    dL = np.asarray(d_l, np.float32).reshape(-1, 256); dR = np.asarray(d_r, np.float32).reshape(-1, 256)
    N = len(kL)
    inv = (f32(1.0) / scale).astype(np.float32)
    u = np.full(N, -1, np.float32); z = np.full(N, -1, np.float32)
    th_orb = (TH_HIGH + TH_LOW) / f32(2)
    maxD = f32(mbf) / f32(mb)
    okR = (oR >= 0) & (oR < L)
    rR = (f32(2.0) * scale[np.where(okR, oR, 0)]).astype(np.float32)
    minr = np.floor((kR[:, 1] - rR).astype(np.float32)).astype(np.int64)
    maxr = np.ceil((kR[:, 1] + rR).astype(np.float32)).astype(np.int64)
    v = []
    for i in range(N):
        uL, vL = kL[i]
        l = int(oL[i])
        minU, maxU = f32(uL - maxD), uL
        if maxU < 0 or l < 0 or l >= L:
            continue
        row = int(vL)
        cand = np.nonzero(okR & (minr <= row) & (row <= maxr) & (oR >= l - 1) & (oR <= l + 1) & (kR[:, 0] >= minU) & (kR[:, 0] <= maxU))[0]
        best, bi = TH_HIGH, -1
        dist = []
        if len(cand):
            dist = desc_dist(dL[i], dR[cand])
            for j, d in zip(cand, dist):     # ascending iR, strict <
                if d < best:
                    best, bi = d, int(j)
        if cs is not None:
            inu = okR & (kR[:, 0] >= minU) & (kR[:, 0] <= maxU)
            inrow = (minr <= row) & (row <= maxr)
            gate = (oR >= l - 1) & (oR <= l + 1)
            cs["candidates"] += len(cand)
            cs["band_edge"] += int(((minr[cand] == row) | (maxr[cand] == row)).sum())
            cs["band_edge_frac_y"] += int((((minr[cand] == row) | (maxr[cand] == row)) & (kR[cand, 1] != np.floor(kR[cand, 1]))).sum())
            cs["band_one_row_out"] += int((inu & gate & ((minr == row + 1) | (maxr == row - 1))).sum())
            rl = f32(f32(2.0) * scale[l])      # the band the LEFT keypoint's octave would give: candidates only the right one admits
            cs["band_right_octave_decides"] += int(((np.floor((kR[cand, 1] - rl).astype(np.float32)) > row) | (np.ceil((kR[cand, 1] + rl).astype(np.float32)) < row)).sum())
            cs["octave_delta0"] += int((oR[cand] == l).sum())
            cs["octave_delta1"] += int((np.abs(oR[cand] - l) == 1).sum())
            cs["octave_delta2_rejected"] += int((inu & inrow & (np.abs(oR - l) == 2)).sum())
            cs["uR_eq_minU"] += int((kR[cand, 0] == minU).sum())
            cs["uR_eq_maxU"] += int((kR[cand, 0] == maxU).sum())
            if bi >= 0:
                cs["descriptor_tie"] += int((np.asarray(dist) == best).sum() > 1)
                cs["best_in_1.3_1.4"] += int(not (best < th_orb))
            elif len(cand):
                cs["best_ge_1.4"] += 1
        if not (best < th_orb) or bi < 0:
            continue
        sc = inv[l]
        su, sv, sr = roundf(f32(uL * sc)), roundf(f32(vL * sc)), roundf(f32(kR[bi, 0] * sc))
        li = 0 if sad_source == SAD_LEVEL0 else l
        IL, IR = levels_l[li], levels_r[li]
        Hs, Ws = IL.shape
        w = 5; Lh = 5
        if cs is not None:
            cs["coarse_matches"] += 1
            cs["subpixel_left"] += int(uL != np.floor(uL) or vL != np.floor(vL))
            cs["round_half"] += int(any(float(f32(c * sc)) % 1.0 == 0.5 for c in (uL, vL, kR[bi, 0])))
            cs["window_at_left_edge_kept"] += int(sr - Lh - w == 0)
            cs["window_at_right_edge_kept"] += int(sr + Lh + w + 1 == Ws - 1)
            cs["window_past_left_edge"] += int(sr - Lh - w == -1)
            cs["window_past_right_edge"] += int(sr + Lh + w + 1 == Ws)
        if sr - Lh - w < 0 or sr + Lh + w + 1 >= Ws:
            continue
        if sv - w < 0 or sv + w >= Hs or su - w < 0 or su + w >= Ws:
            continue
        pl = IL[sv - w:sv + w + 1, su - w:su + w + 1].astype(np.int32)
        vd = [f32(np.abs(pl - IR[sv - w:sv + w + 1, sr + inc - w:sr + inc + w + 1].astype(np.int32)).sum()) for inc in range(-Lh, Lh + 1)]
        bestinc = int(np.argmin(vd)) - Lh     # first strict minimum
        if cs is not None:
            cs["sad_best_at_minus5"] += int(bestinc == -Lh)
            cs["sad_best_at_plus5"] += int(bestinc == Lh)
        if bestinc in (-Lh, Lh):
            continue
        d1, d2, d3 = vd[Lh + bestinc - 1], vd[Lh + bestinc], vd[Lh + bestinc + 1]
        with np.errstate(all="ignore"):
            delta = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
        if cs is not None:
            cs["flat_patch_nan"] += int(np.isnan(delta))
            cs["delta_outside_1"] += int(delta < -1 or delta > 1)
        if delta < -1 or delta > 1 or np.isnan(delta):
            continue
        bestuR = f32(scale[l] * f32(f32(f32(sr) + f32(bestinc)) + delta))
        disp = f32(uL - bestuR)
        if cs is not None:
            cs["disparity_eq_maxD"] += int(disp == maxD)
            cs["disparity_just_under_maxD"] += int(disp < maxD and float(maxD) - float(disp) <= 0.05)
            cs["disparity_negative"] += int(disp < 0)
            cs["disparity_clamped"] += int(disp == 0)
        if disp >= 0 and disp < maxD:
            if disp <= 0:
                disp = f32(0.01); bestuR = f32(uL - f32(0.01))
            z[i] = f32(mbf) / disp; u[i] = bestuR
            v.append((int(vd[Lh + bestinc]), i))
    if v:
        v.sort()
        med = f32(v[len(v) // 2][0]); th = f32(f32(1.5) * f32(1.4)) * med
        for d, i in v:
            if not (f32(d) < th):
                u[i] = -1; z[i] = -1
                if cs is not None:
                    cs["cut_removed"] += 1
                    cs["cut_removed_eq_thDist"] += int(f32(d) == th)
            elif cs is not None:
                cs["survivors"] += 1
                cs["survivor_octaves"].append(int(oL[i]))
        if cs is not None:
            cs["median_sad"] = int(v[len(v) // 2][0])
            cs["survivor_octaves"] = sorted(set(cs["survivor_octaves"]))
    return u, z
