"""numpy restatement of the scale-pyramid contract of rfe_extract_pyramid_u8: level geometry, the 11-bit bilinear
resampling chain, SPextractor's per-level feature budget, and the per-level SuperPoint composition with the ExtractMultiLayers merge.
Test infrastructure only; `extract` composes oracle.superpoint per level."""
import numpy as np

MAX_LEVELS = 16


def geometry(H, W, nlevels, scale_factor):
    """(level_h, level_w, level_scale): s_0 = 1, s_l = float32(float64(s_{l-1}) * float64(sf)); W_l = rint(float32(W) * float32(1 / s_l))."""
    sf = np.float32(scale_factor)
    s = [np.float32(1.0)]
    for _ in range(1, nlevels):
        s.append(np.float32(np.float64(s[-1]) * np.float64(sf)))
    s = np.array(s, np.float32)
    inv = (np.float32(1.0) / s).astype(np.float32)
    lh = np.rint(np.float32(H) * inv).astype(np.int32)   # float32 product, round half to even (lrintf)
    lw = np.rint(np.float32(W) * inv).astype(np.int32)
    return lh, lw, s


def axis_coeffs(S, D):
    """source index i0 and 11-bit weight of i0 + 1 per destination index, as the contract states them (double, then float)"""
    scale = 1.0 / (np.float64(D) / np.float64(S))
    f = ((np.arange(D, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    i0 = fl.astype(np.int64)
    t = (f - fl).astype(np.float32)
    lo = i0 < 0
    i0[lo], t[lo] = 0, 0
    hi = i0 >= S - 1
    i0[hi], t[hi] = S - 1, 0
    w1 = np.rint(t * np.float32(2048)).astype(np.int64)
    return i0, w1


def resample(src, Hd, Wd):
    """one level from the level above: src [..., Hs, Ws] u8 -> [..., Hd, Wd] u8"""
    Hs, Ws = src.shape[-2:]
    x0, a1 = axis_coeffs(Ws, Wd)
    y0, b1 = axis_coeffs(Hs, Hd)
    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
    a0, b0 = 2048 - a1, 2048 - b1
    S = src.astype(np.int64)
    r0, r1 = S[..., y0, :], S[..., y1, :]
    t0 = a0 * r0[..., :, x0] + a1 * r0[..., :, x1]
    t1 = a0 * r1[..., :, x0] + a1 * r1[..., :, x1]
    v = (b0[:, None] * t0 + b1[:, None] * t1 + (1 << 21)) >> 22
    return v.astype(np.uint8)


def build(frames, nlevels, scale_factor):
    """level images of [B,H,W] (or [H,W]) u8 frames, chained as ComputePyramid does: a list of nlevels arrays, level 0 first"""
    img = np.asarray(frames, np.uint8)
    lh, lw, _ = geometry(img.shape[-2], img.shape[-1], nlevels, scale_factor)
    out = [img.copy()]
    for l in range(1, nlevels):
        out.append(resample(out[-1], int(lh[l]), int(lw[l])))
    return out


def features_per_level(nfeatures, scale_factor, nlevels):
    """SPextractor's constructor: mnFeaturesPerLevel (float arithmetic as in include/Extractors/SPextractor.h)"""
    factor = np.float32(1.0) / np.float32(scale_factor)
    den = np.float32(1.0) - np.float32(np.power(np.float64(factor), np.float64(nlevels)))
    n_desired = np.float32(np.float32(np.float32(nfeatures) * (np.float32(1.0) - factor)) / den)
    out, total = [], 0
    for _ in range(nlevels - 1):
        k = int(np.rint(n_desired))
        out.append(k)
        total += k
        n_desired = np.float32(n_desired * factor)
    out.append(max(nfeatures - total, 0))
    return out


def extract(oracle, weights, frames, nlevels, scale_factor, kmax, thr=0.0005, nms_radius=4, border=4, topk_always=False):
    """expected outputs of rfe_extract_pyramid_u8 on [B,H,W] frames: dict n, level_n, kpts, octave, score, desc (+ levels)"""
    img = np.asarray(frames, np.uint8)
    if img.ndim == 2:
        img = img[None]
    B = img.shape[0]
    km = [int(kmax)] * nlevels if np.isscalar(kmax) else [int(k) for k in kmax]
    K = sum(km)
    levels = build(img, nlevels, scale_factor)
    _, _, s = geometry(img.shape[1], img.shape[2], nlevels, scale_factor)
    out = {"n": np.zeros((B,), np.int32), "level_n": np.zeros((B, nlevels), np.int32), "kpts": np.zeros((B, K, 2), np.float32),
           "octave": np.zeros((B, K), np.int32), "score": np.zeros((B, K), np.float32), "desc": np.zeros((B, K, 256), np.float32),
           "levels": levels}
    for b in range(B):
        row = 0
        for l in range(nlevels):
            lv = levels[l][b]
            if km[l] == 0 or lv.shape[0] < 8 or lv.shape[1] < 8:
                continue
            r = oracle.superpoint(weights, np.ascontiguousarray(lv), kmax=km[l], thr=thr, nms_radius=nms_radius, border=border,
                                  topk_always=topk_always)
            n = int(r["n"])
            out["level_n"][b, l] = n
            out["kpts"][b, row:row + n] = r["kxy"][:n].astype(np.float32) * s[l]
            out["octave"][b, row:row + n] = l
            out["score"][b, row:row + n] = r["score"][:n]
            out["desc"][b, row:row + n] = r["desc"][:n]
            row += n
        out["n"][b] = row
    return out
