"""Input cases for the checks against the reference's own C++ (oracle/ref_classic): builders shared by tools/gen_ref_golden.py (which
records them with the reference's outputs under tests/golden/ref_*.npz) and by the live sweep of tests/test_ref_classic.py (which draws
fresh ones).  CPU only.  Every builder returns inputs INSIDE the reference's defined behaviour (in_domain below)."""
import glob
import io
import os

import numpy as np

import pyramid_ref as PR
import stereo_pyramid_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32
MAX_PART = 1000000          # bytes per committed fixture file


# ---------------------------------------------------------------- exact compact descriptors
def quantize(desc, bits=7):
    """int8 codes c with value c * 2**-bits (exact in fp32)"""
    return np.clip(np.rint(np.asarray(desc, np.float64) * 2.0 ** bits), -127, 127).astype(np.int8)


def dequantize(codes, bits=7):
    return (codes.astype(np.float32) * f32(2.0 ** -bits)).astype(np.float32)


# ---------------------------------------------------------------- the reference's defined behaviour
def _roundf(x):
    x = np.asarray(x, np.float32).astype(np.float64)
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5)).astype(np.int64)


def in_domain(case):
    """(keep_left [N], keep_right [Nr]): the left 11x11 patch (at level-scaled coordinates, read from level 0 as the reference does) lies
    inside the level-0 image and the keypoint's row indexes vRowIndices; the right keypoint's row band lies inside [0, H).  Outside this,
    cv::Mat::rowRange throws / vRowIndices is indexed out of range, and the reference has no defined result."""
    H, W = case["img_l"].shape
    _, _, s = SR.geometry(H, W, case["nlevels"], case["scale_factor"])
    inv = (f32(1.0) / s).astype(np.float32)
    kl, kr = case["k_l"], case["k_r"]
    su, sv = _roundf(kl[:, 0] * inv[case["o_l"]]), _roundf(kl[:, 1] * inv[case["o_l"]])
    keep_l = (su - 5 >= 0) & (su + 5 < W) & (sv - 5 >= 0) & (sv + 5 < H) & (kl[:, 1] >= 0) & (kl[:, 1] < H) & (kl[:, 0] >= 0)
    r = (f32(2.0) * s[case["o_r"]]).astype(np.float32)
    keep_r = (np.floor((kr[:, 1] - r).astype(np.float32)) >= 0) & (np.ceil((kr[:, 1] + r).astype(np.float32)) <= H - 1)
    return keep_l, keep_r


def restrict(case):
    """drop the keypoints outside the domain (an input filter: every keypoint that remains is compared)"""
    kl, kr = in_domain(case)
    out = dict(case)
    for k in ("k_l", "o_l", "d_l"):
        out[k] = np.ascontiguousarray(case[k][kl])
    for k in ("k_r", "o_r", "d_r"):
        out[k] = np.ascontiguousarray(case[k][kr])
    return out


def levels_of(case, fill=None):
    """level images for the restatement / the library: level 0 is the image; levels >= 1 are never read with SAD_LEVEL0, so they are either
    the resampled pyramid (fill None) or a constant"""
    H, W = case["img_l"].shape
    L = case["nlevels"]
    if fill is None:
        return PR.build(case["img_l"], L, case["scale_factor"]), PR.build(case["img_r"], L, case["scale_factor"])
    lh, lw, _ = SR.geometry(H, W, L, case["scale_factor"])
    rest = [np.full((int(lh[l]), int(lw[l])), fill, np.uint8) for l in range(1, L)]
    return [case["img_l"]] + rest, [case["img_r"]] + rest


def restatement(case, census=None, fill=77):
    H, W = case["img_l"].shape
    _, _, s = SR.geometry(H, W, case["nlevels"], case["scale_factor"])
    ll, lr = levels_of(case, fill)
    return SR.stereo_match(ll, lr, s, case["k_l"], case["o_l"], case["k_r"], case["o_r"], case["d_l"], case["d_r"], case["mb"], case["mbf"],
                           SR.SAD_LEVEL0, census=census)


def make_case(img_l, img_r, k_l, o_l, k_r, o_r, d_l, d_r, mb, mbf, nlevels=1, scale_factor=1.2):
    return dict(img_l=np.ascontiguousarray(img_l, np.uint8), img_r=np.ascontiguousarray(img_r, np.uint8),
                k_l=np.ascontiguousarray(k_l, np.float32).reshape(-1, 2), o_l=np.ascontiguousarray(o_l, np.int32).reshape(-1),
                k_r=np.ascontiguousarray(k_r, np.float32).reshape(-1, 2), o_r=np.ascontiguousarray(o_r, np.int32).reshape(-1),
                d_l=np.ascontiguousarray(d_l, np.float32).reshape(-1, 256), d_r=np.ascontiguousarray(d_r, np.float32).reshape(-1, 256),
                mb=float(f32(mb)), mbf=float(f32(mbf)), nlevels=int(nlevels), scale_factor=float(f32(scale_factor)))


# ---------------------------------------------------------------- family (a) / (c) / (d): extracted keypoints
def shifted_pair(H, W, disp, seed, noise=8):
    """tests/test_stereo.py: one textured scene, pure horizontal shift, independent sensor noise per view"""
    from rover_slam_amd import synth
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(rng, H, W + disp, margin=0)
    left = np.clip(scene[:, :W] + rng.integers(0, noise, (H, W)), 0, 255).astype(np.uint8)
    right = np.clip(scene[:, disp:disp + W] + rng.integers(0, noise, (H, W)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def extracted_case(oracle, wsp, H, W, disp, seed, nlevels=1, kmax=400, thr=0.0005, mb=0.11, mbf=0.11 * 435.0, topk_always=False):
    """keypoints and descriptors of the CPU oracle (per level through tests/pyramid_ref.py), descriptors rounded to int8 codes * 2**-7"""
    left, right = shifted_pair(H, W, disp, seed)
    ex = PR.extract(oracle, wsp, np.stack([left, right]), nlevels, 1.2, kmax, thr=thr, topk_always=topk_always)
    nl, nr = int(ex["n"][0]), int(ex["n"][1])
    c = make_case(left, right, ex["kpts"][0, :nl], ex["octave"][0, :nl], ex["kpts"][1, :nr], ex["octave"][1, :nr],
                  dequantize(quantize(ex["desc"][0, :nl])), dequantize(quantize(ex["desc"][1, :nr])), mb, mbf, nlevels, 1.2)
    return restrict(c)


# ---------------------------------------------------------------- family (b): constructed, single level
def _unit_pair(slot, dist):
    """two unit vectors at L2 distance `dist` in the plane of axes (2*slot, 2*slot+1): different slots are orthogonal (distance sqrt 2 > 1.4)"""
    a, b = np.zeros(256, np.float64), np.zeros(256, np.float64)
    th = 2.0 * np.arcsin(dist / 2.0)
    a[2 * slot] = 1.0
    b[2 * slot], b[2 * slot + 1] = np.cos(th), np.sin(th)
    return a.astype(np.float32), b.astype(np.float32)


class _Builder:
    """left / right images of independent noise, into which each slot writes one 11-row texture: the left 11x11 patch around (su, sv) is
    a copy of the right texture around (sr_true, sv) plus a perturbation whose absolute sum is EXACTLY `sad` -- so the SAD search finds
    its minimum `sad` at the window centred on sr_true, and every SAD is an exact, chosen integer."""

    def __init__(self, H, W, seed):
        self.rng = np.random.default_rng(seed)
        self.H, self.W = H, W
        self.L = self.rng.integers(0, 256, (H, W)).astype(np.uint8)
        self.R = self.rng.integers(0, 256, (H, W)).astype(np.uint8)
        self.kl, self.kr, self.dl, self.dr, self.ol, self.orr, self.names = [], [], [], [], [], [], []
        self.slot = 0

    def texture(self, su, sv, sr_true, sad, kind="random"):
        """kind: random | symmetric (mirror-symmetric about sr_true: d1 == d3, delta == 0 exactly) | flat"""
        lo, hi = max(sr_true - 16, 0), min(sr_true + 16, self.W - 1)
        t = np.arange(lo, hi + 1) - sr_true
        if kind == "random":
            T = self.rng.integers(40, 216, (11, hi - lo + 1))
        elif kind == "symmetric":
            assert lo == sr_true - 16 and hi == sr_true + 16
            half = self.rng.integers(40, 216, (11, 17))
            T = half[:, np.abs(t)]
        else:
            T = np.full((11, hi - lo + 1), 128)
        self.R[sv - 5:sv + 6, lo:hi + 1] = T
        patch = T[:, (sr_true - 5 - lo):(sr_true + 6 - lo)].copy()
        assert patch.shape == (11, 11), "the true window must lie inside the right image"
        add = np.full(121, sad // 121)
        add[:sad % 121] += 1
        assert add.max() <= 39
        if kind == "symmetric":
            assert sad == 0
        self.L[sv - 5:sv + 6, su - 5:su + 6] = patch + add.reshape(11, 11)

    def left(self, x, y, desc, name, octave=0):
        self.kl.append((x, y)); self.dl.append(desc); self.ol.append(octave); self.names.append(name)
        return len(self.kl) - 1

    def right(self, x, y, desc, octave=0):
        self.kr.append((x, y)); self.dr.append(desc); self.orr.append(octave)
        return len(self.kr) - 1

    def pair(self, name, uL, vL, uR, vR, sad, dist=0.3, inc=0, kind="random", su=None, sv=None, sr=None, octL=0, octR=0, place=True):
        """one left keypoint, one right keypoint carrying the matching descriptor; the texture is placed so that the SAD minimum sits `inc`
        pixels from round(uR) (su / sv / sr: the integer coordinates the reference will compute, given when they are not round(level 0))"""
        a, b = _unit_pair(self.slot, dist)
        self.slot += 1
        su = int(SR.roundf(f32(uL))) if su is None else su
        sv = int(SR.roundf(f32(vL))) if sv is None else sv
        sr = int(SR.roundf(f32(uR))) if sr is None else sr
        if place:
            self.texture(su, sv, sr + inc, sad, kind)
        self.left(uL, vL, a, name, octL)
        self.right(uR, vR, b, octR)
        return a, b

    def case(self, mb, mbf, nlevels=1, scale_factor=1.2):
        c = make_case(self.L, self.R, self.kl, self.ol, self.kr, self.orr, np.stack(self.dl), np.stack(self.dr), mb, mbf, nlevels, scale_factor)
        c["names"] = list(self.names)
        return c


def constructed_single(seed=0, jitter=0):
    """family (b): one keypoint (or more) per edge of Frame::ComputeStereoMatches, H x W = 528 x 320, maxD = mbf / mb = 40 exactly.
    Slots sit 12 rows apart (row bands reach 3 rows at most) and carry mutually orthogonal descriptors, so they do not interact.
    `jitter` moves the plain slots' columns for the live sweep."""
    H, W, D = 528, 320, 20
    b = _Builder(H, W, seed)
    rows = iter(range(12, H - 8, 12))
    j = lambda: int(b.rng.integers(0, jitter + 1))     # noqa: E731
    sads = iter(range(1000, 2000, 10))
    # plain matches below the median.  With the three SAD-0 slots at the end, 15 matches lie below 1000 and 15 at or above it: the sorted
    # list has an EVEN length 30, element 15 (= size / 2) is 1000 and element 14 is 990: thDist = 1.5f * 1.4f * 1000 = 2100 exactly in fp32.
    for k, sad in enumerate((300, 400, 500, 600, 700, 800, 850, 900, 950, 970, 980, 990)):
        y = next(rows)
        x = 60 + 16 * k + j()
        b.pair(f"plain{k}", x, y, x - D, y, sad, dist=0.2 + 0.09 * k, inc=(k % 7) - 3)
    y = next(rows); b.pair("plain_hi0", 90, y, 90 - D, y, 1200, inc=2)
    y = next(rows); b.pair("plain_hi1", 110, y, 110 - D, y, 1400, inc=-2)
    y = next(rows); b.pair("cut_kept_2099", 200, y, 200 - D, y, 2099)
    y = next(rows); b.pair("cut_equal_thDist_2100", 210, y, 210 - D, y, 2100)
    y = next(rows); b.pair("cut_removed_3000", 220, y, 220 - D, y, 3000)
    # sub-pixel coordinates; .5 halves round AWAY from zero (where the integer part is even, half-to-even would differ), in u, v and uR
    y = next(rows); b.pair("subpixel", 100.25, y + 0.75, 80.3, y + 0.2, next(sads))
    y = next(rows); b.pair("half_u", 120.5, y, 100, y, next(sads))
    y = next(rows); b.pair("half_v_even", 130, y + 0.5, 110, y, next(sads))            # rows are multiples of 12: even
    y = next(rows); b.pair("half_uR_odd", 150, y, 130.5, y, next(sads), inc=4)         # sr = 131; half-to-even gives 130, the minimum at +5: dropped
    # row band of the right keypoint: floor(y - 2) .. ceil(y + 2)
    y = next(rows); b.pair("band_frac_top", 160, y + 3, 140, y + 0.3, next(sads))      # maxr = ceil(y + 2.3) = y + 3: inside
    next(rows)                                                                          # (that texture sits 3 rows low: leave a gap)
    y = next(rows); b.pair("band_frac_bottom_out", 164, y - 3, 144, y + 0.3, next(sads))   # minr = floor(y - 1.7) = y - 2: row y - 3 is out
    y = next(rows); b.pair("band_2_rows_off", 170, y, 150, y + 2, next(sads))
    y = next(rows); b.pair("band_3_rows_off", 174, y, 154, y + 3, next(sads))
    # duplicated right descriptor: the LOWEST iR wins (the first one sits at the true place, the second 15 px to the left)
    y = next(rows)
    _, dup = b.pair("duplicate_desc", 180, y, 160, y, next(sads))
    b.right(145, y, dup)
    # descriptor distance thresholds: accepted below (1.4f + 1.2f) / 2; a candidate at or above 1.4 is never the best
    y = next(rows); b.pair("dist_1.29", 190, y, 170, y, next(sads), dist=1.29)
    y = next(rows); b.pair("dist_1.35", 194, y, 174, y, next(sads), dist=1.35)
    y = next(rows); b.pair("dist_1.41", 198, y, 178, y, next(sads), dist=1.41)
    # SAD window against the image sides: iniu = sr - 10 < 0 and endu = sr + 11 >= W drop the keypoint
    y = next(rows); b.pair("window_left_kept", 10 + 12, y, 10, y, next(sads))
    y = next(rows); b.pair("window_left_dropped", 9 + 12, y, 9, y, 0, place=False)
    y = next(rows); b.pair("window_right_kept", W - 12 + 4, y, W - 12, y, next(sads))
    y = next(rows); b.pair("window_right_dropped", W - 11 + 4, y, W - 11, y, 0, place=False)
    # best SAD on the rim of the +-5 search: dropped
    y = next(rows); b.pair("sad_at_minus5", 230, y, 210, y, next(sads), inc=-5)
    y = next(rows); b.pair("sad_at_plus5", 234, y, 214, y, next(sads), inc=5)
    # a flat patch: all eleven SADs are 0, the first strict minimum is the rim (-5): dropped there.  (0/0 in the parabola needs
    # d1 == d2 == d3 while the first strict minimum needs d1 > d2: it cannot be reached; for the same reason |deltaR| <= 0.5 always.)
    y = next(rows); b.pair("flat_patch", 240, y, 220, y, 0, kind="flat")
    # the largest |deltaR| there is: d3 == d2 < d1 gives +0.5.  Left patch and the windows at inc 0 and +1 are flat, the rest is not.
    y = next(rows)
    b.pair("delta_half", 244, y, 224, y, 0, kind="flat")
    b.R[y - 5:y + 6, 224 - 16:224 - 5] = b.rng.integers(40, 120, (11, 11))
    b.R[y - 5:y + 6, 224 + 7:224 + 17] = b.rng.integers(140, 216, (11, 10))
    # symmetric texture: delta == 0 exactly, so the disparity is an exact, chosen number
    y = next(rows); b.pair("zero_disparity_clamp", 250, y, 250, y, 0, kind="symmetric")            # uR == maxU; 0 -> 0.01
    y = next(rows); b.pair("disparity_at_maxD", 260, y, 220, y, 0, kind="symmetric")                # uR == minU; 40 is not < 40
    y = next(rows); b.pair("disparity_under_maxD", f32(270) - f32(0.01), y, 230, y, 0, kind="symmetric", su=270)
    y = next(rows); b.pair("negative_disparity", f32(280) - f32(0.25), y, f32(280) - f32(0.25), y, 0, kind="symmetric", su=280, sr=280)
    c = b.case(0.5, 20.0)
    assert all(in_domain(c)[0]) and all(in_domain(c)[1]), "family (b) is built inside the domain"
    return c


def constructed_pyramid(seed=1):
    """family (d), constructed: 4 levels, 240 x 320, scale 1.2; the patches come from LEVEL 0 at level-scaled coordinates.
    Octave gate: left octave 1 against right octaves 1, 2 (taken) and 3 (two away: not a candidate), left octave 2 against right octave 0.
    Row band: a pair that matches only because the RIGHT keypoint's octave sets the band, and one that would match only if the left one's did."""
    H, W, L, D = 240, 320, 4, 24
    _, _, s = SR.geometry(H, W, L, 1.2)
    inv = (f32(1.0) / s).astype(np.float32)
    b = _Builder(H, W, seed)
    specs = [(f"plain{k}_o{oL}{oR}", oL, oR, 500 + 100 * k, (k % 5) - 2, None)
             for k, (oL, oR) in enumerate(((0, 0), (1, 1), (2, 2), (3, 3), (0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0), (2, 3), (3, 2)))]
    specs += [("gate_delta0", 1, 1, 620, 0, None), ("gate_delta1", 1, 2, 640, 0, None), ("gate_delta2_up", 1, 3, 660, 0, None),
              ("gate_delta2_down", 2, 0, 680, 0, None),
              # right octave 1: r = 2.4.  y_R = row - 3.1: maxr = ceil(row - 0.7) = row, inside; the left octave's r = 2 would give row - 1
              ("band_right_octave_admits", 0, 1, 700, 0, -3.1),
              # right octave 0: r = 2: maxr = ceil(row - 1.1) = row - 1, outside; the LEFT octave's r = 2.4 would admit it
              ("band_left_octave_would_admit", 1, 0, 720, 0, -3.1),
              ("cut_removed", 0, 0, 3500, 0, None)]
    specs.sort(key=lambda t: -t[1])          # texture rows are LEVEL rows: the high octaves take the low ones, so that v * s stays inside H
    for k, (name, oL, oR, sad, inc, yr_off) in enumerate(specs):
        uL, vL = f32(f32(70 + 4 * k) * s[oL]), f32(f32(12 + 12 * k) * s[oL])
        uR = f32(uL - f32(D))
        su, sv, sr = (int(SR.roundf(f32(v * inv[oL]))) for v in (uL, vL, uR))      # where the reference reads, in the level-0 image
        vR = vL if yr_off is None else f32(int(vL) + yr_off)
        b.pair(name, uL, vL, uR, vR, sad, inc=inc, su=su, sv=sv, sr=sr, octL=oL, octR=oR)
    c = b.case(0.11, 0.11 * 435.0, L, 1.2)
    assert all(in_domain(c)[0]) and all(in_domain(c)[1]), "family (d) constructed is built inside the domain"
    return c


# ---------------------------------------------------------------- fixtures on disk
def save(name, arrays):
    """tests/golden/ref_<name>.npz, split into ref_<name>.partK.npz when one file would pass MAX_PART bytes"""
    for old in glob.glob(os.path.join(GOLDEN, f"ref_{name}.npz")) + glob.glob(os.path.join(GOLDEN, f"ref_{name}.part*.npz")):
        os.remove(old)
    path = os.path.join(GOLDEN, f"ref_{name}.npz")
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) <= MAX_PART:
        return [path]
    os.remove(path)

    def packed(a):
        buf = io.BytesIO()
        np.savez_compressed(buf, a=a)
        return buf.getbuffer().nbytes

    items = []                                         # (key, array, compressed bytes); an array too large for one file is split by rows
    for key, a in arrays.items():
        a = np.asarray(a)
        pieces = 1
        while True:
            parts = np.array_split(a, pieces, axis=0) if pieces > 1 else [a]
            sizes = [packed(x) for x in parts]
            if max(sizes) <= MAX_PART - 4096:
                break
            pieces += 1
        items += [(key if pieces == 1 else f"{key}@{i}", x, n) for i, (x, n) in enumerate(zip(parts, sizes))]
    bins = []                                          # first fit, in order
    for key, a, n in items:
        for b in bins:
            if b[0] + n + 512 <= MAX_PART - 4096:
                b[0] += n + 512; b[1][key] = a
                break
        else:
            bins.append([n + 512, {key: a}])
    paths = []
    for k, (_, part) in enumerate(bins):
        p = os.path.join(GOLDEN, f"ref_{name}.part{k}.npz")
        np.savez_compressed(p, **part)
        assert os.path.getsize(p) <= MAX_PART, (p, os.path.getsize(p))
        paths.append(p)
    return paths


def load(name):
    files = sorted(glob.glob(os.path.join(GOLDEN, f"ref_{name}.npz")) + glob.glob(os.path.join(GOLDEN, f"ref_{name}.part*.npz")))
    if not files:
        raise FileNotFoundError(f"tests/golden/ref_{name}*.npz (python tools/gen_ref_golden.py)")
    raw = {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            for k in z.files:
                raw[k] = z[k]
    out = {}
    for k in sorted(raw, key=lambda k: (k.split("@")[0], int(k.split("@")[1]) if "@" in k else 0)):
        base = k.split("@")[0]
        out[base] = raw[k] if base not in out else np.concatenate([out[base], raw[k]], axis=0)
    return out


def pack_case(case):
    """arrays of one stereo case; descriptors as int8 codes when that is exact"""
    out = {k: case[k] for k in ("img_l", "img_r", "k_l", "o_l", "k_r", "o_r")}
    for k in ("d_l", "d_r"):
        q = quantize(case[k])
        if np.array_equal(dequantize(q).view(np.uint32), case[k].view(np.uint32)):
            out[k + "_q7"] = q
        else:
            out[k] = case[k]
    out["params"] = np.array([case["mb"], case["mbf"], case["scale_factor"]], np.float32)
    out["nlevels"] = np.array([case["nlevels"]], np.int32)
    if "names" in case:
        out["names"] = np.array(case["names"])
    return out


def unpack_case(z):
    c = {k: z[k] for k in ("img_l", "img_r", "k_l", "o_l", "k_r", "o_r")}
    for k in ("d_l", "d_r"):
        c[k] = dequantize(z[k + "_q7"]) if k + "_q7" in z else z[k]
    c["mb"], c["mbf"], c["scale_factor"] = (float(v) for v in z["params"])
    c["nlevels"] = int(z["nlevels"][0])
    if "names" in z:
        c["names"] = [str(s) for s in z["names"]]
    return c


def subset(case, idx_l, idx_r):
    out = dict(case)
    for k in ("k_l", "o_l", "d_l"):
        out[k] = np.ascontiguousarray(case[k][idx_l])
    for k in ("k_r", "o_r", "d_r"):
        out[k] = np.ascontiguousarray(case[k][idx_r])
    out.pop("names", None)
    return out


STEREO_FIXTURES = ("a_240x320", "b_constructed", "c_4096", "c_1025_63", "c_1_63", "d_4lev_240x320", "d_8lev_480x752", "d_constructed")


def load_stereo(name):
    """(case, recorded mvuRight, recorded mvDepth, recorded census dict) of one stereo fixture; the N = 1025 / N = 1 capacity cases are
    index subsets of c_4096"""
    z = load(name)
    if "idx_l" in z:
        case = subset(unpack_case(load("c_4096")), z["idx_l"], z["idx_r"])
    else:
        case = unpack_case(z)
    census = {str(k): int(v) for k, v in zip(z["census_keys"], z["census_vals"])}
    census["survivor_octaves"] = [int(o) for o in z["census_octaves"]]
    return case, z["ref_u"], z["ref_z"], census


def same_bits(a, b):
    """equal as uint32 views: neither -1 nor a NaN can hide a difference"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
