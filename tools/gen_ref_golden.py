#!/usr/bin/env python3
"""Record what the reference's own C++ computes (oracle/_ref/ref_classic, built by oracle/ref_classic/build_ref.py from a Rover-SLAM
checkout) as fixtures tests/golden/ref_*.npz: inputs, the reference's outputs, and the branch census of each stereo case.
Fixed seeds, CPU only.  Keypoints and descriptors come from the CPU oracle (pyramid levels through tests/pyramid_ref.py); descriptors of
extracted cases are rounded to int8 codes * 2**-7 BEFORE the reference sees them, so the stored codes are the exact inputs.

Place recognition (--only bow): tests/golden/ref_bow_*.npz from oracle/_ref/ref_bow, DBoW3's and KeyFrameDatabase's own bodies; inputs
from tests/ref_bow_cases.py.  --check records into a temporary directory instead and compares the bytes with the committed files.

    python tools/gen_ref_golden.py [--report profiles/ref_classic_census.md] [--only bow] [--check]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyramid_ref as PR                      # noqa: E402
import bow_ref as BR                          # noqa: E402
import ref_bow_cases as BC                    # noqa: E402
import ref_classic_cases as RC                # noqa: E402
import stereo_pyramid_ref as SR               # noqa: E402
from oracle import oracle as O                # noqa: E402
from oracle.ref_classic import client as R    # noqa: E402
from rover_slam_amd import weights as Wt      # noqa: E402

f32 = np.float32
GEO_SIZES = ((480, 640), (480, 752), (376, 1241), (240, 320))       # (H, W)
GEO_LEVELS = (1, 4, 8, 16)
GEO_SCALES = (1.2, 1.5, 2.0, 1.1)
NORMKP_SIZES = ((300, 400), (480, 640), (376, 1241), (480, 752))
DISTINCTIVE_COUNTS = (1, 2, 3, 4, 5, 64, 65, 130, 512)


def ref_stereo(c, sanitized):
    return R.stereo(c["img_l"], c["img_r"], c["k_l"], c["o_l"], c["k_r"], c["o_r"], c["d_l"], c["d_r"], c["mb"], c["mbf"],
                    c["nlevels"], c["scale_factor"], sanitized=sanitized)


def record_stereo(name, c, sanitized, report, extra=None):
    """the reference's outputs + the census of the restatement, which must first equal the reference on this very case"""
    u, z = ref_stereo(c, sanitized)
    census = {}
    ur, zr = RC.restatement(c, census)
    same = np.array_equal(u.view(np.uint32), ur.view(np.uint32)) and np.array_equal(z.view(np.uint32), zr.view(np.uint32))
    assert census["survivors"] >= 1, f"{name}: no match survives -- outside the domain (vDistIdx[size/2] undefined)"
    arrays = RC.pack_case(c) if extra is None else dict(extra)
    arrays["ref_u"], arrays["ref_z"] = u, z
    keys = [k for k in SR.CENSUS_KEYS] + ["median_sad"]
    arrays["census_keys"] = np.array(keys)
    arrays["census_vals"] = np.array([census[k] for k in keys], np.int64)
    arrays["census_octaves"] = np.array(census["survivor_octaves"], np.int32)
    files = RC.save(name, arrays)
    size = sum(os.path.getsize(f) for f in files)
    report.append((name, len(c["k_l"]), len(c["k_r"]), same, census, size, len(files)))
    print(f"{name}: N={len(c['k_l'])} Nr={len(c['k_r'])} survivors={census['survivors']} cut={census['cut_removed']} "
          f"octaves={census['survivor_octaves']} restatement==reference: {same}  ({size} bytes in {len(files)} file(s))")
    return u, z


def gen_stereo(sanitized, report):
    wsp = Wt.make_superpoint(seed=7)
    record_stereo("a_240x320", RC.extracted_case(O, wsp, 240, 320, 17, seed=3, kmax=400), sanitized, report)
    record_stereo("b_constructed", RC.constructed_single(), sanitized, report)
    # (c) capacity: 480 x 752, N = Nr = 4096; N = 1025 with Nr = 63 and N = 1 are index subsets of it
    big = RC.extracted_case(O, wsp, 480, 752, 13, seed=13, kmax=4800, thr=0.0, topk_always=True)
    assert len(big["k_l"]) >= 4096 and len(big["k_r"]) >= 4096, (len(big["k_l"]), len(big["k_r"]))
    big = RC.subset(big, np.arange(4096), np.arange(4096))
    u, _ = record_stereo("c_4096", big, sanitized, report)
    left = np.arange(1025)
    hit = [i for i in left if u[i] >= 0]
    partner = []
    for i in hit:                                  # the right keypoint each surviving match landed on
        j = int(np.argmin(np.abs(big["k_r"][:, 0] - u[i]) + 4 * np.abs(big["k_r"][:, 1] - big["k_l"][i, 1])))
        if j not in partner:
            partner.append(j)
        if len(partner) == 63:
            break
    assert len(partner) == 63
    right = np.sort(np.array(partner))
    record_stereo("c_1025_63", RC.subset(big, left, right), sanitized, report, extra={"idx_l": left.astype(np.int32), "idx_r": right.astype(np.int32)})
    one = np.array([hit[0]])
    record_stereo("c_1_63", RC.subset(big, one, right), sanitized, report, extra={"idx_l": one.astype(np.int32), "idx_r": right.astype(np.int32)})
    # (d) the pyramid as written: patches from level 0
    record_stereo("d_4lev_240x320", RC.extracted_case(O, wsp, 240, 320, 17, seed=17, nlevels=4, kmax=300), sanitized, report)
    record_stereo("d_8lev_480x752", RC.extracted_case(O, wsp, 480, 752, 13, seed=13, nlevels=8, kmax=PR.features_per_level(1000, 1.2, 8)),
                  sanitized, report)
    record_stereo("d_constructed", RC.constructed_pyramid(), sanitized, report)


def gen_geometry(sanitized, notes):
    calls = [(H, W, L, sf) for (H, W) in GEO_SIZES for L in GEO_LEVELS for sf in GEO_SCALES]
    # sizes where multiplying by the reciprocal and dividing round to different pixel counts
    found = []
    for sf, L in ((1.2, 8), (1.1, 8), (1.5, 4), (1.2, 16)):
        _, _, s = SR.geometry(8, 8, L, sf)
        inv = (f32(1.0) / s).astype(np.float32)
        for X in range(8, 4097):
            x = f32(X)
            a, b = np.rint(x * inv), np.rint(x / s)
            if (a != b).any():
                found.append((X, L, sf))
    notes.append(f"geometry: {len(found)} (size, nlevels, scale) combinations in 8..4096 where lrintf(X * (1/s)) != lrintf(X / s) at some level; "
                 f"the first 16 are recorded: {found[:16]}")
    differs = list(range(len(calls), len(calls) + min(len(found), 16)))
    calls += [(X, X, L, sf) for X, L, sf in found[:16]]
    n = len(calls)
    out = {"args": np.array([(H, W, L) for H, W, L, _ in calls], np.int32), "sf": np.array([c[3] for c in calls], np.float32),
           "scale": np.zeros((n, 16), np.float32), "inv": np.zeros((n, 16), np.float32), "level_w": np.zeros((n, 16), np.int32),
           "level_h": np.zeros((n, 16), np.int32), "fpl": np.zeros((n, 16), np.int32), "division_differs": np.array(differs, np.int32),
           "n_division_differs_found": np.array([len(found)], np.int32)}
    for i, (H, W, L, sf) in enumerate(calls):
        g = R.geometry(H, W, L, sf, 1000, sanitized=sanitized)
        for k in ("scale", "inv", "level_w", "level_h", "fpl"):
            out[k][i, :L] = g[k]
    RC.save("geometry", out)
    print(f"geometry: {n} calls, {len(found)} division-differs combinations found")


def gen_distinctive(sanitized):
    rng = np.random.default_rng(21)
    lens = list(DISTINCTIVE_COUNTS) + [0, 10, 7, 2, 9] + [int(v) for v in rng.integers(1, 40, 20)]
    off = np.zeros(len(lens) + 1, np.int32); off[1:] = np.cumsum(lens)
    centers = rng.standard_normal((len(lens), 256))
    desc = np.repeat(centers, lens, axis=0) + 0.3 * rng.standard_normal((off[-1], 256))
    desc = desc / np.linalg.norm(desc, axis=1, keepdims=True)
    codes = RC.quantize(desc)
    p = len(DISTINCTIVE_COUNTS) + 1                       # the 10-observation point: a duplicated observation -> tied rows
    codes[off[p] + 7] = codes[off[p] + 3]
    p += 1                                                # the 7-observation point: ALL rows equal -> every median ties, index 0 wins
    codes[off[p]:off[p + 1]] = codes[off[p]]
    best = R.distinctive(RC.dequantize(codes), off, sanitized=sanitized)
    RC.save("distinctive", {"desc_q7": codes, "offsets": off, "ref_best": best})
    print(f"distinctive: {len(lens)} points, {int(off[-1])} observations, best[:12] = {best[:12].tolist()}")


def gen_small(sanitized):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((37, 256)).astype(np.float32); a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.standard_normal((101, 256)).astype(np.float32); b /= np.linalg.norm(b, axis=1, keepdims=True)
    for j in range(0, 101, 3):                            # a third are noisy copies, so that distances spread over 0.3 .. 1.45
        v = a[j % 37] + rng.uniform(0.01, 0.09) * rng.standard_normal(256).astype(np.float32)
        b[j] = (v / np.linalg.norm(v)).astype(np.float32)
    b[5] = a[5]                                           # an exact zero
    RC.save("distance", {"a": a, "b": b, "ref_dist": R.distance(a, b, sanitized=sanitized)})
    nk = {}
    for h, w in NORMKP_SIZES:
        k = np.concatenate([rng.integers(0, [w, h], (100, 2)).astype(np.float32), (rng.random((100, 2)) * [w, h]).astype(np.float32),
                            np.array([[0, 0], [w - 1, h - 1], [w / 2, h / 2], [w, h]], np.float32)])
        nk[f"k_{h}x{w}"] = k
        nk[f"ref_{h}x{w}"] = R.normalize_keypoints(k, h, w, sanitized=sanitized)
    RC.save("normkp", nk)
    d = rng.standard_normal((6, 256)).astype(np.float32)
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0], np.float32)
    d[0, :] = np.resize(tiny, 256)
    d[1, :] = np.resize(tiny[::-1], 256)
    d[2, ::2] = 0.0; d[2, 1::2] = -0.0
    d[3, :] = np.resize(np.array([1e-45, -1e-45, 3e-42, -3e-42], np.float32), 256)
    RC.save("binarize", {"desc": d, "ref_bits": R.binarize(d, sanitized=sanitized)})
    print("distance / normkp / binarize recorded")


def gen_bow(sanitized):
    """vocabularies as DBoW3's toStream wrote them, its dump of them, Vocabulary::transform on every case, the database scripts"""
    for name in BC.VOCABS:
        v, pools, cases = BC.source(name)
        stream = R.voc_write(BR.stream_bytes(v), False, sanitized=sanitized)          # our writer -> fromStream -> DBoW3's toStream
        d = R.voc_dump(stream, sanitized=sanitized)
        arrays = {"stream": np.frombuffer(stream, np.uint8), "pools": np.array(list(pools)),
                  "dump_hdr": np.array([d[k] for k in ("k", "L", "scoring", "weighting", "n_nodes", "n_words", "D")], np.int32),
                  "dump_words": d["words"], "cases": np.array([(list(pools).index(p), n, u) for p, n, u in cases], np.int32)}
        if name == "oneword":                                                          # the smallest tree: also as a compressed stream
            arrays["stream_compressed"] = np.frombuffer(R.voc_write(stream, True, sanitized=sanitized), np.uint8)
        for k in BR.VOCAB_ARRAYS:
            arrays["dump_" + k] = d[k]
        for p, a in pools.items():
            arrays["pool_" + p] = a
        census, fv_ok = [], []
        dv = BC.dump_dict(arrays)
        for i, (p, n, u) in enumerate(cases):
            r = R.transform(stream, pools[p][:n], u, sanitized=sanitized)
            ok = bool((r["nid"] >= 0).all())
            fv_ok.append(ok)
            for k in BC.BOW_OUT:
                if ok or not k.startswith("fv_"):                                      # an unwritten *nid: the FeatureVector is garbage
                    arrays[f"c{i}_{k}"] = r[k]
            census.append(BC.transform_census(dv, pools[p][:n], u))
        arrays["fv_recorded"] = np.array(fv_ok, np.uint8)
        arrays["census_keys"] = np.array(BC.TRANSFORM_CENSUS)
        arrays["census"] = np.array(census, np.int64)
        files = RC.save("bow_" + name, arrays)
        print(f"bow_{name}: {d['n_nodes']} nodes, {len(cases)} cases, census {np.sum(census, axis=0).tolist()}, "
              f"{sum(os.path.getsize(f) for f in files)} bytes in {len(files)} file(s)")
    arrays = {"scripts": np.array([s["name"] for s in BC.kfdb_scripts()]), "census_keys": np.array(BC.KFDB_CENSUS)}
    for s in BC.kfdb_scripts():
        r = R.kfdb(s["n_words"], s["ops"], s["bows"], s["connected"], sanitized=sanitized)
        for k, a in BC.pack_script(s).items():
            arrays[f"{s['name']}_{k}"] = a
        for k in BC.KFDB_OUT:
            arrays[f"{s['name']}_{k}"] = r[k]
        arrays[f"{s['name']}_census"] = np.array(BC.kfdb_census(s), np.int64)
        print(f"bow_kfdb {s['name']}: {int(r['sharing'].shape[1])} entries, {len(s['connected'])} queries, census {arrays[s['name'] + '_census'].tolist()}")
    # L1Scoring::score on its own: pairs of the scripts' BowVectors, the score as float64
    s = BC.script_grow()
    pairs = [(600, e) for e in range(0, 600, 37)] + [(601, 601), (602, 5), (603, 600), (601, 600)]
    arrays["score_pairs"] = np.array(pairs, np.int32)
    arrays["score_ref"] = np.array([R.score(*s["bows"][a], *s["bows"][b], sanitized=sanitized) for a, b in pairs], np.float64)
    files = RC.save("bow_kfdb", arrays)
    print(f"bow_kfdb: {sum(os.path.getsize(f) for f in files)} bytes in {len(files)} file(s)")


def check_bow(sanitized):
    """regenerate into a temporary directory: every ref_bow_* file must come out with the committed bytes"""
    import filecmp
    import glob
    import tempfile
    kept = RC.GOLDEN
    with tempfile.TemporaryDirectory() as d:
        RC.GOLDEN = d
        try:
            gen_bow(sanitized)
        finally:
            RC.GOLDEN = kept
        new = sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "ref_bow_*.npz")))
        old = sorted(os.path.basename(f) for f in glob.glob(os.path.join(kept, "ref_bow_*.npz")))
        bad = [f for f in new if f not in old or not filecmp.cmp(os.path.join(d, f), os.path.join(kept, f), shallow=False)]
        if new != old or bad:
            sys.exit(f"--check: the regenerated fixtures differ: {bad or (new, old)}")
    print(f"--check: {len(new)} ref_bow_* files regenerated with identical bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--report", default=None, help="write the census tables (markdown) here")
    ap.add_argument("--only", default="", help="comma-separated subset of: stereo,geometry,distinctive,small,bow")
    ap.add_argument("--check", action="store_true", help="bow: regenerate into a temporary directory and compare the bytes")
    args = ap.parse_args()
    if not R.usable() or not R.usable_bow():
        sys.exit("oracle/_ref/ref_classic is not built (python oracle/ref_classic/build_ref.py needs the Rover-SLAM checkout)")
    sanitized = R.usable(sanitized=True)
    try:
        R.geometry(240, 320, 4, 1.2, sanitized=sanitized)
    except R.RefError:
        sanitized = False                    # a sanitizer runtime that cannot start here: use the plain build (_GLIBCXX_ASSERTIONS only)
    print(f"reference harness: {'AddressSanitizer + UBSan' if sanitized else 'plain'} build")
    only = set(filter(None, args.only.split(",")))
    report, notes = [], []
    if args.check:
        return check_bow(sanitized and R.usable_bow(sanitized=True))
    if not only or "bow" in only:
        gen_bow(sanitized and R.usable_bow(sanitized=True))
    if not only or "geometry" in only:
        gen_geometry(sanitized, notes)
    if not only or "distinctive" in only:
        gen_distinctive(sanitized)
    if not only or "small" in only:
        gen_small(sanitized)
    if not only or "stereo" in only:
        gen_stereo(sanitized, report)
    if args.report:
        keys = [k for k in SR.CENSUS_KEYS]
        with open(args.report, "w") as f:
            f.write("| census | " + " | ".join(r[0] for r in report) + " |\n|---|" + "---|" * len(report) + "\n")
            f.write("| N / Nr | " + " | ".join(f"{r[1]} / {r[2]}" for r in report) + " |\n")
            for k in keys + ["median_sad"]:
                f.write(f"| {k} | " + " | ".join(str(r[4][k]) for r in report) + " |\n")
            f.write("| survivor octaves | " + " | ".join(str(r[4]["survivor_octaves"]) for r in report) + " |\n")
            f.write("| restatement == reference | " + " | ".join(str(r[3]) for r in report) + " |\n")
            f.write("| bytes (files) | " + " | ".join(f"{r[5]} ({r[6]})" for r in report) + " |\n\n")
            for n in notes:
                f.write(n + "\n")


if __name__ == "__main__":
    main()
