#!/usr/bin/env python3
"""Timing of SuperPoint on a scale pyramid (rfe_extract_pyramid_u8): what SPextractor(1000, 1.2, 8) with RFE_SP_PYRAMID=1 costs per frame.

Configurations: 640 x 480, one frame; 752 x 480, both stereo views (B = 2).  8 levels, scale factor 1.2, budgets mnFeaturesPerLevel(1000).
Per configuration, one JSON line: p50 / p95 of the device-resident call (host clock around the call and a device synchronise, after
warm-up), of the host entry, and of the same work as plain per-level rfe_extract_u8_dev calls on the same level images with the same
budgets (issued back to back, one synchronise), interleaved with the pyramid call in the same process; their ratio; and one oracle check
of the last timed outputs (the only thing that decides the exit status).

    python tools/bench_pyramid.py [--iters N] [--warmup W] [--no-oracle] [--only pyramid]
    python tools/bench_pyramid.py --summarise-trace results.db     (a rocprofv3 --kernel-trace database of an `--only pyramid` run)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [("640x480_b1", 1, 480, 640), ("752x480_b2", 2, 480, 752)]
L, SF = 8, 1.2


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def run(args):
    from rover_slam_amd import capi, weights as Wt, synth
    import pyramid_ref as P
    lib = capi.lib
    wsp = Wt.make_superpoint(seed=7)
    ctx = capi.Context(0)
    ctx.set_weights(capi.KIND_SUPERPOINT, wsp)
    km = np.array(P.features_per_level(1000, SF, L), np.int32)
    K = int(km.sum())
    ok_all = True
    for name, B, H, W in CONFIGS:
        frames = synth.make_frames(B, H, W, seed=3)[0]
        lh, lw, _ = P.geometry(H, W, L, SF)
        tot = int((lh.astype(np.int64) * lw).sum())
        img = ctx.alloc(frames.nbytes).upload(frames)
        d = {k: ctx.alloc(nb) for k, nb in (("n", B * 4), ("ln", B * L * 4), ("kp", B * K * 8), ("oc", B * K * 4), ("sc", B * K * 4),
                                             ("de", B * K * 1024), ("lv", B * tot))}
        # per-level reference calls: each level image as its own tight [B, H_l, W_l] buffer (rfe_extract_u8_dev's frame pitch is stride * H)
        ctx._chk(lib.rfe_extract_pyramid_u8_dev(ctx.h, img.ptr, H, W, W, B, L, SF, km.ctypes.data, 0.0005, d["n"].ptr, d["ln"].ptr, d["kp"].ptr,
                                                d["oc"].ptr, d["sc"].ptr, d["de"].ptr, d["lv"].ptr))
        levels = capi.split_levels(d["lv"].download((B, tot), np.uint8), lh, lw)
        lvl = [ctx.alloc(lv.nbytes).upload(np.ascontiguousarray(lv)) for lv in levels]
        per = {k: ctx.alloc(nb) for k, nb in (("n", B * 4), ("kxy", B * 4096 * 8), ("sc", B * 4096 * 4), ("de", B * 4096 * 1024))}
        run_levels = [l for l in range(L) if km[l] > 0 and lh[l] >= 8 and lw[l] >= 8]
        hn = np.zeros((B,), np.int32); hln = np.zeros((B, L), np.int32); hkp = np.zeros((B, K, 2), np.float32)
        hoc = np.zeros((B, K), np.int32); hsc = np.zeros((B, K), np.float32); hde = np.zeros((B, K, 256), np.float32)

        def pyr_dev():
            ctx._chk(lib.rfe_extract_pyramid_u8_dev(ctx.h, img.ptr, H, W, W, B, L, SF, km.ctypes.data, 0.0005, d["n"].ptr, d["ln"].ptr, d["kp"].ptr,
                                                    d["oc"].ptr, d["sc"].ptr, d["de"].ptr, None))
            ctx.synchronize()

        def pyr_host():
            ctx._chk(lib.rfe_extract_pyramid_u8(ctx.h, frames.ctypes.data, H, W, W, B, L, SF, km.ctypes.data, 0.0005, hn.ctypes.data, hln.ctypes.data,
                                                hkp.ctypes.data, hoc.ctypes.data, hsc.ctypes.data, hde.ctypes.data, None))

        def per_level():
            for l in run_levels:
                ctx._chk(lib.rfe_extract_u8_dev(ctx.h, lvl[l].ptr, int(lh[l]), int(lw[l]), int(lw[l]), B, int(km[l]), 0.0005, per["n"].ptr,
                                                per["kxy"].ptr, per["sc"].ptr, per["de"].ptr))
            ctx.synchronize()

        fns = {"dev": pyr_dev} if args.only == "pyramid" else {"dev": pyr_dev, "host": pyr_host, "per_level": per_level}
        times = {k: [] for k in fns}
        for it in range(args.warmup + args.iters):
            for k, fn in fns.items():          # interleaved: every iteration times each form once
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if it >= args.warmup:
                    times[k].append(dt)
        res = {"config": name, "B": B, "H": H, "W": W, "nlevels": L, "scale_factor": SF, "kmax": km.tolist(), "iters": args.iters}
        for k, v in times.items():
            res[f"{k}_p50_ms"] = round(pct(v, 50), 4)
            res[f"{k}_p95_ms"] = round(pct(v, 95), 4)
        if "per_level" in times:
            res["dev_over_per_level_p50"] = round(res["dev_p50_ms"] / res["per_level_p50_ms"], 4)
        if not args.no_oracle:       # the last timed device outputs against the oracle composed per level
            from oracle import oracle as O
            O.build()
            ref = P.extract(O, wsp, frames, L, SF, km)
            got = {"n": d["n"].download((B,), np.int32), "level_n": d["ln"].download((B, L), np.int32),
                   "kpts": d["kp"].download((B, K, 2), np.float32), "octave": d["oc"].download((B, K), np.int32),
                   "score": d["sc"].download((B, K), np.float32), "desc": d["de"].download((B, K, 256), np.float32)}
            ok = all(np.array_equal(got[k], ref[k]) for k in got)
            if "host" in times:
                ok = ok and np.array_equal(hn, ref["n"]) and np.array_equal(hkp, ref["kpts"]) and np.array_equal(hde, ref["desc"])
            res["oracle_check"] = "pass" if ok else "FAIL"
            res["keypoints"] = got["n"].tolist()
            ok_all = ok_all and ok
        print(json.dumps(res), flush=True)
        for b in list(d.values()) + lvl + list(per.values()) + [img]:
            b.free()
    ctx.close()
    return 0 if ok_all else 1


def summarise(path):
    """Per pyramid call of a trace: resample chain and merge cost, call window, busy / idle share, per-level window and idle share."""
    import sqlite3
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    ncol = "name" if "name" in cols else "kernel_name"
    rows = sorted(db.execute(f"select {ncol}, start, end from kernels").fetchall(), key=lambda r: r[1])
    calls, cur = [], []
    for r in rows:
        cur.append(r)
        if "pyr_merge_kernel" in r[0]:
            calls.append(cur)
            cur = []

    def busy(ks, t0, t1):
        iv = sorted((max(s, t0), min(e, t1)) for _, s, e in ks if e > t0 and s < t1)
        tot, a, b = 0, None, None
        for s, e in iv:
            if a is None or s > b:
                if a is not None:
                    tot += b - a
                a, b = s, e
            else:
                b = max(b, e)
        return tot + ((b - a) if a is not None else 0)

    # an `--only pyramid` run times the configurations one after the other, the same number of calls each
    groups = [calls[i * len(calls) // len(CONFIGS):(i + 1) * len(calls) // len(CONFIGS)] for i in range(len(CONFIGS))] \
        if len(calls) % len(CONFIGS) == 0 else [calls]
    print(f"source: {path}  ({len(calls)} pyramid calls)\n")
    for gi, g in enumerate(groups):
        print(f"### {CONFIGS[gi][0] if len(groups) == len(CONFIGS) else 'all calls'}\n")
        if summarise_calls(g, busy):
            return 1
    return 0


def summarise_calls(calls, busy):
    out = []
    for c in calls:
        t0, t1 = c[0][1], max(e for _, _, e in c)
        lv_starts = [s for nm, s, _ in c if "conv1ab_fused_kernel" in nm]
        merge_s = [s for nm, s, _ in c if "pyr_merge_kernel" in nm][0]
        edges = lv_starts + [merge_s]
        per_level = [(edges[i + 1] - edges[i], busy(c, edges[i], edges[i + 1])) for i in range(len(lv_starts))]
        out.append({"window": t1 - t0, "busy": busy(c, t0, t1), "chain": sum(e - s for nm, s, e in c if "pyr_resample_kernel" in nm),
                    "chain_launches": sum(1 for nm, _, _ in c if "pyr_resample_kernel" in nm),
                    "merge": sum(e - s for nm, s, e in c if "pyr_merge_kernel" in nm), "levels": per_level, "kernels": len(c)})
    if not out:
        print("no pyramid calls in the trace")
        return 1
    out = out[len(out) // 4:]      # drop the first quarter (warm-up)
    med = lambda k: float(np.median([o[k] for o in out])) / 1e3  # noqa: E731  (us)
    print(f"{len(calls)} calls, medians over the last {len(out)}\n")
    print("| per call (median) | us |\n|---|---:|")
    print(f"| window: first kernel start to merge end | {med('window'):.1f} |")
    print(f"| kernel-busy time | {med('busy'):.1f} |")
    print(f"| idle share of the window | {100 * (1 - med('busy') / med('window')):.1f} % |")
    print(f"| resample chain ({out[0]['chain_launches']} launches, side stream) | {med('chain'):.1f} |")
    print(f"| merge (1 launch) | {med('merge'):.1f} |")
    print(f"| kernels per call | {out[0]['kernels']} |")
    nl = len(out[0]["levels"])
    print("\n| level | window us (conv1ab start to next level) | busy us | idle share |\n|---:|---:|---:|---:|")
    for l in range(nl):
        w = float(np.median([o["levels"][l][0] for o in out if len(o["levels"]) == nl])) / 1e3
        b = float(np.median([o["levels"][l][1] for o in out if len(o["levels"]) == nl])) / 1e3
        print(f"| {l} | {w:.1f} | {b:.1f} | {100 * (1 - b / w):.1f} % |")
    print()
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--only", choices=["pyramid"], default=None)
    ap.add_argument("--summarise-trace", default=None)
    a = ap.parse_args()
    sys.exit(summarise(a.summarise_trace) if a.summarise_trace else run(a))
