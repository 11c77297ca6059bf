#!/usr/bin/env python3
"""Measurement of the device-resident OptimizeSim3 (rfe_optimize_sim3_dev) at n = 50, 150 and 500 matched pairs (N = n rows,
a fifth of KF1's observations gross outliers, four levels), B = 1 and 8 problems per call, with the scale free and fixed.

Per size, in one process, alternating so that drift of the shared host hits every row:
  * new: every array resident, host clock around call + synchronise (p50 / p95 over --iters calls after --warmup), and the kernel's own
    time from rfe_profile_read (a run of its own);
  * old: the only route a tree without the call offers from Python -- the numpy restatement on the host (tests/optimize_sim3_ref.py), one
    problem at a time.  The reference's own route is g2o in C++, which this project does not build: that time was NOT measured.
The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone decides the exit
status.  Prints markdown (-> profiles/optimize_sim3.md).
usage: python tools/bench_optimize_sim3.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DT = {"s12": np.float64, "s12_f32": np.float32, "keep": np.uint8, "chi2": np.float64, "trace": np.float64, "stats": np.int32}
IN = {"s12_0": np.float64, "xw1": np.float32, "xw2": np.float32, "valid": np.uint8, "kpts1": np.float32, "octave1": np.int32, "idx2": np.int32,
      "kpts2": np.float32, "octave2": np.int32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import optimize_sim3_ref as R
    import stamp
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident OptimizeSim3: times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"Four levels, every pair in KF2, 20 % gross outliers, start 0.05 rad, 0.1 and 3 % off, {a.warmup} warm-up + {a.iters} timed calls per "
          f"row; times in microseconds.\n")
    for n in (50, 150, 500):
        for B in (1, 8):
            for fix in (False, True):
                cases = [R.scene(900 + b, n, fix_scale=fix) for b in range(B)]
                probs = [c["P"] for c in cases]
                P = capi.optimize_sim3_params(probs)
                st = {k: np.ascontiguousarray(np.stack([c[k] for c in cases]), IN[k]) for k in IN}
                ref = R.optimize_sim3_batch(probs, *[st[k] for k in IN])
                up = lambda x: ctx.alloc(max(x.nbytes, 4)).upload(x)   # noqa: E731
                d = {k: up(v) for k, v in st.items()}
                shape = {"s12": (B, 8), "s12_f32": (B, 8), "keep": (B, n), "chi2": (B, n, 2), "trace": (B, 2, 8), "stats": (B, 8)}
                init = {k: (np.ones if k == "keep" else np.zeros)(shape[k], DT[k]) for k in DT}
                o = {k: up(init[k]) for k in DT}

                def new_dev():
                    ctx.optimize_sim3_dev(P, d["s12_0"], d["xw1"], d["xw2"], d["valid"], d["kpts1"], d["idx2"], d["kpts2"], B, n, n, o["s12"],
                                          o["keep"], o["stats"], octave1=d["octave1"], octave2=d["octave2"], s12_f32=o["s12_f32"], chi2=o["chi2"],
                                          trace=o["trace"])
                    ctx.synchronize()

                def old():
                    return [R.solve(c) for c in cases]
                new_dev()
                got = {k: o[k].download(shape[k], DT[k]) for k in DT}
                good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in DT)
                ok = ok and bool(good)
                s = ref["stats"]
                print(f"## n = {n}, B = {B}, fix_scale = {int(fix)}\n")
                print(f"Check against the restatement (every output): {'pass' if good else 'FAIL'}.  Per problem {s[:, 1].min()}..{s[:, 1].max()} pairs, "
                      f"{s[:, 2].min()}..{s[:, 2].max()} removed after round 1, {s[:, 4].min()}..{s[:, 4].max()} LM iterations, {s[:, 5].min()}.."
                      f"{s[:, 5].max()} trials and {s[:, 6].min()}..{s[:, 6].max()} rejected (one pass over the pairs per trial, plus one per rejected "
                      f"trial that a round goes on from, plus one per round).\n")

                def times(fn, warm, iters):
                    ts = []
                    for it in range(warm + iters):
                        t0 = time.perf_counter()
                        fn()
                        if it >= warm:
                            ts.append((time.perf_counter() - t0) * 1e6)
                    return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))
                routes = (("new: `rfe_optimize_sim3_dev`, every output", new_dev), ("old: the numpy restatement on the host", old))
                rows = {name: [] for name, _ in routes}
                for rep in range(2):
                    for name, fn in routes:
                        rows[name].append(times(fn, a.warmup, a.iters) if fn is not old else times(fn, 1, max(a.iters // 40, 3)))
                print("| route | p50, call + synchronise (two runs) | p95 (two runs) |")
                print("|---|---:|---:|")
                for name, _ in routes:
                    r = rows[name]
                    print(f"| {name} | {r[0][0]:.1f} / {r[1][0]:.1f} | {r[0][1]:.1f} / {r[1][1]:.1f} |")
                ctx.profile(True); ctx.profile_reset()
                for _ in range(a.iters):
                    new_dev()
                ms, calls = ctx.profile_read()["optimize_sim3"]
                ctx.profile(False); ctx.profile_reset()
                passes = s[:, 5] + s[:, 6] + s[:, 3]                 # an upper bound: a rejected trial that ends its round costs no further pass
                print(f"\nThe kernel alone (`optimize_sim3` profile stage), mean per call: {ms / calls * 1e3:.1f}; at most {passes.max()} passes "
                      f"in the slowest problem: {ms / calls * 1e3 / passes.max():.1f} per pass.\n")
                for b in list(d.values()) + list(o.values()):
                    b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
