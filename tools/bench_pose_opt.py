#!/usr/bin/env python3
"""Measurement of the device-resident PoseOptimization (rfe_pose_optimization_dev) at N = 300, 1024 and 4096 features (nine in
ten with a map point, a fifth of those gross outliers, mono and stereo edges mixed over four levels) and B = 1 and 8 problems per call.

Per size, in one process, alternating so that drift of the shared host hits every row:
  * new: every array resident, host clock around call + synchronise (p50 / p95 over --iters calls after --warmup); the same plus the
    download of pose_f32 (the one 7-float read a resident caller makes before the frustum search); and the kernel's own time from
    rfe_profile_read (a run of its own);
  * old: the only route a tree without the call offers from Python -- the numpy restatement on the host (tests/pose_opt_ref.py), one
    problem at a time.  The reference's own route is g2o in C++, which this project does not build: that time was NOT measured.
The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone decides the exit
status.  Prints markdown (-> profiles/pose_opt.md).
usage: python tools/bench_pose_opt.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DT = {"pose": np.float64, "pose_f32": np.float32, "outlier": np.uint8, "chi2": np.float32, "trace": np.float64, "stats": np.int32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import pose_opt_ref as R
    import stamp
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident PoseOptimization: times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"Four levels, mixed mono / stereo edges, 20 % gross outliers, start 0.05 rad and 0.1 m off, {a.warmup} warm-up + {a.iters} timed calls "
          f"per row; times in microseconds.\n")
    for N in (300, 1024, 4096):
        for B in (1, 8):
            cases = [R.scene(500 + b, N, "mixed") for b in range(B)]
            P = cases[0]["P"]
            p = capi.pose_params(P["fx"], P["fy"], P["cx"], P["cy"], P["bf"], P["inv_level_sigma2"])
            st = {k: np.stack([c[k] for c in cases]) for k in ("pose0", "kpts", "octave", "uright", "xw", "has_mp")}
            ref = R.pose_optimization_batch(P, st["pose0"], st["kpts"], st["octave"], st["uright"], st["xw"], st["has_mp"])
            up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 4)).upload(np.ascontiguousarray(x))   # noqa: E731
            d = {k: up(v) for k, v in st.items()}
            shape = {"pose": (B, 7), "pose_f32": (B, 7), "outlier": (B, N), "chi2": (B, N), "trace": (B, 4, 8), "stats": (B, 8)}
            o = {k: up(np.zeros(shape[k], DT[k])) for k in DT}

            def new_dev(extra=("pose_f32", "chi2", "trace")):
                ctx.pose_optimization_dev(p, d["pose0"], d["kpts"], d["xw"], d["has_mp"], B, N, o["pose"], o["outlier"], o["stats"],
                                          octave=d["octave"], uright=d["uright"], **{k: o[k] for k in extra})
                ctx.synchronize()

            def new_pose():
                new_dev(("pose_f32",))
                return o["pose_f32"].download((B, 7), np.float32)

            def old():
                return [R.solve(c) for c in cases]
            new_dev()
            got = {k: o[k].download(shape[k], DT[k]) for k in DT}
            good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in DT) and np.array_equal(new_pose(), ref["pose_f32"])
            ok = ok and bool(good)
            s = ref["stats"]
            print(f"## N = {N}, B = {B}\n")
            print(f"Check against the restatement (every output): {'pass' if good else 'FAIL'}.  Per problem {s[:, 1].min()}..{s[:, 1].max()} edges, "
                  f"{s[:, 2].min()}..{s[:, 2].max()} outliers, {s[:, 4].min()}..{s[:, 4].max()} LM iterations and {s[:, 5].min()}..{s[:, 5].max()} trials "
                  f"(one pass over the edges per trial, plus one per rejected trial that a round goes on from).\n")

            def times(fn, warm, iters):
                ts = []
                for it in range(warm + iters):
                    t0 = time.perf_counter()
                    fn()
                    if it >= warm:
                        ts.append((time.perf_counter() - t0) * 1e6)
                return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))
            routes = (("new: `rfe_pose_optimization_dev`, every output", new_dev), ("new, pose_f32 alone, downloaded", new_pose),
                      ("old: the numpy restatement on the host", old))
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
            ms, calls = ctx.profile_read()["pose_opt"]
            ctx.profile(False); ctx.profile_reset()
            print(f"\nThe kernel alone (`pose_opt` profile stage), mean per call: {ms / calls * 1e3:.1f}.\n")
            for b in list(d.values()) + list(o.values()):
                b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
