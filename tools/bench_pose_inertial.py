#!/usr/bin/env python3
"""Measurement of the device-resident PoseInertialOptimization (rfe_pose_inertial_optimization_dev) in both modes at
N = 150, 600 and 4096 features (nine in ten with a map point, a fifth of those gross outliers, mono and stereo edges mixed over four
levels), one problem per call.

Per size, in one process, alternating so that drift of the shared host hits every row:
  * new: every array resident, host clock around call + synchronise (p50 / p95 over --iters calls after --warmup), LastKeyFrame and
    LastFrame; and the kernel's own time from rfe_profile_read (a run of its own);
  * beside it: rfe_pose_optimization_dev on the same build at the same size (tests/pose_opt_ref.py's scene), the 6-dimensional
    Levenberg-Marquardt whose serial section is about a hundredth of this one's;
  * old: the numpy restatement on the host (tests/pose_inertial_ref.py).  The reference's own route is g2o in C++, which this project
    does not build: that time was NOT measured.
The kernel's time at N = 150 against N = 4096 splits it into lane 0's serial section (the same at every size) and the passes over the
edges (which grow with N): that split decides whether the serial section is worth spreading over a wave.
The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone decides the exit
status.  Prints markdown (-> profiles/pose_inertial.md).
usage: python tools/bench_pose_inertial.py [--iters 100] [--warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DT = {"state": np.float64, "state_f32": np.float32, "outlier": np.uint8, "chi2": np.float32, "prior_out": np.float64, "trace": np.float64,
      "stats": np.int32}
IN = {"mode": np.int32, "rec_init": np.int32, "cam": np.float32, "state": np.float32, "prev_state": np.float32, "preint": np.float32,
      "cov_rw": np.float32, "kpts": np.float32, "octave": np.int32, "uright": np.float32, "xw": np.float32, "has_mp": np.uint8,
      "track_depth": np.float32}


def times(fn, warm, iters):
    ts = []
    for it in range(warm + iters):
        t0 = time.perf_counter()
        fn()
        if it >= warm:
            ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import pose_inertial_ref as R
    import pose_opt_ref as PO
    import stamp
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident PoseInertialOptimization: times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"Four levels, mixed mono / stereo edges, 20 % gross outliers, start 2 degrees and 5 cm off, a preintegration over 0.05 s, "
          f"{a.warmup} warm-up + {a.iters} timed calls per row; times in microseconds.\n")
    up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 4)).upload(np.ascontiguousarray(x))   # noqa: E731
    kernel = {}
    for N in (150, 600, 4096):
        print(f"## N = {N}\n")
        routes, frees = [], []
        for mode, label in ((R.MODE_LAST_KEYFRAME, "LastKeyFrame"), (R.MODE_LAST_FRAME, "LastFrame")):
            c = R.scene(500 + N, N, mode, "mixed")
            P, x = c["P"], c["args"]
            p = capi.pose_inertial_params(P["fx"], P["fy"], P["cx"], P["cy"], P["bf"], P["inv_level_sigma2"])
            ref = R.solve(c)
            d = {k: up(np.asarray(x[k], dt)) for k, dt in IN.items()}
            d["prior_in"] = up(np.asarray(x["prior_in"], np.float64)) if x["prior_in"] is not None else None
            shape = {"state": (21,), "state_f32": (21,), "outlier": (N,), "chi2": (N,), "prior_out": (246,), "trace": (4, 8), "stats": (16,)}
            o = {k: up(np.zeros(shape[k], DT[k])) for k in DT}
            frees += [b for b in list(d.values()) + list(o.values()) if b is not None]

            def new_dev(p=p, d=d, o=o, N=N):
                ctx.pose_inertial_optimization_dev(p, d["mode"], d["cam"], d["state"], d["prev_state"], d["preint"], d["cov_rw"], d["kpts"], d["xw"],
                                                   d["has_mp"], d["track_depth"], 1, N, o["state"], o["outlier"], o["stats"], prior_in=d["prior_in"],
                                                   rec_init=d["rec_init"], octave=d["octave"], uright=d["uright"], state_f32=o["state_f32"],
                                                   chi2=o["chi2"], prior_out=o["prior_out"], trace=o["trace"])
                ctx.synchronize()
            new_dev()
            got = {k: o[k].download(shape[k], DT[k]) for k in DT}
            good = all(np.array_equal(got[k], np.asarray(ref[k]), equal_nan=True) for k in DT)
            ok = ok and bool(good)
            s = ref["stats"]
            print(f"{label}: check against the restatement (every output) {'pass' if good else 'FAIL'}; {s[1]} edges, {s[2]} outliers, {s[6]} "
                  f"Gauss-Newton iterations.\n")
            routes.append((f"new: `rfe_pose_inertial_optimization_dev`, {label}", new_dev, (a.warmup, a.iters)))
            routes.append((f"old: the numpy restatement on the host, {label}", lambda c=c: R.solve(c), (1, 3)))
            ctx.profile(True); ctx.profile_reset()
            for _ in range(max(a.iters // 4, 5)):
                new_dev()
            ms, calls = ctx.profile_read()["pose_inertial"]
            ctx.profile(False); ctx.profile_reset()
            kernel[(N, label)] = ms / calls * 1e3
        pc = PO.scene(500 + N, N, "mixed")
        PP = pc["P"]
        pp = capi.pose_params(PP["fx"], PP["fy"], PP["cx"], PP["cy"], PP["bf"], PP["inv_level_sigma2"])
        dp = {k: up(pc[k]) for k in ("pose0", "kpts", "octave", "uright", "xw", "has_mp")}
        op = {"pose": up(np.zeros(7)), "outlier": up(np.zeros(N, np.uint8)), "stats": up(np.zeros(8, np.int32))}
        frees += list(dp.values()) + list(op.values())

        def pose_opt():
            ctx.pose_optimization_dev(pp, dp["pose0"], dp["kpts"], dp["xw"], dp["has_mp"], 1, N, op["pose"], op["outlier"], op["stats"],
                                      octave=dp["octave"], uright=dp["uright"])
            ctx.synchronize()
        routes.append(("beside it: `rfe_pose_optimization_dev`, the same size", pose_opt, (a.warmup, a.iters)))
        rows = {name: [] for name, _, _ in routes}
        for rep in range(2):
            for name, fn, (w, n) in routes:
                rows[name].append(times(fn, w, n))
        print("| route | p50, call + synchronise (two runs) | p95 (two runs) |")
        print("|---|---:|---:|")
        for name, _, _ in routes:
            r = rows[name]
            print(f"| {name} | {r[0][0]:.1f} / {r[1][0]:.1f} | {r[0][1]:.1f} / {r[1][1]:.1f} |")
        print(f"\nThe kernel alone (`pose_inertial` profile stage), mean per call: LastKeyFrame {kernel[(N, 'LastKeyFrame')]:.1f}, "
              f"LastFrame {kernel[(N, 'LastFrame')]:.1f}.\n")
        for b in frees:
            b.free()
    print("## Which side dominates\n")
    for label in ("LastKeyFrame", "LastFrame"):
        lo, hi = kernel[(150, label)], kernel[(4096, label)]
        print(f"{label}: {lo:.1f} at 150 features, {hi:.1f} at 4096.  A pass costs a lane one edge at 150 features and sixteen at 4096; lane 0's serial section "
              f"is the same at both.  With T = S + edges-per-lane x c that gives c = {(hi - lo) / 15:.1f} and S = {lo - (hi - lo) / 15:.1f}: the serial "
              f"section is {100 * (1 - (hi - lo) / 15 / lo):.0f} % of the call at 150 features and {100 * (lo - (hi - lo) / 15) / hi:.0f} % at 4096.\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
