#!/usr/bin/env python3
"""Measurement of the device-resident LocalBundleAdjustment (rfe_local_ba_dev) at a few sizes up to P = 64 free keyframes
(four levels, mixed mono / stereo, every point seen by four keyframes, 5 % of the observations displaced by 10 .. 20 px).

Per size, in one process, alternating so that drift of the shared host hits every row:
  * new: every array resident, host clock around the call (it is synchronous: it returns when the optimisation has finished), p50 / p95
    over --iters calls after --warmup, and the stages' own times from rfe_profile_read (a run of its own);
  * old: the only route a tree without the call offers from Python -- the numpy restatement on the host (tests/local_ba_ref.py).
    The reference's own route is g2o in C++, which this project does not build: that time was NOT measured.
The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone decides the exit
status.  Prints markdown (-> profiles/local_ba.md).
usage: python tools/bench_local_ba.py [--iters 30] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DT = {"pose": np.float64, "pose_f32": np.float32, "point": np.float64, "point_f32": np.float32, "erase": np.uint8, "chi2": np.float64,
      "trace": np.float64, "stats": np.int32}
IN = (("kf_pose", np.float32), ("kf_cam", np.float32), ("kf_nlevels", np.int32), ("kf_sigma2", np.float32), ("kf_feat_off", np.int32),
      ("kpts", np.float32), ("xw", np.float32), ("edge_point", np.int32), ("edge_kf", np.int32), ("edge_feat", np.int32))
STAGES = ("lba_validate", "lba_structure", "lba_linearise", "lba_trial", "lba_errors", "lba_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import local_ba_ref as R
    import stamp
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident LocalBundleAdjustment: times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"Four levels, mixed mono / stereo, four observations per point, 5 % displaced by 10 .. 20 px, start 0.02 rad / 0.05 m / 0.05 m off, "
          f"iterations = 10; {a.warmup} warm-up + {a.iters} timed calls per row; times in milliseconds.\n")
    for Pn, Fn, L in ((4, 2, 300), (10, 4, 1500), (24, 8, 4000), (64, 16, 8000)):
        c = R.scene(800 + Pn, Pn, Fn, L, "mixed", gross=0.05, gross_px=(10.0, 20.0))
        t0 = time.perf_counter()
        ref = R.local_ba(c, c["params"])
        t_ref = (time.perf_counter() - t0) * 1e3
        E, Nf, its = len(c["edge_point"]), len(c["kpts"]), c["params"]["iterations"]
        up = lambda x: ctx.alloc(max(x.nbytes, 8)).upload(x)   # noqa: E731
        d = [up(np.ascontiguousarray(c[k], dt)) for k, dt in IN]
        oc, ur = up(np.ascontiguousarray(c["octave"], np.int32)), up(np.ascontiguousarray(c["uright"], np.float32))
        shape = {"pose": (Pn, 7), "pose_f32": (Pn, 7), "point": (L, 3), "point_f32": (L, 3), "erase": (E,), "chi2": (E,), "trace": (its, 4), "stats": (8,)}
        o = {k: up(np.zeros(shape[k], DT[k])) for k in DT}
        lp = capi.local_ba_params(its)

        def new_dev():
            ctx.local_ba_dev(lp, Pn, Fn, L, E, Nf, *d, o["pose"], o["point"], o["erase"], o["stats"], octave=oc, uright=ur, pose_f32=o["pose_f32"],
                             point_f32=o["point_f32"], chi2=o["chi2"], trace=o["trace"])
        new_dev()
        got = {k: o[k].download(shape[k], DT[k]) for k in DT}
        good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in DT)
        ok = ok and bool(good)
        s = ref["stats"]
        print(f"## P = {Pn}, F = {Fn}, L = {L}, E = {E}\n")
        print(f"Check against the restatement (every output): {'pass' if good else 'FAIL'}.  {s[0]} LM iterations, {s[1]} trials, {s[2]} rejected, "
              f"{s[3]} failed solves, {s[4]} edges erased, {s[6]} edges on free keyframes, {s[7]} Schur pair-list entries.\n")
        ts = []
        for it in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            new_dev()
            if it >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        print("| route | p50 | p95 |")
        print("|---|---:|---:|")
        print(f"| new: `rfe_local_ba_dev`, every output | {np.percentile(ts, 50):.2f} | {np.percentile(ts, 95):.2f} |")
        print(f"| old: the numpy restatement on the host (one run) | {t_ref:.0f} | |")
        ctx.profile(True); ctx.profile_reset()
        for _ in range(max(a.iters // 3, 3)):
            new_dev()
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile(False); ctx.profile_reset()
        n = max(a.iters // 3, 3)
        print("\nThe stages alone (profile events), mean per call: " +
              ", ".join(f"`{k}` {prof[k][0] / n:.3f}" for k in STAGES if k in prof) + ".\n")
        for b in d + [oc, ur] + list(o.values()):
            b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
