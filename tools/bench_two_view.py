#!/usr/bin/env python3
"""Measurement of the device-resident TwoViewReconstruction (rfe_two_view_dev) at 100, 300, 1000 and 4096 matches x 200
iterations, one problem per call, on the general planted scene of tests/two_view_ref.py.

Per size, in one process:
  * new: every array resident, host clock around call + synchronise (p50 / p95 over --iters calls after --warmup);
  * the numpy restatement on the host (tests/two_view_ref.py: every hypothesis at once);
  * the sequential transcription of the reference's lines on the host (tests/two_view_seq.py: numpy.linalg.svd per hypothesis), the
    nearest thing to the reference's own route that runs here.
NOT measured: the reference's own C++ (Eigen's JacobiSVD on two std::threads; Eigen is not built here), which this project has never
timed either.  The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone
decides the exit status -- no time does.  Prints markdown (-> profiles/two_view.md).
usage: python tools/bench_two_view.py [--iters 100] [--warmup 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def times(fn, warm, iters):
    ts = []
    for it in range(warm + iters):
        t0 = time.perf_counter()
        fn()
        if it >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import stamp
    import two_view_ref as R
    import two_view_seq as Q
    ctx = capi.Context(0)
    print("# Device-resident TwoViewReconstruction: times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"General planted scene, 0.2 px noise, 5 % outliers, 200 iterations of both models, one problem per call; {a.warmup} warm-up + "
          f"{a.iters} timed calls for the device row, 3 calls for the host rows; milliseconds.\n")
    print("| matches | check | answer, model, nGood | `rfe_two_view_dev` p50 / p95 | restatement (numpy, host) | transcription (numpy.linalg.svd, host) |")
    print("|---:|---|---|---:|---:|---:|")
    ok = True
    DT = R.OUT
    for n in (100, 300, 1000, 4096):
        c = R.scene(900 + n, n, its=200, extra1=0 if n == 4096 else 17, extra2=0 if n == 4096 else 29)
        P, n1, n2, H = c["P"], c["P"]["n1"], c["P"]["n2"], 200
        ref = R.run(c)
        up = lambda x, dt: ctx.alloc(max(np.ascontiguousarray(x, dt).nbytes, 4)).upload(np.ascontiguousarray(x, dt))   # noqa: E731
        d = {"kpts1": up(c["kpts1"], np.float32), "kpts2": up(c["kpts2"], np.float32), "S": up(np.array([c["S"]]), np.int32),
             "pairs": up(c["pairs"], np.int32), "draws": up(c["draws"], np.int32)}
        shape = {"R21": (9,), "t21": (3,), "p3d": (n1, 3), "triangulated": (n1,), "inliers_h": (n,), "inliers_f": (n,), "scores": (H, 2),
                 "models": (2, 9), "cand": (8, 16), "stats": (16,)}
        o = {k: up(np.zeros(shape[k], DT[k]), DT[k]) for k in DT}
        PA = capi.two_view_params([P])

        def new_dev():
            ctx.two_view_dev(PA, d["kpts1"], d["kpts2"], d["S"], d["pairs"], d["draws"], 1, n1, n2, n, H, o["R21"], o["t21"], o["stats"],
                             **{k: o[k] for k in DT if k not in ("R21", "t21", "stats")})
            ctx.synchronize()
        new_dev()
        got = {k: o[k].download(shape[k], DT[k]) for k in DT}
        good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in DT)
        ok = ok and bool(good)
        t_new = times(new_dev, a.warmup, a.iters)
        t_ref = times(lambda: R.run(c), 0, 3)
        t_seq = times(lambda: Q.reconstruct(P, c["kpts1"], c["kpts2"], c["pairs"], c["draws"]), 0, 3)
        s = ref["stats"]
        print(f"| {n} | {'pass' if good else 'FAIL'} | {s[0]}, {('none', 'H', 'F')[s[1]]}, {int(ref['cand'][max(s[7], 0), 12])} | "
              f"{t_new[0]:.3f} / {t_new[1]:.3f} | {t_ref[0]:.0f} | {t_seq[0]:.0f} |")
        for b in list(d.values()) + list(o.values()):
            b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
