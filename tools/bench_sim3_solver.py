#!/usr/bin/env python3
"""Measurement of the device-resident Sim3Solver (rfe_sim3_ransac_dev) at n = 50, 150 and 500 correspondences (40 % gross
outliers under a planted Sim3), its = 300 hypotheses, and B = 1 and 8 problems per call.  min_inliers is set above every count, so that all
300 hypotheses are the reference's own work too (no early convergence).

Per size, in one process, alternating so that drift of the shared host hits every row:
  * new: every array resident, host clock around call + synchronise (p50 / p95 over --iters calls after --warmup); and the three launches'
    own times from rfe_profile_read (a run of its own) with their shares;
  * old: the only route a tree without the call offers from Python -- the numpy restatement on the host (tests/sim3_solver_ref.py), one
    problem at a time.
NOT measured: the reference's own route, Eigen's EigenSolver and fixed-size products in C++ (Eigen is not built here), and what the call
saves inside a running loop closer, where the caller stops at the first convergence and the device evaluates every hypothesis.
The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone decides the exit
status.  The departures of the contract from the reference's own choices are measured on the host (tests/sim3_solver_ref.py: measure) and
printed first.  Prints markdown (-> profiles/sim3_solver.md).
usage: python tools/bench_sim3_solver.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STAGES = ("sim3_front", "sim3_hypotheses", "sim3_select")


def departures(R):
    import test_sim3_solver_ref as T
    cases = [T.sized(*a) for a in T.SIZES] + [R.forced(k) for k in R.FORCED] + [T.planted()]
    m = R.measure(cases)
    print("## Departures (a)-(c), measured on the host\n")
    print(f"The contract (fixed-schedule Jacobi on the symmetric N in double, R from the float unit quaternion, left-to-right fp32 sums) against "
          f"the same sequential transcription with the reference's own choices (numpy.linalg.eigh on float64, the angle-axis / half-angle sin "
          f"cos route, float64 sums), over the {len(cases)} cases of tests/test_sim3_solver_ref.py: {m['hypotheses']} hypotheses compared, "
          f"{m['degenerate']} apart (two largest eigenvalues within {R.DEGENERATE:g} |N|: a collinear triple, whose rotation about the line is "
          f"free).\n")
    print("| quantity | largest over all hypotheses | test bound (x 4) |")
    print("|---|---:|---:|")
    print(f"| rotation angle between the two R, rad | {m['angle']:.3g} | {T.ANGLE_BOUND:.3g} |")
    print(f"| relative difference of s | {m['s']:.3g} | {T.S_BOUND:.3g} |")
    print(f"| relative difference of t | {m['t']:.3g} | {T.T_BOUND:.3g} |")
    print(f"| Jacobi residual, norm(N q - lambda q) / norm(N), {R.SWEEPS} sweeps | {m['residual']:.3g} | {T.RESIDUAL_BOUND:.3g} |")
    print(f"\nEvery hypothesis' inlier count, every final flag and every statistic agreed: {m['same_inliers']}.  Smallest relative distance "
          f"of any e1 / e2 of the float64 run to its integer bound: {m['margin']:.3g} (the test asks for more than {T.MARGIN:g}).\n")
    return bool(m["same_inliers"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import sim3_solver_ref as R
    import stamp
    ctx = capi.Context(0)
    print("# Device-resident Sim3Solver: departures and times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    ok = departures(R)
    print("## Times\n")
    print(f"Planted Sim3 (s = 1.3, 0.4 rad), 40 % gross outliers, its = 300, min_inliers = n (no convergence: all 300 hypotheses are the "
          f"reference's too); {a.warmup} warm-up + {a.iters} timed calls per row; times in microseconds.\n")
    DT, H = R.OUT, 300
    for n in (50, 150, 500):
        for B in (1, 8):
            cases = [R.scene(700 + b, n, outliers=0.4, its=H, min_inliers=n) for b in range(B)]
            st = {k: np.stack([c[k] for c in cases]) for k in ("xw1", "xw2", "s1", "s2", "draws")}
            P = capi.sim3_solver_params([c["P"] for c in cases])
            refs = [R.solve(c) for c in cases]
            ref = {k: np.stack([np.asarray(r[k]) for r in refs]) for k in DT}
            up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 4)).upload(np.ascontiguousarray(x))   # noqa: E731
            d = {k: up(v) for k, v in st.items()}
            shape = {"T12": (B, 16), "R": (B, 9), "t": (B, 3), "s": (B,), "inliers": (B, n), "best_inliers": (B, n), "counts": (B, H),
                     "hyps": (B, H, 32), "stats": (B, 8)}
            o = {k: up(np.zeros(shape[k], DT[k])) for k in DT}

            def new_dev():
                ctx.sim3_ransac_dev(P, d["xw1"], d["xw2"], d["s1"], d["s2"], d["draws"], B, n, H, o["T12"], o["stats"],
                                    **{k: o[k] for k in DT if k not in ("T12", "stats")})
                ctx.synchronize()

            def old():
                return [R.solve(c) for c in cases]
            new_dev()
            got = {k: o[k].download(shape[k], DT[k]) for k in DT}
            good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in DT)
            ok = ok and bool(good)
            s = ref["stats"]
            print(f"### n = {n}, B = {B}\n")
            print(f"Check against the restatement (every output): {'pass' if good else 'FAIL'}.  Best counts {s[:, 2].min()}..{s[:, 2].max()}, "
                  f"converged {int(s[:, 0].sum())} of {B}.\n")

            def times(fn, warm, iters):
                ts = []
                for it in range(warm + iters):
                    t0 = time.perf_counter()
                    fn()
                    if it >= warm:
                        ts.append((time.perf_counter() - t0) * 1e6)
                return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))
            routes = (("new: `rfe_sim3_ransac_dev`, every output", new_dev), ("old: the numpy restatement on the host", old))
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
            prof = ctx.profile_read()
            ctx.profile(False); ctx.profile_reset()
            us = {k: prof[k][0] / prof[k][1] * 1e3 for k in STAGES}
            tot = sum(us.values())
            print("\nThe three launches (profile stages, events around each), mean per call: "
                  + ", ".join(f"`{k}` {us[k]:.1f} ({100 * us[k] / tot:.0f} %)" for k in STAGES) + f"; together {tot:.1f}.\n")
            for b in list(d.values()) + list(o.values()):
                b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
