#!/usr/bin/env python3
"""Measurement of the device-resident SearchByProjection1 (rfe_search_by_projection_dev) at Rover-SLAM's sizes: a 752 x 480
frame with Nf = 1024 features, a local map of Nq = 2000 projected points, window factor th in {1, 6} (th = 1: tracking a stereo / RGB-D
frame from the motion model; th = 6: the widest factor Tracking::SearchLocalPoints passes, right after a relocalisation).

Per th, in one process:
  * the new call: host clock around call + synchronise (p50 / p95 over --iters calls after --warmup), --iters asynchronous calls issued
    back to back between two synchronisations, and the per-kernel time from rfe_profile_read (a run of its own: the events keep
    consecutive kernels from overlapping);
  * rfe_search_candidates_dev ALONE on the same candidate lists (uploaded once as CSR): the device part of the route a tree without the
    new call offers.  It is a lower bound of that route, which pays the host grid walk, the per-frame upload of the lists and the host
    assignment loop on top.
The outputs of the new call are compared with tests/projection_search_ref.py (exact) before anything is timed; that comparison alone
decides the exit status.  Prints markdown (-> profiles/projection_search.md).
usage: python tools/bench_projection_search.py [--iters 200] [--warmup 20] [--once TH]   (--once: check + a few calls, for a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, NF, NQ = 752, 480, 1024, 2000


def make_case(th, seed=0):
    """tests/projection_search_ref.py's contention case at Rover-SLAM's sizes (descriptor clusters follow the coarse position)"""
    import projection_search_ref as PS
    rng = np.random.default_rng(seed)
    kxy = np.stack([rng.integers(0, W, NF), rng.integers(0, H, NF)], 1).astype(np.int32)
    centre = rng.standard_normal((40, 256)).astype(np.float32)
    cluster = (kxy[:, 0] // 94 + 8 * (kxy[:, 1] // 96)) % 40
    desc = centre[cluster] + np.float32(0.03) * rng.standard_normal((NF, 256)).astype(np.float32)
    desc = np.ascontiguousarray(desc / np.linalg.norm(desc, axis=1, keepdims=True), np.float32)
    src = rng.integers(0, NF, NQ)
    q = np.ascontiguousarray(desc[src] + np.float32(0.02) * rng.standard_normal((NQ, 256)).astype(np.float32), np.float32)
    proj = np.ascontiguousarray(kxy[src].astype(np.float32) + rng.uniform(-3, 3, (NQ, 2)).astype(np.float32), np.float32)
    radius = (np.where(rng.random(NQ) < 0.5, np.float32(2.5), np.float32(4.0)).astype(np.float32) * np.float32(th)).astype(np.float32)
    c = {"bounds": (0.0, 0.0, float(W), float(H)), "kxy": kxy, "kpts": kxy.astype(np.float32), "desc": desc, "q": q, "proj": proj,
         "radius": radius, "skip": (rng.random(NF) < 0.2).astype(np.uint8), "observed": (rng.random(NQ) < 0.9).astype(np.uint8)}
    c["lists"] = PS.case_lists(c)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--once", type=float, default=None)
    a = ap.parse_args()
    from rover_slam_amd import capi
    from oracle import oracle as O
    import projection_search_ref as PS
    import stamp
    O.build()
    ctx = capi.Context(0)
    lib = capi.lib
    ok = True
    print("# Device-resident SearchByProjection1 at Rover-SLAM's sizes\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"{W} x {H}, Nf = {NF} features, Nq = {NQ} map points, {a.warmup} warm-up + {a.iters} timed calls per row; times in microseconds.\n")
    for th in ([a.once] if a.once is not None else [1.0, 6.0]):
        c = make_case(th)
        off, cand = PS.to_csr(c["lists"])
        total = int(off[-1])
        ref = PS.search_by_projection_seq(O, c["q"], c["desc"], c["lists"], c["skip"], c["observed"])
        up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 4)).upload(np.ascontiguousarray(x))   # noqa: E731
        d = {k: up(c[k]) for k in ("q", "proj", "radius", "desc", "kxy", "skip", "observed")}
        d["off"], d["cand"] = up(off), up(cand)
        o = {k: ctx.alloc(n * 4) for k, n in (("assign", NF), ("bi", NQ), ("bd", NQ), ("sd", NQ), ("st", 4), ("bi2", NQ), ("bd2", NQ), ("sd2", NQ))}
        cap = max(total, 1)

        def new():
            ctx.search_by_projection_dev(d["q"], d["proj"], d["radius"], NQ, d["desc"], NF, c["bounds"], cap, o["assign"], o["st"], kxy=d["kxy"],
                                         observed=d["observed"], skip=d["skip"], best_idx=o["bi"], best_dist=o["bd"], second_dist=o["sd"])

        def scan():
            ctx._chk(lib.rfe_search_candidates_dev(ctx.h, d["q"].ptr, NQ, d["desc"].ptr, NF, d["off"].ptr, d["cand"].ptr, d["skip"].ptr,
                                                   o["bi2"].ptr, o["bd2"].ptr, o["sd2"].ptr))
        new(); scan(); ctx.synchronize()
        st = o["st"].download((4,), np.int32)
        got = {"assign": o["assign"].download((NF,), np.int32), "best_idx": o["bi"].download((NQ,), np.int32),
               "best_dist": o["bd"].download((NQ,), np.float32), "second_dist": o["sd"].download((NQ,), np.float32)}
        good = all(np.array_equal(got[k], ref[k]) for k in got) and st[0] == ref["nmatches"] and st[1] == total and st[3] == 0
        sbi, sbd, ssd = O.search_candidates(c["q"], c["desc"], off, cand, c["skip"])
        good = good and np.array_equal(o["bi2"].download((NQ,), np.int32), sbi) and np.array_equal(o["bd2"].download((NQ,), np.float32), sbd)
        ok = ok and bool(good)
        differ = int((sbi != ref["best_idx"]).sum())
        print(f"## th = {th:g}\n")
        print(f"Check against the restatement: {'pass' if good else 'FAIL'}.  {total} candidates ({total / NQ:.1f} per map point, most "
              f"{max(len(l) for l in c['lists'])}), {int(st[0])} accepted map points, {int(st[2])} rounds; {differ} of {NQ} map points end "
              f"with another feature than the static scan gives them.\n")
        if a.once is not None:
            for _ in range(5):
                new(); scan()
            ctx.synchronize()
            continue

        def sync_times(fn):
            ts = []
            for it in range(a.warmup + a.iters):
                t0 = time.perf_counter()
                fn(); ctx.synchronize()
                if it >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e6)
            return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))

        def back_to_back(fn):
            fn(); ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) / a.iters * 1e6
        # alternate the two so that drift of the shared host hits both
        rows = {"new": [], "scan": []}
        for rep in range(2):
            rows["new"].append(sync_times(new) + (back_to_back(new),))
            rows["scan"].append(sync_times(scan) + (back_to_back(scan),))
        print("| call | p50, call + synchronise (two runs) | p95 | back to back, per call (two runs) |")
        print("|---|---:|---:|---:|")
        for name, key in ((f"`rfe_search_by_projection_dev` (grid + lists + scan + assignment)", "new"),
                          (f"`rfe_search_candidates_dev` alone, same {total} candidates (lists made and uploaded beforehand)", "scan")):
            r = rows[key]
            print(f"| {name} | {r[0][0]:.1f} / {r[1][0]:.1f} | {r[0][1]:.1f} / {r[1][1]:.1f} | {r[0][2]:.1f} / {r[1][2]:.1f} |")
        rn, rs = min(r[0] for r in rows["new"]), min(r[0] for r in rows["scan"])
        bn, bs = min(r[2] for r in rows["new"]), min(r[2] for r in rows["scan"])
        print(f"\nRatio new call / bare scan: {rn / rs:.2f} (p50 with synchronise), {bn / bs:.2f} (back to back).\n")
        ctx.profile(True); ctx.profile_reset()
        for _ in range(a.iters):
            new()
        scan_n = a.iters
        for _ in range(scan_n):
            scan()
        prof = ctx.profile_read()
        ctx.profile(False); ctx.profile_reset()
        print("| kernel (profile stage) | mean per call |")
        print("|---|---:|")
        tot = 0.0
        for name in ("ps_grid", "ps_count", "ps_fill", "ps_resolve"):
            ms, calls = prof[name]
            tot += ms / calls * 1e3
            print(f"| `{name}` | {ms / calls * 1e3:.1f} |")
        print(f"| sum of the four | {tot:.1f} |")
        ms, calls = prof["search_candidates"]
        print(f"| `search_candidates` (the bare scan) | {ms / calls * 1e3:.1f} |\n")
        for b in list(d.values()) + list(o.values()):
            b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
