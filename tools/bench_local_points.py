#!/usr/bin/env python3
"""Measurement of the device-resident SearchLocalPoints (rfe_search_local_points / _dev) at a tracking-like size: a 752 x 480
frame with Nf = 1024 features, Np = 4000 local map points, th in {1, 6}, one scale level, far points on.

Per th, in one process, alternating so that drift of the shared host hits every row:
  * new, device form: every array resident, host clock around call + synchronise (p50 / p95 over --iters calls after --warmup), and the
    per-kernel time from rfe_profile_read (a run of its own: the events keep consecutive kernels from overlapping);
  * old, device form: the only route a tree without the new call offers with resident descriptors -- isInFrustum and the radius on the
    host (tests/local_points_ref.front, vectorised numpy), proj / radius uploaded, rfe_search_by_projection_dev, synchronise;
  * new and old, host form: the same two routes through the host-pointer entries, which upload the descriptors (5 MB) on every call.
The outputs of the new call are compared with tests/local_points_ref.py (exact) before anything is timed; that comparison alone decides
the exit status.  Prints markdown (-> profiles/search_local_points.md).
usage: python tools/bench_local_points.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, NF, NP = 752, 480, 1024, 4000
STAGES = ("lp_frustum", "ps_grid", "ps_count", "ps_fill", "ps_resolve")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from rover_slam_amd import capi
    from oracle import oracle as O
    import local_points_ref as LP
    import stamp
    O.build()
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident SearchLocalPoints at a tracking size\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"{W} x {H}, Nf = {NF} features, Np = {NP} local map points, one scale level, RFE_LEVEL_ZERO, far points on, {a.warmup} warm-up + "
          f"{a.iters} timed calls per row; times in microseconds.\n")
    base, c = LP.make_case(0, W=W, H=H, Nf=NF, Np=NP)
    for th in (1, 6):
        P = LP.P(base, th, True, LP.LEVEL_ZERO)
        ref = LP.search(O, P, c)
        total = max(ref["candidates"], 1)
        p = LP.to_capi(P)
        up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 4)).upload(np.ascontiguousarray(x))   # noqa: E731
        d = {k: up(c[k]) for k in ("q", "pw", "normal", "min_dist", "max_dist", "scale_dist", "valid", "observed", "desc", "kpts", "skip")}
        o = {k: ctx.alloc(n * 4) for k, n in (("assign", NF), ("best_idx", NP), ("best_dist", NP), ("second_dist", NP), ("proj", 2 * NP),
                                              ("proj_xr", NP), ("depth", NP), ("view_cos", NP), ("level", NP), ("reject", NP), ("st", 8),
                                              ("oproj", 2 * NP), ("oradius", NP), ("st_old", 4))}
        per_point = ("best_idx", "best_dist", "second_dist", "proj", "proj_xr", "depth", "view_cos", "level", "reject")

        def new_dev():
            ctx.search_local_points_dev(p, d["q"], d["pw"], d["normal"], d["min_dist"], d["max_dist"], d["scale_dist"], NP, d["desc"], NF, total,
                                        o["assign"], o["st"], valid=d["valid"], observed=d["observed"], kpts=d["kpts"], skip=d["skip"],
                                        **{k: o[k] for k in per_point})
            ctx.synchronize()

        def old_dev():
            f = LP.front(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["valid"])
            o["oproj"].upload(f["proj"]); o["oradius"].upload(f["radius"])
            ctx.search_by_projection_dev(d["q"], o["oproj"], o["oradius"], NP, d["desc"], NF, P["bounds"], total, o["assign"], o["st_old"],
                                         kpts=d["kpts"], skip=d["skip"], observed=d["observed"], best_idx=o["best_idx"], best_dist=o["best_dist"],
                                         second_dist=o["second_dist"])
            ctx.synchronize()

        def new_host():
            return ctx.search_local_points(p, c["q"], c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["desc"],
                                           valid=c["valid"], observed=c["observed"], kpts=c["kpts"], skip=c["skip"])

        def old_host():
            f = LP.front(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["valid"])
            return ctx.search_by_projection(c["q"], f["proj"], f["radius"], c["desc"], P["bounds"], kpts=c["kpts"], skip=c["skip"],
                                            observed=c["observed"])
        new_dev()
        st = o["st"].download((8,), np.int32)
        shape = lambda k: (NF,) if k == "assign" else ((NP, 2) if k == "proj" else (NP,))   # noqa: E731
        got = {k: o[k].download(shape(k), ref[k].dtype) for k in LP.KEYS}
        good = all(np.array_equal(got[k], ref[k]) for k in got)
        good = good and list(st[[0, 1, 3, 4, 5]]) == [ref["nmatches"], ref["candidates"], 0, ref["in_frustum"], ref["searched"]]
        h = new_host()
        good = good and all(np.array_equal(h[k], ref[k]) for k in got)
        oh = old_host()
        good = good and np.array_equal(oh["assign"], ref["assign"]) and np.array_equal(oh["best_idx"], ref["best_idx"])
        old_dev()
        good = good and np.array_equal(o["assign"].download((NF,), np.int32), ref["assign"])
        ok = ok and bool(good)
        print(f"## th = {th}\n")
        print(f"Check against the restatement (device and host form, and the old routes): {'pass' if good else 'FAIL'}.  "
              f"{ref['in_frustum']} of {NP} map points are in the frustum, {ref['searched']} reach the search, {ref['candidates']} candidates (most "
              f"{max(len(l) for l in ref['lists'])} per map point), {int(st[0])} accepted, {int(st[2])} rounds.\n")

        def times(fn):
            ts = []
            for it in range(a.warmup + a.iters):
                t0 = time.perf_counter()
                fn()
                if it >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e6)
            return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))
        routes = (("new, device form: `rfe_search_local_points_dev`", new_dev),
                  ("old, device form: numpy front + upload of proj / radius + `rfe_search_by_projection_dev`", old_dev),
                  ("new, host form: `rfe_search_local_points`", new_host),
                  ("old, host form: numpy front + `rfe_search_by_projection`", old_host))
        rows = {name: [] for name, _ in routes}
        for rep in range(2):
            for name, fn in routes:
                rows[name].append(times(fn))
        print("| route | p50, call + synchronise (two runs) | p95 (two runs) |")
        print("|---|---:|---:|")
        for name, _ in routes:
            r = rows[name]
            print(f"| {name} | {r[0][0]:.1f} / {r[1][0]:.1f} | {r[0][1]:.1f} / {r[1][1]:.1f} |")
        t0 = time.perf_counter()
        for _ in range(a.iters):
            LP.front(P, c["pw"], c["normal"], c["min_dist"], c["max_dist"], c["scale_dist"], c["valid"])
        front_us = (time.perf_counter() - t0) / a.iters * 1e6
        best = {name: min(r[0] for r in rows[name]) for name, _ in routes}
        names = [name for name, _ in routes]
        print(f"\nThe numpy front alone: {front_us:.1f} per call.  Old / new, p50: {best[names[1]] / best[names[0]]:.2f} (device form), "
              f"{best[names[3]] / best[names[2]]:.2f} (host form).  Old minus its host front: {best[names[1]] - front_us:.1f} (device form), "
              f"{best[names[3]] - front_us:.1f} (host form).\n")
        ctx.profile(True); ctx.profile_reset()
        for _ in range(a.iters):
            new_dev()
        prof = ctx.profile_read()
        ctx.profile(False); ctx.profile_reset()
        print("| kernel (profile stage) | mean per call |")
        print("|---|---:|")
        tot = 0.0
        for name in STAGES:
            ms, calls = prof[name]
            tot += ms / calls * 1e3
            print(f"| `{name}` | {ms / calls * 1e3:.1f} |")
        print(f"| sum of the five | {tot:.1f} |\n")
        for b in list(d.values()) + list(o.values()):
            b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
