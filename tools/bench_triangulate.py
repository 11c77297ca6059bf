#!/usr/bin/env python3
"""Measurement of the device-resident CreateNewMapPoints (rfe_triangulate_neighbours_dev) at a mapping-like size: 752 x 480
keyframes of 1024 features, Kmax = 1024 match slots per neighbour (about 800 used), 10 / 20 / 30 neighbours, eight scale levels.

Per neighbour count, in one process, alternating so that drift of the shared host hits every row:
  * new: every array resident (S / pairs where rfe_match_dev leaves them), host clock around call + synchronise (p50 / p95 over --iters
    calls after --warmup); the same plus the download of the created list (out_n, out_idx1, out_idx2, out_x3d, out_stereo, stats), which
    is what the mapping thread goes on with; and the per-stage time from rfe_profile_read (a run of its own);
  * old: the only route a tree without the call offers -- S and pairs downloaded, then the filter and the geometry loop on the host, here
    the vectorised numpy restatement (tests/triangulation_ref.py; the reference's own loop is scalar C++ with Eigen, which this project
    does not build: that time was NOT measured).
The outputs of the new call are compared with the restatement (exact) before anything is timed; that comparison alone decides the exit
status.  Prints markdown (-> profiles/triangulate.md).
usage: python tools/bench_triangulate.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H, N, K = 752, 480, 1024, 1024
STAGES = ("tri_eval", "tri_resolve")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import triangulation_ref as T
    import stamp
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident CreateNewMapPoints at a mapping size\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"{W} x {H}, {N} features per keyframe, Kmax = {K}, eight levels, far points on, not inertial, {a.warmup} warm-up + {a.iters} timed "
          f"calls per row; times in microseconds.\n")
    for Nn in (10, 20, 30):
        base, c = T.make_case(7, W=W, H=H, N1=N, N2=(N,) * Nn, S=tuple(760 + 8 * (n % 6) for n in range(Nn)), Kmax=K, invalid=None, plants=False)
        P = T.P(base, True, False)
        ref = T.triangulate(P, c)
        p, v1 = T.to_capi(P), T.view_to_capi(c["view1"])
        views = (capi.TriView * Nn)(*[T.view_to_capi(v) for v in c["views2"]])
        up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 4)).upload(np.ascontiguousarray(x))   # noqa: E731
        d = {k: up(c[k]) for k in ("kpts1", "octave1", "uright1", "depth1", "has_mp1", "kpts2", "octave2", "uright2", "depth2", "has_mp2", "n2", "S",
                                   "pairs")}
        d["views2"] = up(np.frombuffer(bytes(views), np.uint8))
        dt = {"code": np.int32, "x3d": np.float32, "point_stereo": np.uint8, "out_n": np.int32, "out_idx1": np.int32, "out_idx2": np.int32,
              "out_x3d": np.float32, "out_stereo": np.uint8, "matches": np.int32}
        shape = {"code": (Nn, K), "x3d": (Nn, K, 3), "point_stereo": (Nn, K), "out_n": (N,), "out_idx1": (N,), "out_idx2": (N,), "out_x3d": (N, 3),
                 "out_stereo": (N,), "matches": (Nn,)}
        o = {k: ctx.alloc(int(np.prod(shape[k])) * np.dtype(dt[k]).itemsize) for k in dt}
        o["stats"] = ctx.alloc(32)
        lst = ("out_n", "out_idx1", "out_idx2", "out_x3d", "out_stereo")

        def new_dev(outs=tuple(dt)):
            ctx.triangulate_neighbours_dev(p, v1, d["kpts1"], d["octave1"], d["uright1"], d["depth1"], d["has_mp1"], N, d["views2"], d["kpts2"],
                                           d["octave2"], d["uright2"], d["depth2"], d["has_mp2"], d["n2"], Nn, N, d["S"], d["pairs"], K, o["stats"],
                                           **{k: o[k] for k in outs})
            ctx.synchronize()

        def new_list():
            new_dev(lst)
            st = o["stats"].download((8,), np.int32)
            return st, [o[k].download(shape[k], dt[k])[:st[0]] for k in lst]

        def old():
            S = d["S"].download((Nn,), np.int32)
            pairs = d["pairs"].download((Nn, K, 2), np.int32)
            return T.triangulate(P, dict(c, S=S, pairs=pairs))
        new_dev()
        got = {k: o[k].download(shape[k], dt[k]) for k in dt}
        st = o["stats"].download((8,), np.int32)
        for k in lst:
            got[k] = got[k][:st[0]]
        good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in dt) and np.array_equal(st, ref["stats"])
        st2, l2 = new_list()
        good = good and np.array_equal(st2, ref["stats"]) and all(np.array_equal(x, ref[k], equal_nan=True) for k, x in zip(lst, l2))
        good = good and np.array_equal(old()["out_x3d"], ref["out_x3d"], equal_nan=True)
        ok = ok and bool(good)
        print(f"## {Nn} neighbours\n")
        print(f"Check against the restatement (every output, all of them and the list alone): {'pass' if good else 'FAIL'}.  {int(st[1])} slots, "
              f"{int(st[2])} dropped for a map point, {int(st[0])} points created ({int(st[3])} from stereo, {int(st[4])} stereo attempts), "
              f"{int((ref['code'] == T.CLAIMED).sum())} slots claimed by an earlier neighbour.\n")

        def times(fn):
            ts = []
            for it in range(a.warmup + a.iters):
                t0 = time.perf_counter()
                fn()
                if it >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e6)
            return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))
        routes = (("new: `rfe_triangulate_neighbours_dev`, every output", new_dev), ("new, the list alone, downloaded", new_list),
                  ("old: S / pairs downloaded + the numpy restatement on the host", old))
        rows = {name: [] for name, _ in routes}
        for rep in range(2):
            for name, fn in routes:
                rows[name].append(times(fn) if fn is not old else times_few(fn, a))
        print("| route | p50, call + synchronise (two runs) | p95 (two runs) |")
        print("|---|---:|---:|")
        for name, _ in routes:
            r = rows[name]
            print(f"| {name} | {r[0][0]:.1f} / {r[1][0]:.1f} | {r[0][1]:.1f} / {r[1][1]:.1f} |")
        best = [min(r[0] for r in rows[name]) for name, _ in routes]
        print(f"\nOld / new, p50: {best[2] / best[0]:.0f} (every output), {best[2] / best[1]:.0f} (list downloaded).\n")
        ctx.profile(True); ctx.profile_reset()
        for _ in range(a.iters):
            new_dev()
        prof = ctx.profile_read()
        ctx.profile(False); ctx.profile_reset()
        print("| profile stage | mean per call |")
        print("|---|---:|")
        for name in STAGES:
            ms, calls = prof[name]
            print(f"| `{name}` | {ms / calls * 1e3:.1f} |")
        print()
        for b in list(d.values()) + list(o.values()):
            b.free()
    ctx.close()
    return 0 if ok else 1


def times_few(fn, a):
    """the host route takes tens of milliseconds: a tenth of the calls"""
    ts = []
    for it in range(max(a.warmup // 10, 1) + max(a.iters // 10, 5)):
        t0 = time.perf_counter()
        fn()
        if it >= max(a.warmup // 10, 1):
            ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))


if __name__ == "__main__":
    sys.exit(main())
