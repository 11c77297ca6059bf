#!/usr/bin/env python3
"""Measurement of the device-resident GlobalBundleAdjustemnt (rfe_global_ba_dev).

Rows checked bit for bit against the restatement (tests/global_ba_ref.py) before anything is timed -- that comparison alone decides the
exit status: 6l's four rows (robust, the fixed keyframes last), a ring of 70 and a chain of 260 keyframes (robust = 0), and one row past
rfe_local_ba's edge cap (eight keyframes, 16 400 points seen by all, E = 131 200).  Then p50 / p95 over --iters synchronous calls with
every array resident, the stages' own times from rfe_profile_read (a run of its own), and the tiles processed against the dense count.
The (64, 16, 8000, 32 000) row also runs through rfe_local_ba_dev in the same loop, alternating.
Rows too large for the restatement (about 256 and 1024 keyframes in a band of covisibility closed by one loop, about 30 000 and 200 000
points): only that the host and device forms agree, that every output is finite and that currentChi never rises is checked there.
Prints markdown (-> profiles/global_ba.md).  No exit status depends on a time.
usage: python tools/bench_global_ba.py [--iters 20] [--warmup 2] [--no-large]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DT = {"pose": np.float64, "pose_f32": np.float32, "point": np.float64, "point_f32": np.float32, "included": np.uint8, "chi2": np.float64,
      "trace": np.float64, "stats": np.int32}
IN = (("kf_pose", np.float32), ("kf_cam", np.float32), ("kf_nlevels", np.int32), ("kf_sigma2", np.float32), ("kf_feat_off", np.int32),
      ("fixed", np.uint8), ("kpts", np.float32), ("xw", np.float32), ("edge_point", np.int32), ("edge_kf", np.int32), ("edge_feat", np.int32))
STAGES = ("gba_validate", "gba_structure", "gba_linearise", "gba_trial", "gba_errors", "gba_finish")
LSTAGES = ("lba_validate", "lba_structure", "lba_linearise", "lba_trial", "lba_errors", "lba_finish")


def band(K, L, width=6, loop=40, seed=0):
    """per point four keyframes out of a window of `width` consecutive ones; the last `loop` points close the ring"""
    rng = np.random.default_rng(seed)
    vis = []
    for p in range(L):
        if p >= L - loop:
            ks = sorted({0, 1, K - 2, K - 1})
        else:
            s = int(rng.integers(0, K - width + 1))
            ks = sorted(int(v) for v in s + rng.choice(width, 4, replace=False))
        vis.append(ks)
    return vis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-large", action="store_true")
    a = ap.parse_args()
    from rover_slam_amd import capi
    import global_ba_ref as G
    import local_ba_ref as LR
    import stamp
    ctx = capi.Context(0)
    ok = True
    print("# Device-resident GlobalBundleAdjustemnt: times\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    print(f"Four levels, mixed mono / stereo; {a.warmup} warm-up + {a.iters} timed synchronous calls per row, every array resident; times in "
          f"milliseconds.\n")

    def params_of(c):
        p = c["params"]
        return capi.global_ba_params(p["iterations"], p["max_trials"], p["user_lambda_init"], p["robust"], p["huber2_mono"], p["huber2_stereo"])

    def resident(c):
        K, L, E, Nf, its = len(c["fixed"]), len(c["xw"]), len(c["edge_point"]), len(c["kpts"]), c["params"]["iterations"]
        up = lambda x: ctx.alloc(max(x.nbytes, 8)).upload(x)   # noqa: E731
        d = [up(np.ascontiguousarray(c[k], dt)) for k, dt in IN]
        oc, ur = up(np.ascontiguousarray(c["octave"], np.int32)), up(np.ascontiguousarray(c["uright"], np.float32))
        shape = {"pose": (K, 7), "pose_f32": (K, 7), "point": (L, 3), "point_f32": (L, 3), "included": (L,), "chi2": (E,), "trace": (its, 4), "stats": (8,)}
        o = {k: up(np.zeros(shape[k], DT[k])) for k in DT}
        lp = params_of(c)

        def call():
            ctx.global_ba_dev(lp, K, L, E, Nf, *d, o["pose"], o["point"], o["included"], o["stats"], octave=oc, uright=ur, pose_f32=o["pose_f32"],
                              point_f32=o["point_f32"], chi2=o["chi2"], trace=o["trace"])

        def read():
            return {k: o[k].download(shape[k], DT[k]) for k in DT}
        return call, read, d + [oc, ur] + list(o.values())

    def timed(calls):
        """p50 / p95 of every callable, alternating, so that drift of the shared host hits every route"""
        ts = [[] for _ in calls]
        for it in range(a.warmup + a.iters):
            for n, f in enumerate(calls):
                t0 = time.perf_counter()
                f()
                if it >= a.warmup:
                    ts[n].append((time.perf_counter() - t0) * 1e3)
        return [(np.percentile(t, 50), np.percentile(t, 95)) for t in ts]

    def stages(call, names):
        n = max(a.iters // 4, 3)
        ctx.profile(True); ctx.profile_reset()
        for _ in range(n):
            call()
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile(False); ctx.profile_reset()
        return ", ".join(f"`{k}` {prof[k][0] / n:.3f}" for k in names if k in prof)

    rows = []
    for Pn, Fn, L in ((4, 2, 300), (10, 4, 1500), (24, 8, 4000), (64, 16, 8000)):
        lc = LR.scene(800 + Pn, Pn, Fn, L, "mixed", gross=0.05, gross_px=(10.0, 20.0))
        rows.append((f"6l's row P = {Pn}, F = {Fn}, L = {L} (robust)", G.from_local(lc), lc))
    for name, K, ppk in (("loop", 70, 6), ("chain", 260, 3)):
        c = G.scene(900 + K, K, [0], G.pattern(name, K, ppk=ppk), "mixed", ring=name == "loop")
        c["params"] = G.params(iterations=10)
        rows.append((f"{name} of {K} keyframes, {ppk} points per keyframe (robust = 0)", c, None))
    c = G.from_local(LR.scene(808, 7, 1, 16400, "mixed", all_see=True))
    c["params"] = G.params(iterations=3)
    rows.append(("eight keyframes, 16 400 points seen by all: past rfe_local_ba's edge cap (robust = 0, 3 iterations)", c, None))

    print("## Rows checked bit for bit\n")
    for title, c, lc in rows:
        t0 = time.perf_counter()
        ref = G.global_ba(c, c["params"])
        t_ref = (time.perf_counter() - t0) * 1e3
        call, read, bufs = resident(c)
        call()
        got = read()
        good = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in DT)
        ok = ok and bool(good)
        s = ref["stats"]
        print(f"### {title}\n")
        print(f"K = {len(c['fixed'])}, L = {len(c['xw'])}, E = {len(c['edge_point'])}.  Check against the restatement (every output): "
              f"{'pass' if good else 'FAIL'}.  {s[0]} LM iterations, {s[1]} trials, {s[2]} rejected, {s[3]} failed solves, {s[5]} free keyframes, "
              f"{s[6]} tiles processed of {s[7]} in the dense triangle.\n")
        calls, labels = [call], ["`rfe_global_ba_dev`, every output"]
        if lc is not None and lc["P"] == 64:
            lp = lc["params"]
            up = lambda x: ctx.alloc(max(x.nbytes, 8)).upload(x)   # noqa: E731
            lin = [up(np.ascontiguousarray(lc[k], dt)) for k, dt in IN if k != "fixed"]
            loc, lur = up(np.ascontiguousarray(lc["octave"], np.int32)), up(np.ascontiguousarray(lc["uright"], np.float32))
            E, L = len(lc["edge_point"]), len(lc["xw"])
            lo = [up(np.zeros((64, 7))), up(np.zeros((L, 3))), up(np.zeros(E, np.uint8)), up(np.zeros(8, np.int32))]
            lpar = capi.local_ba_params(lp["iterations"], lp["max_trials"], lp["user_lambda_init"], lp["th2_mono"], lp["th2_stereo"])

            def local_call():
                ctx.local_ba_dev(lpar, lc["P"], lc["F"], L, E, len(lc["kpts"]), *lin, *lo, octave=loc, uright=lur)
            local_call()
            same_pose = np.array_equal(lo[0].download((64, 7), np.float64), got["pose"][:64])
            ok = ok and bool(same_pose)
            calls.append(local_call)
            labels.append(f"`rfe_local_ba_dev` on the same problem (poses bit-equal: {'yes' if same_pose else 'NO'})")
            bufs += lin + [loc, lur] + lo
        res = timed(calls)
        print("| route | p50 | p95 |")
        print("|---|---:|---:|")
        for lab, (p50, p95) in zip(labels, res):
            print(f"| {lab} | {p50:.2f} | {p95:.2f} |")
        print(f"| the numpy restatement on the host (one run) | {t_ref:.0f} | |")
        print("\nThe stages alone (profile events), mean per call: " + stages(call, STAGES) + ".")
        if len(calls) > 1:
            print("\n`rfe_local_ba_dev`'s stages: " + stages(calls[1], LSTAGES) + ".")
            g, l = res[0][0], res[1][0]
            print(f"\nThe tiled factorisation {'does not lose' if g <= l else 'LOSES'} to the one-workgroup one on this row: {g:.2f} against {l:.2f} ms "
                  f"a call; the stage that differs is the trial (the solve rides in `gba_trial` / `lba_trial`).")
        print()
        for b in bufs:
            b.free()

    if not a.no_large:
        print("## Rows too large for the restatement\n")
        print("Checked here: the host and device forms agree on every output, every output is finite, currentChi never rises over the accepted "
              "iterations.  Nothing else was checked at these sizes.\n")
        for K, L in ((256, 30000), (1024, 200000)):
            c = G.scene(1000 + K, K, [0], band(K, L, seed=K), "mixed", ring=True, spacing=0.4)
            c["params"] = G.params(iterations=5)
            call, read, bufs = resident(c)
            call()
            got = read()
            host = ctx.global_ba(params_of(c), *(c[k] for k, _ in IN), octave=c["octave"], uright=c["uright"])
            agree = all(np.array_equal(got[k], host[k], equal_nan=True) for k in DT)
            finite = all(np.all(np.isfinite(got[k])) for k in ("pose", "point", "chi2", "trace"))
            chi = got["trace"][:got["stats"][0], 2]
            falls = bool(np.all(np.diff(chi) <= 0))
            ok = ok and agree and finite and falls
            s = got["stats"]
            print(f"### band of six keyframes closed by one loop: K = {K}, L = {L}, E = {len(c['edge_point'])} (robust = 0, 5 iterations)\n")
            print(f"Host and device forms agree: {'yes' if agree else 'NO'}; finite: {'yes' if finite else 'NO'}; currentChi never rises: "
                  f"{'yes' if falls else 'NO'} ({chi[0]:.6g} -> {chi[-1]:.6g}).  {s[0]} LM iterations, {s[1]} trials, {s[2]} rejected, {s[3]} failed "
                  f"solves, {s[5]} free keyframes, {s[6]} tiles processed of {s[7]} in the dense triangle.\n")
            (p50, p95), = timed([call])
            print("| route | p50 | p95 |")
            print("|---|---:|---:|")
            print(f"| `rfe_global_ba_dev`, every output | {p50:.2f} | {p95:.2f} |")
            print("\nThe stages alone (profile events), mean per call: " + stages(call, STAGES) + ".\n")
            for b in bufs:
                b.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
