#!/usr/bin/env python3
"""Timing of the per-stereo-frame entry for scale pyramids (rfe_stereo_frame_pyramid_dev) at 752 x 480, 8 levels, scale factor 1.2, budgets
mnFeaturesPerLevel(1000), against the work a tree without it can do for such a frame.

    --mode frame      rfe_stereo_frame_pyramid_dev in steady state (previous view present); the last timed outputs are checked against
                      the oracle composed per level + tests/stereo_pyramid_ref.py -- the only thing that decides the exit status
    --mode yardstick  rfe_extract_pyramid_u8_dev with B = 2 plus one rfe_match_dev pair at Mmax = Nmax = Ktot, issued back to back with
                      one synchronise: everything except the stereo match.  Uses entries older than this tool, so --root may name
                      another checkout of the project (a built parent commit) to be measured with the same script
    --mode single     rfe_stereo_frame_dev at Kmax = 1000 on the same views (for a kernel trace next to the pyramid one)

One JSON line: p50 / p95 in ms of the host clock around call + device synchronise, after warm-up.  No timing decides the exit status."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, L, SF, DISP = 480, 752, 8, 1.2, 13
MB, MBF = 0.11, 0.11 * 435.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["frame", "yardstick", "single"], default="frame")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--root", default=HERE, help="checkout whose built library is measured")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    from rover_slam_amd import capi, weights as Wt, synth
    import pyramid_ref as P
    lib = capi.lib
    wsp, wlg = Wt.make_superpoint(seed=7), Wt.make_lightglue(seed=11)
    ctx = capi.Context(0)
    ctx.set_weights(capi.KIND_SUPERPOINT, wsp)
    ctx.set_weights(capi.KIND_LIGHTGLUE, wlg)
    km = np.array(P.features_per_level(1000, SF, L), np.int32)
    K = int(km.sum())
    rng = np.random.default_rng(13)
    scene = synth.make_scene(rng, H, W + DISP, margin=0)
    left = np.clip(scene[:, :W] + rng.integers(0, 8, (H, W)), 0, 255).astype(np.uint8)
    right = np.clip(scene[:, DISP:DISP + W] + rng.integers(0, 8, (H, W)), 0, 255).astype(np.uint8)
    frames = np.ascontiguousarray(np.stack([left, right]))
    img = ctx.alloc(frames.nbytes).upload(frames)
    res = {"mode": a.mode, "root": os.path.basename(os.path.abspath(a.root)), "H": H, "W": W, "nlevels": L, "scale_factor": SF, "kmax": km.tolist(),
           "iters": a.iters}
    st = None
    if a.mode == "frame":
        st = capi.StereoPyramidStream(ctx, H, W, L, SF, km, mb=MB, mbf=MBF)

        def call():
            st.push(img.ptr, img.ptr + H * W)
            ctx.synchronize()
    elif a.mode == "single":
        st = capi.StereoStream(ctx, H, W, K, mb=MB, mbf=MBF)

        def call():
            st.push(img.ptr, img.ptr + H * W)
            ctx.synchronize()
    else:
        d = {k: ctx.alloc(nb) for k, nb in (("n", 8), ("kp", 2 * K * 8), ("oc", 2 * K * 4), ("sc", 2 * K * 4), ("de", 2 * K * 1024), ("kn", 2 * K * 8),
                                             ("S", 4), ("pairs", K * 8), ("ms", K * 4))}

        def extract():
            ctx._chk(lib.rfe_extract_pyramid_u8_dev(ctx.h, img.ptr, H, W, W, 2, L, SF, km.ctypes.data, 0.0005, d["n"].ptr, None, d["kp"].ptr,
                                                    d["oc"].ptr, d["sc"].ptr, d["de"].ptr, None))
        extract()
        ctx.synchronize()
        kp = d["kp"].download((2, K, 2), np.float32)
        d["kn"].upload(((kp - np.float32([W / 2, H / 2])) / np.float32(max(H, W) / 2)).astype(np.float32))   # NormalizeKeypoints, staged once

        def call():
            extract()
            ctx._chk(lib.rfe_match_dev(ctx.h, d["kn"].ptr, d["kn"].ptr + K * 8, d["de"].ptr, d["de"].ptr + K * 1024, d["n"].ptr, d["n"].ptr + 4,
                                       1, K, K, 0.1, d["S"].ptr, d["pairs"].ptr, d["ms"].ptr))
            ctx.synchronize()
    times = []
    for it in range(a.warmup + a.iters):
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if it >= a.warmup:
            times.append(dt)
    res["p50_ms"] = round(float(np.percentile(times, 50)), 4)
    res["p95_ms"] = round(float(np.percentile(times, 95)), 4)
    ok = True
    if a.mode == "frame" and not a.no_check:
        import stereo_pyramid_ref as SR
        from oracle import oracle as O
        O.build()
        got = st.results()
        ref = P.extract(O, wsp, frames, L, SF, km)
        ok = all(np.array_equal(got[k], ref[k]) for k in ("n", "level_n", "kpts", "octave", "score", "desc"))
        nl, nr = int(ref["n"][0]), int(ref["n"][1])
        _, _, s = P.geometry(H, W, L, SF)
        u, z = SR.stereo_match([lv[0] for lv in ref["levels"]], [lv[1] for lv in ref["levels"]], s, ref["kpts"][0, :nl], ref["octave"][0, :nl],
                               ref["kpts"][1, :nr], ref["octave"][1, :nr], ref["desc"][0, :nl], ref["desc"][1, :nr], MB, MBF, SR.SAD_LEVEL)
        ok = ok and np.array_equal(got["u_right"][:nl], u) and np.array_equal(got["depth"][:nl], z) and bool((got["u_right"][nl:] == -1).all())
        res["check"] = "pass" if ok else "FAIL"
        res["keypoints"] = [nl, nr]
        res["stereo_matches"] = int((u >= 0).sum())
        res["temporal_matches"] = got["S"]
    print(json.dumps(res), flush=True)
    if st is not None:
        st.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
