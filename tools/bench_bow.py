#!/usr/bin/env python3
"""Measurement of the device-resident ComputeBoW3 and keyframe-database scoring (rfe_bow_transform_dev, rfe_bow_db_query_dev).

  * transform: N = 1024 SuperPoint-like float descriptors against a full k = 10, L = 6 vocabulary (1 111 111 nodes, 10^6 words, D = 256,
    random 0/1 node descriptors, 284 MB of them on the device); descriptors resident, host clock around call + synchronise, p50 / p95 over
    --iters calls after --warmup; the per-stage time from rfe_profile_read in a run of its own;
  * query: a database of 1 000 / 10 000 BoW vectors of 600..1000 words, each drawn from a pool of 20 000 of the vocabulary's words so that
    keyframes share words the way views of one place do; the query is one more such vector, resident.
Next to each, in the same process and alternating, the numpy restatement on the host (tests/bow_ref.py) on the same inputs -- NOT the
reference's DBoW3 C++, which this project does not build: that time was not measured.  The outputs of the device calls are compared with
the restatement (exact, float64 bit for bit) before anything is timed; that comparison alone decides the exit status.  Prints markdown
(-> profiles/bow.md).
usage: python tools/bench_bow.py [--iters 200] [--warmup 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K, L, D, N = 10, 6, 256, 1024


def full_vocab(rng):
    """the full k-ary tree in breadth-first numbering, built with array arithmetic: node i's children are k i + 1 .. k i + k"""
    n = (K ** (L + 1) - 1) // (K - 1)
    inner = (K ** L - 1) // (K - 1)
    ids = np.arange(n, dtype=np.int64)
    off = np.minimum(ids, inner) * K
    word_id = np.where(ids >= inner, ids - inner, -1).astype(np.int32)
    weight = np.zeros((n,), np.float64)
    weight[inner:] = np.log(rng.integers(1000, 2000, n - inner) / rng.integers(1, 900, n - inner))
    return {"k": K, "L": L, "weighting": 0, "scoring": 0, "n_nodes": n, "D": D, "parent": ((ids - 1) // K).astype(np.int32),
            "child_offsets": np.r_[off, n - 1].astype(np.int32), "children": np.arange(1, n, dtype=np.int32),
            "desc": rng.integers(0, 2, (n, D), dtype=np.uint8), "weight": weight, "word_id": word_id}


def times(fn, warmup, iters):
    ts = []
    for it in range(warmup + iters):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.percentile(ts, 50)), float(np.percentile(ts, 95))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from rover_slam_amd import capi
    import bow_ref as B
    import stamp
    ctx = capi.Context(0)
    rng = np.random.default_rng(1)
    ok = True
    print("# Device-resident ComputeBoW3 and keyframe-database scores\n")
    sp = os.path.join(ROOT, ".build_stamp.json")                  # written by tools/stamp.py where the library was built
    bst = json.load(open(sp)) if os.path.exists(sp) else stamp.current()
    bst["box_so_sha256"] = stamp.so_identity()["so_sha256"]
    print(stamp.line(bst) + "\n")
    few = (max(a.warmup // 10, 1), max(a.iters // 10, 5))
    up = lambda x: ctx.alloc(max(np.ascontiguousarray(x).nbytes, 8)).upload(np.ascontiguousarray(x))   # noqa: E731

    # ---------------------------------------------------------------- transform
    v = full_vocab(rng)
    vocab = capi.BowVocab(ctx, v)
    desc = rng.standard_normal((N, D)).astype(np.float32)
    u8 = B.binarize(desc)
    ref = B.transform(v, u8, 0)
    d = up(desc)
    dt = dict(B.DTYPES, bow_n=np.int32, fv_n=np.int32)
    size = {"word": N, "node": N, "weight": N, "bow_n": 1, "bow_word": N, "bow_value": N, "fv_n": 1, "fv_node": N, "fv_offsets": N + 1, "fv_feat": N}
    o = {k: ctx.alloc(n * np.dtype(dt[k]).itemsize) for k, n in size.items()}

    def new_transform():
        ctx.bow_transform_dev(vocab, N, 0, desc_f32=d, **o)
        ctx.synchronize()
    new_transform()
    got = {k: o[k].download((n,), dt[k]) for k, n in size.items()}
    nb, nf = int(got["bow_n"][0]), int(got["fv_n"][0])
    cut = {"word": N, "node": N, "weight": N, "bow_word": nb, "bow_value": nb, "fv_node": nf, "fv_offsets": nf + 1, "fv_feat": int(got["fv_offsets"][nf])}
    good = all(np.array_equal(got[k][:n].view(np.uint8), ref[k].view(np.uint8)) for k, n in cut.items())
    ok = ok and bool(good)
    print(f"## transform: N = {N}, k = {K}, L = {L}, D = {D}, {v['n_nodes']} nodes\n")
    print(f"Check against the restatement (every output, float64 bit for bit): {'pass' if good else 'FAIL'}.  {nb} words, {nf} nodes in the "
          f"feature vector at levelsup 0.  {a.warmup} warm-up + {a.iters} timed calls; times in microseconds.\n")
    rows = {"new": [], "host": []}
    for rep in range(2):
        rows["new"].append(times(new_transform, a.warmup, a.iters))
        rows["host"].append(times(lambda: B.transform(v, B.binarize(desc), 0), *few))
    print("| route | p50, call + synchronise (two runs) | p95 (two runs) |")
    print("|---|---:|---:|")
    print(f"| `rfe_bow_transform_dev`, descriptors resident | {rows['new'][0][0]:.1f} / {rows['new'][1][0]:.1f} | {rows['new'][0][1]:.1f} / {rows['new'][1][1]:.1f} |")
    print(f"| the numpy restatement on the host | {rows['host'][0][0]:.0f} / {rows['host'][1][0]:.0f} | {rows['host'][0][1]:.0f} / {rows['host'][1][1]:.0f} |")
    ctx.profile(True); ctx.profile_reset()
    for _ in range(a.iters):
        new_transform()
    prof = ctx.profile_read()
    ctx.profile(False); ctx.profile_reset()
    print("\n| profile stage | mean per call |")
    print("|---|---:|")
    for name in ("bow_descend", "bow_build"):
        ms, calls = prof[name]
        print(f"| `{name}` | {ms / calls * 1e3:.1f} |")
    rows_read = N * L * K
    print(f"\nNode rows read per call: {rows_read} x {D} B = {rows_read * D / 1e6:.1f} MB (the top levels out of cache, the leaves' parents mostly not: "
          f"{K ** (L - 1)} nodes at depth {L - 1}).\n")
    for b in [d] + list(o.values()):
        b.free()
    vocab.close()

    # ---------------------------------------------------------------- query
    pool = rng.choice(K ** L, 20000, replace=False)

    def vector():
        w = np.sort(rng.choice(pool, int(rng.integers(600, 1001)), replace=False)).astype(np.int32)
        x = rng.random(len(w)) + 1e-3
        return w, x / B.sequential_sum(x)
    db = capi.BowDatabase(ctx)
    entries = []
    qw, qx = vector()
    dq = (up(qw), up(qx))
    for E in (1000, 10000):
        while len(entries) < E:
            entries.append(vector())
            db.add(*entries[-1])
        score0 = np.full((E,), -1.0)
        ref = B.db_query(entries, qw, qx, None, score0)
        o = {"common": ctx.alloc(4 * E), "scored": ctx.alloc(E), "score": up(score0), "stats": ctx.alloc(16)}

        def new_query():
            db.query_dev(dq[0], dq[1], len(qw), o["common"], o["scored"], o["score"], o["stats"])
            ctx.synchronize()
        new_query()
        got = {"common": o["common"].download((E,), np.int32), "scored": o["scored"].download((E,), np.uint8),
               "score": o["score"].download((E,), np.float64), "stats": o["stats"].download((4,), np.int32)}
        good = all(np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)) for k in got)
        ok = ok and bool(good)
        stored = sum(len(w) for w, _ in entries)
        print(f"## query: {E} keyframes, {stored} stored words, a query of {len(qw)} words\n")
        print(f"Check against the restatement (counts, gate, float64 scores bit for bit): {'pass' if good else 'FAIL'}.  max / min common words "
              f"{int(got['stats'][0])} / {int(got['stats'][1])}, {int(got['stats'][2])} keyframes share a word, {int(got['stats'][3])} scored.\n")
        rows = {"new": [], "host": []}
        for rep in range(2):
            rows["new"].append(times(new_query, a.warmup, a.iters))
            rows["host"].append(times(lambda: B.db_query(entries, qw, qx, None, score0), 1, 3))
        print("| route | p50, call + synchronise (two runs) | p95 (two runs) |")
        print("|---|---:|---:|")
        print(f"| `rfe_bow_db_query_dev`, query resident | {rows['new'][0][0]:.1f} / {rows['new'][1][0]:.1f} | {rows['new'][0][1]:.1f} / {rows['new'][1][1]:.1f} |")
        print(f"| the numpy restatement on the host | {rows['host'][0][0]:.0f} / {rows['host'][1][0]:.0f} | {rows['host'][0][1]:.0f} / {rows['host'][1][1]:.0f} |")
        best = min(r[0] for r in rows["new"])
        print(f"\nStored words read by the count kernel: {stored * 4 / 1e6:.1f} MB, i.e. {stored * 4 / best / 1e3:.1f} GB/s at the better p50 of the whole "
              f"call (values, 8 B per word, are read for the scored keyframes only).\n")
        for b in o.values():
            b.free()
    for b in dq:
        b.free()
    db.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
