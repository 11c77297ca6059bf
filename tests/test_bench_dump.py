"""CPU: bench.py --dump-outputs writer.  Results as float32 / float64 .npy files, entries past a frame's keypoint count or a pair's
match count zeroed, 64 MB in all at most (a fixed, seeded row sample of the largest arrays beyond that), the same files for the same input."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _outputs(B, K=1024, seed=1):
    rng = np.random.default_rng(seed)
    return {"n": rng.integers(500, K + 1, B).astype(np.int32), "kxy": rng.integers(1, 600, (B, K, 2)).astype(np.int32),
            "score": rng.random((B, K), np.float32) + 1, "desc": rng.random((B, K, 256), np.float32) + 1,
            "S": rng.integers(0, 300, B - 1).astype(np.int32), "pairs": rng.integers(1, K, (B - 1, K, 2)).astype(np.int32),
            "ms": rng.random((B - 1, K), np.float32) + 1}


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_bench_batch_written_whole_and_masked(tmp_path):
    arr = _outputs(33)
    keep = {k: v.copy() for k, v in arr.items()}
    r = bench.dump_outputs(str(tmp_path), arr, n=arr["n"], S=arr["S"])
    got = _files(tmp_path)
    assert set(got) == set(arr) and sorted(r["files"]) == sorted(k + ".npy" for k in arr)
    assert all(np.array_equal(arr[k], keep[k]) for k in arr)                     # the caller's arrays are not touched
    for k, v in got.items():
        assert v.dtype == (np.float32 if arr[k].dtype.kind == "f" else np.float64) and v.shape == arr[k].shape, k
    n, S = arr["n"], arr["S"]
    for i in range(33):
        for k in ("kxy", "score", "desc"):
            assert np.array_equal(got[k][i, :n[i]], arr[k][i, :n[i]]) and not got[k][i, n[i]:].any(), k
    for q in range(32):
        for k in ("pairs", "ms"):
            assert np.array_equal(got[k][q, :S[q]], arr[k][q, :S[q]]) and not got[k][q, S[q]:].any(), k
    assert np.array_equal(got["n"], n) and np.array_equal(got["S"], S)


def test_large_batch_sampled_within_64_mb_and_repeatable(tmp_path):
    arr = _outputs(80)                                                            # 80 frames: 84 MB of descriptors alone
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arr, n=arr["n"], S=arr["S"])
    bench.dump_outputs(str(b), arr, n=arr["n"], S=arr["S"])
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 10 ** 6
    ga, gb = _files(a), _files(b)
    assert set(ga) == set(arr) | {"desc_rows"} and all(np.array_equal(ga[k], gb[k]) for k in ga)
    rows = ga["desc_rows"].astype(np.int64)
    assert len(rows) > 50000 and np.all(np.diff(rows) > 0)
    flat = arr["desc"].reshape(-1, 256) * (np.arange(1024)[None, :] < arr["n"][:, None]).reshape(-1, 1)
    assert np.array_equal(ga["desc"], flat[rows])
    assert ga["kxy"].shape == (80, 1024, 2)                                      # the small arrays stay whole
