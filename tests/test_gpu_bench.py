"""GPU: bench.py's own contract on the box the driver uses -- one JSON line with the fields the task statement names, and
the N-rank flow (bench.py --gpus 2 spawning two ranks that share the one GPU over gloo: a functional check of sharding,
rank census and the ONE-gather result path; RCCL itself needs N GPUs and is exercised by the driver's scaling run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=e, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:      # the reason lives in the JSON line on stdout (invalid / invalid_aux / *.error), not only on stderr
        why = {}
        try:
            d = json.loads(r.stdout.strip().splitlines()[-1])
            why = {k: d[k] for k in ("invalid", "invalid_aux", "perf_notes") if k in d}
            for sect in ("variants", "latency", "pool_c_abi", "pcie_inclusive"):
                v = d.get(sect)
                if isinstance(v, dict):
                    errs = {k: x["error"] for k, x in v.items() if isinstance(x, dict) and "error" in x}
                    if "error" in v and isinstance(v["error"], str):
                        errs["error"] = v["error"]
                    if errs:
                        why[sect + ".errors"] = errs
        except (ValueError, IndexError):
            why = {"stdout_tail": r.stdout[-1500:]}
        pytest.fail(f"bench.py {' '.join(argv)} exited {r.returncode}\nline says: {json.dumps(why, indent=1)[:3000]}\nstderr tail:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_line_contract_single_gpu():
    d = _bench("--full", "--steps", "3", "--warmup", "1", "--sustained-steps", "20", "--no-cpu-baseline")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "sustained"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["scaling"] == "weak" and d["dtype"] == "f32" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0.3 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3          # 32 frames per step per GPU
    s = d["sustained"]
    assert s["steps"] == 20 and s["ms_per_step"]["min"] <= s["ms_per_step"]["mean"] <= s["ms_per_step"]["max"]


def test_bench_gpus2_over_gloo_on_one_gpu():
    d = _bench("--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--sustained-steps", "0", env={"RFE_BENCH_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and "child processes" in d["launcher"]
    assert d["rccl"]["world_size"] == 2 and d["rccl"]["allreduce_sum_of_ones"] == 2 and len(d["rccl"]["devices"]) == 2
    assert d["gather"]["collectives_per_step"] == 1 and d["gather"]["last_step_payload_verified"] is True
    assert len(d["per_rank_ms_per_step"]["all"]) == 2 and isinstance(d["per_rank_ms_per_step"]["outlier"], bool)
    assert d["rccl"]["untimed_collective_warmup_rounds"] >= 3          # whatever --warmup says, the timed region never holds the group's first collectives
    assert abs(d["value"] - 2 * 32 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3      # whole-job frames over the max-over-ranks time


def test_bench_rccl_code_path_at_world_size_one():
    """RCCL needs one GPU per rank, so the N-rank run belongs to the driver's 8-GPU box; what CAN run here is the same code path
    at world size 1 (RFE_BENCH_FORCE_PG=1): process group on the "nccl" backend bound to the device, object all-gather, device
    all-reduce, barrier-bracketed timing and the per-step dist.gather of the packed results into the preallocated buffer."""
    d = _bench("--full", "--steps", "2", "--warmup", "1", "--sustained-steps", "4", "--no-cpu-baseline", "--no-pcie", env={"RFE_BENCH_FORCE_PG": "1"})
    assert d["n_gpus"] == 1 and d["rccl"]["backend"] == "nccl" and d["rccl"]["world_size"] == 1 and d["rccl"]["allreduce_sum_of_ones"] == 1
    assert d["gather"]["collectives_per_step"] == 1 and d["gather"]["last_step_payload_verified"] is True
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    assert d["rccl"]["untimed_collective_warmup_rounds"] >= 3          # the timed region never holds a communicator's first collectives
    assert "r04_pairing_step_time_ratio" not in d.get("perf_notes", {})  # no step-time comparison against a loop that holds collectives


def test_bench_plain_line_and_outputs(tmp_path):
    """A plain run (no --full): the headline fields only, `steps` timed steps, and --dump-outputs writes the last timed step's results as
    float32 / float64 .npy files within 64 MB, zero past every frame's keypoint count and every pair's match count"""
    out = tmp_path / "outputs"
    d = _bench("--steps", "4", "--warmup", "1", "--dump-outputs", str(out))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
        assert k in d, k
    assert d["steps"] == 4 and d["dtype"] == "f32" and d["higher_is_better"] is True and d["unit"] == "frames/s"
    for k in ("roofline", "stages", "sustained", "variants", "pcie_inclusive", "pool_c_abi", "latency", "cpu_baseline"):
        assert k not in d, k
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
    a = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(a) == {"n", "kxy", "score", "desc", "S", "pairs", "ms"} and sorted(d["dump_outputs"]["files"]) == sorted(f + ".npy" for f in a)
    assert sum(os.path.getsize(out / (f + ".npy")) for f in a) <= 64 * 10 ** 6
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["n"].shape == (33,) and a["desc"].shape == (33, 1024, 256) and a["S"].shape == (32,) and a["pairs"].shape == (32, 1024, 2)
    n, S = a["n"].astype(int), a["S"].astype(int)
    assert (n > 0).all() and (n <= 1024).all() and S.sum() > 0
    for i in range(33):
        assert not a["desc"][i, n[i]:].any() and not a["kxy"][i, n[i]:].any() and np.isfinite(a["desc"][i, :n[i]]).all()
    for q in range(32):
        assert not a["pairs"][q, S[q]:].any() and not a["ms"][q, S[q]:].any() and (a["ms"][q, :S[q]] > 0.1).all()
