"""GPU: the randomised sweep of the seven device-resident solver stages (PoseOptimization, OptimizeSim3, Sim3Solver,
TwoViewReconstruction, LocalBundleAdjustment, GlobalBundleAdjustemnt, OptimizeEssentialGraph) against their restatements, and the stages
the way Rover-SLAM's threads call them.  The cases come from tests/solver_sweep.py: drawn compositions of sizes on different sides of a
lane, wave, chunk or tile boundary in one call, with every option of the entries; tests/test_solver_sweep_draws.py holds the draws to
being hard.  Every case runs through the host form and the _dev form by the helpers of the stage's own tests/test_gpu_<stage>.py
(poisoned padding, guard words, sentinel fills) and every output must equal the restatement's exactly.  An assertion names the case by
the line that rebuilds it.  Times and counts: profiles/solver_sweep.md."""
import threading
import time

import numpy as np
import pytest

import solver_sweep as SW

pytestmark = pytest.mark.gpu
JOIN_LIMIT = 120.0                               # seconds for the three threads together; they take about two


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi            # not at import time: collection must not load the library in front of the modules that load torch
    c = capi.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- A. one pytest case per (stage, seed)
@pytest.mark.parametrize("seed", SW.SEEDS)
@pytest.mark.parametrize("stage", SW.STAGES)
def test_sweep(ctx, stage, seed):
    cases = SW.draw(stage, seed)
    t0 = time.perf_counter()
    for case in cases:
        SW.reference(case)
    t1 = time.perf_counter()
    for case in cases:
        SW.check(ctx, case)
    print(f"{stage} seed {seed}: {len(cases)} calls, {sum(SW.problems(c) for c in cases)} problems, restatement {t1 - t0:.2f} s, "
          f"host and dev form {time.perf_counter() - t1:.2f} s")


# ---------------------------------------------------------------- B. the stages as Rover-SLAM's threads call them
def weight(case):
    """bytes of a case's arrays"""
    d = case["a"] if "a" in case else case["c"]
    return sum(v.nbytes for v in d.values() if isinstance(v, np.ndarray))


def test_one_context_across_stages():
    """one context, one drawn case of each stage in a shuffled order, a large case, a small one, a large one ..., then the same list
    backwards: each stage finds the workspaces as six other stages left them, grown by a larger call or not"""
    from rover_slam_amd import capi
    rng = np.random.default_rng(5)
    order = [SW.STAGES[i] for i in rng.permutation(len(SW.STAGES))]
    seq = []
    for k, stage in enumerate(order):
        cases = sorted(SW.draw(stage, 3), key=weight)
        seq.append(cases[-1] if k % 2 == 0 else cases[0])
    assert all(weight(a) > weight(b) for a, b in zip(seq[0::2], seq[1::2]))
    c = capi.Context(0)
    try:
        for case in seq + seq[::-1]:
            SW.check(c, case)
    finally:
        c.close()


def thread_lists():
    """tracking: pose_opt and two_view; local mapping: local_ba; loop closing: sim3_solver, optimize_sim3, essential_graph, global_ba"""
    po, tv = SW.draw("pose_opt", 2), SW.draw("two_view", 2)
    lb = sorted(SW.draw("local_ba", 2), key=weight)
    return {"tracking": [po[0], tv[0], po[1], tv[1], po[2]],
            "local_mapping": [lb[-1], lb[0], lb[-2], lb[1], lb[-3]],
            "loop_closing": [SW.draw("sim3_solver", 2)[0], SW.draw("optimize_sim3", 2)[0], max(SW.draw("essential_graph", 2), key=weight),
                             max(SW.draw("global_ba", 2), key=weight), SW.draw("optimize_sim3", 2)[1]]}


def test_three_threads_three_contexts():
    """Tracking, LocalMapping and LoopClosing each own a context and call their stages while the others call theirs.  Run once: the
    references first, the threads only call the library (host form and _dev form of each case) and keep what comes back, the main
    thread compares after the joins"""
    from rover_slam_amd import capi
    lists = thread_lists()
    for cases in lists.values():
        assert 4 <= len(cases) <= 6
        for case in cases:
            SW.reference(case)
    ctxs = {name: capi.Context(0) for name in lists}
    barrier = threading.Barrier(len(lists))
    got = {name: [] for name in lists}

    def work(name):
        at = "the barrier"
        try:
            barrier.wait(timeout=JOIN_LIMIT)
            for case in lists[name]:
                for form, run in zip(("host", "dev"), SW.forms(ctxs[name], case)):
                    at = f"{case['tag']} [{form} form]"
                    got[name].append((case, form, run()))
        except BaseException as e:                            # kept for the main thread; the thread ends here
            got[name].append(RuntimeError(f"{at}: {e!r}"))

    threads = [threading.Thread(target=work, args=(name,), daemon=True) for name in lists]
    deadline = time.monotonic() + JOIN_LIMIT
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(deadline - time.monotonic(), 0.0))
    alive = [name for name, t in zip(lists, threads) if t.is_alive()]
    if alive:                                                 # nothing further is started: no close, no comparison
        pytest.fail(f"still running after {JOIN_LIMIT} s: {alive}")
    for c in ctxs.values():
        c.close()
    for name, results in got.items():
        for r in results:
            if isinstance(r, BaseException):
                raise AssertionError(f"thread {name}: {r!r}") from r
        assert len(results) == 2 * len(lists[name]), name
        for case, form, out in results:
            SW.compare(case, out, SW.reference(case), f"{form}, thread {name}")
