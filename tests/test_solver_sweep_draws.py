"""CPU, restatement only: the randomised solver sweep (tests/solver_sweep.py, run on the device by test_gpu_solver_sweep.py) must not
pass because its draws are tame.  Over the four seeds of each stage: every value of the stage's size list occurs, a batched stage has a
call past its chunk size, the RANSAC and single-pose stages end in their success exit for at least a third of the problems and in another
exit at least once, the graph stages accept an LM step in at least half of their cases and reject a trial at least once, and no case is
outside the entry's caps.  These are conditions on the draw rules: where one fails, the weights of the draw change, never the condition,
and the draw stays a pure function of (stage, seed)."""
import numpy as np
import pytest

import essential_graph_ref as EG
import global_ba_ref as GB
import local_ba_ref as LB
import solver_sweep as SW

BATCHED = ("pose_opt", "optimize_sim3", "sim3_solver", "two_view")
GRAPH = ("local_ba", "global_ba", "essential_graph")


def all_cases(stage):
    return [c for seed in SW.SEEDS for c in SW.draw(stage, seed)]


def covered(values, drawn, what):
    for v in values:
        hit = any(v[0] <= d <= v[1] for d in drawn) if isinstance(v, tuple) else v in drawn
        assert hit, f"{what}: {v} is never drawn"


def problem_sizes(stage, case):
    if stage == "pose_opt":
        return [len(s["kpts"]) for s in case["scenes"]]
    if stage in ("optimize_sim3", "sim3_solver"):
        return [s["P"]["n"] for s in case["scenes"]]
    return [s["S"] for s in case["scenes"]]


def test_the_draw_is_a_function_of_stage_and_seed():
    for stage in SW.STAGES:
        a = SW.draw(stage, 1)
        SW._DRAWN.pop((stage, 1, None))
        b = SW.draw(stage, 1)
        assert a is not b and [c["tag"] for c in a] == [c["tag"] for c in b]
        assert len({c["tag"] for seed in SW.SEEDS for c in SW.draw(stage, seed)}) == len(SW.SEEDS) * SW.CALLS[stage]
        for x, y in zip(a, b):
            for k in ("a", "c"):
                if k in x:
                    assert all(np.array_equal(x[k][n], y[k][n], equal_nan=True) for n in x[k] if isinstance(x[k][n], np.ndarray))


@pytest.mark.parametrize("stage", BATCHED)
def test_batched_stage(stage):
    cases = all_cases(stage)
    sizes = [n for c in cases for n in problem_sizes(stage, c)]
    covered(SW.SIZES[stage], sizes, stage)
    Bs = [SW.problems(c) for c in cases]
    assert min(Bs) >= 1 and max(Bs) <= SW.MAX_B[stage]
    if stage == "optimize_sim3":                      # one, two and three launches, the last chunk partial
        assert any(B <= 8 for B in Bs) and any(8 < B < 16 for B in Bs) and any(16 < B < 24 for B in Bs)
    elif stage == "sim3_solver":
        assert any(B <= 16 for B in Bs) and any(B > 16 for B in Bs)
    else:                                             # one launch whatever B: both ends of the range
        assert any(B <= 2 for B in Bs) and any(B >= SW.FIRST_B[stage][0][0] for B in Bs)
    done = [ok for c in cases for ok in SW.outcomes(c)]
    assert len(done) == len(sizes)
    print(f"{stage}: {len(cases)} calls, {len(done)} problems, {sum(done)} end in the success exit")
    assert 3 * sum(done) >= len(done) and sum(done) < len(done)


def test_batched_caps_and_options():
    """what rover_fe.h caps: N, N2, N1max, N2max, Kmax <= 4096, H <= 1024, its <= H; and the options of the table all occur"""
    for stage in BATCHED:
        for c in all_cases(stage):
            a = c["a"]
            for k in ("kpts", "kpts1", "kpts2", "xw1", "pairs"):
                assert k not in a or a[k].shape[1] <= 4096
            if "draws" in a:
                its = [200 if s["P"]["its"] == 0 else s["P"]["its"] for s in c["scenes"]]
                assert a["draws"].shape[1] <= 1024 and max(its) <= a["draws"].shape[1] and min(its) >= 1
    po = all_cases("pose_opt")
    assert {c["octave"] for c in po} == {c["uright"] for c in po} == {True, False}
    assert any(c["N"] == max(problem_sizes("pose_opt", c)) for c in po) and any(c["N"] > max(problem_sizes("pose_opt", c)) + 20 for c in po)
    assert {tuple(s["uright"].tolist()) == () or bool((s["uright"] >= 0).any()) for c in po for s in c["scenes"]} == {True, False}
    assert any(c["P"]["iterations"] == (0, 0, 0, 0) for c in po) and any(min(c["P"]["iterations"]) >= 1 for c in po)
    assert {c["P"]["max_trials"] for c in po} == {0, 1, 2, 3}
    osim = [s for c in all_cases("optimize_sim3") for s in c["scenes"]]
    assert {(s["P"]["fix_scale"], s["P"]["all_points"]) for s in osim} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any((s["idx2"][:s["P"]["n"]] < 0).any() for s in osim) and {s["P"]["max_trials"] for s in osim} == {0, 1, 2}
    for c in all_cases("optimize_sim3"):
        n = max(problem_sizes("optimize_sim3", c))
        assert len({n, c["N"], c["N2"]}) == 3
    s3 = [s for c in all_cases("sim3_solver") for s in c["scenes"]]
    its = [s["P"]["its"] for s in s3]
    assert its.count(300) == len(SW.SEEDS) and min(its) >= 1 and max(i for i in its if i != 300) <= 40 and len(set(its)) > 20
    assert {s["P"]["fix_scale"] for s in s3} == {0, 1}
    assert any(s["P"]["min_inliers"] == s["P"]["n"] >= 63 for s in s3) and any(s["P"]["min_inliers"] == 3 < s["P"]["n"] for s in s3)
    tv = [s for c in all_cases("two_view") for s in c["scenes"]]
    its = [s["P"]["its"] for s in tv]
    assert its.count(0) == len(SW.SEEDS) and max(its) <= 24 and len(set(its)) > 15
    assert all(len({s["S"], s["P"]["n1"], s["P"]["n2"]}) == 3 for s in tv) and {s["P"]["sigma"] for s in tv} == {0.0, 1.0, 1.5}
    assert len({c["pad"] for c in all_cases("two_view")}) > 12


def test_two_view_kinds_and_exits():
    import two_view_ref as TV
    kinds, exits = set(), set()
    for c in all_cases("two_view"):
        kinds |= {s["P"]["rh_threshold"] for s in c["scenes"]}
        exits |= {int(r[11]) for r in SW.reference(c)["stats"]}
        assert not SW.reference(c)["stats"][:, 12].any()          # no refused-looking problem: no flag is set
    assert len(kinds) >= 3 and {TV.EXIT_OK, TV.EXIT_NO_WINNER, TV.EXIT_PARALLAX} <= exits, (kinds, exits)
    tags = " ".join(c["tag"] for c in all_cases("two_view"))
    assert all(f"'{k}'" in tags for k in SW.TV_KINDS)


@pytest.mark.parametrize("stage", GRAPH)
def test_graph_stage(stage):
    cases = all_cases(stage)
    steps = [SW.steps(c) for c in cases]              # the restatement refuses (Invalid) what the entry refuses: no case is one
    print(f"{stage}: {len(cases)} cases, (accepted, rejected) {steps}")
    assert 2 * sum(1 for a, _ in steps if a >= 1) >= len(cases)
    assert any(r >= 1 for _, r in steps)
    if stage == "local_ba":
        covered(SW.SIZES["local_ba.P"], [c["c"]["P"] for c in cases], "local_ba P")
        covered(SW.SIZES["local_ba.L"], [len(c["c"]["xw"]) for c in cases], "local_ba L")
        for c in cases:
            c = c["c"]
            assert 0 <= c["P"] <= LB.MAX_FREE and 0 <= c["F"] <= 5 and c["P"] + c["F"] >= 1 and 1 <= c["params"]["iterations"] <= 4
            assert len(c["xw"]) <= LB.MAX_POINTS and len(c["edge_point"]) <= LB.MAX_EDGES
        assert {c["c"]["F"] for c in cases} >= {0, 1, 5} and {c["c"]["params"]["max_trials"] for c in cases} == {0, 1, 2}
        tags = " ".join(c["tag"] for c in cases)
        assert all(f"kind={k}" in tags for k in ("mono", "stereo", "mixed")) and "all_see=True" in tags and "gross=0.0" in tags and "gross=0.2" in tags
    elif stage == "global_ba":
        tags = " ".join(c["tag"] for c in cases)
        assert all(f"pattern={n} " in tags for n in SW.GB_PATTERNS) and "ring=True" in tags and "ring=False" in tags
        K = [len(c["c"]["fixed"]) for c in cases]
        covered([v for v in SW.SIZES["global_ba"] if v not in (2, 3)], K, "global_ba K")         # pairs5 lifts a 2 or 3 to 5
        free = [int((c["c"]["fixed"] == 0).sum()) for c in cases]
        nfix = {int(c["c"]["fixed"].sum()) for c in cases}
        assert min(K) >= 2 and max(K) <= 70 and min(K) <= 8 and max(free) > LB.MAX_FREE and nfix == {0, 1, 2, 3}
        # the kernels tile four poses a side: one short of a tile edge, on it and one past it, with a random fixed set in the middle of the indices
        assert {f % GB.TILE_V for f in free} >= {GB.TILE_V - 1, 0, 1}
        assert any(c["c"]["fixed"][0] == 0 and c["c"]["fixed"].any() for c in cases)
        assert {c["c"]["params"]["robust"] for c in cases} == {True, False} and {c["c"]["params"]["iterations"] for c in cases} == {1, 2, 3, 4}
        assert all(len(c["c"]["xw"]) <= GB.MAX_POINTS and len(c["c"]["edge_point"]) <= GB.MAX_EDGES and GB.schur_pairs(c["c"]) <= GB.MAX_PAIRS for c in cases)
    else:
        tags = " ".join(c["tag"] for c in cases)
        N = [len(c["c"]["fixed"]) for c in cases]
        covered(SW.SIZES["essential_graph"], N, "essential_graph N")
        assert min(N) == 1 and max(N) <= 40 and max(N) > 4 * EG.TILE_V and {len(c["c"]["point_ref"]) for c in cases} == {0, 1, 257}
        assert all(f"kind={k} " in tags for k in SW.EG_KINDS) and all(f"{k}={v} " in tags for k in ("shuffle", "fix_scale") for v in (True, False))
        assert "fixed=None" in tags and "fixed=0 " in tags and "band=0 " in tags and "band=4 " in tags and "dup=0 " in tags and "corrected=3 " in tags
        assert any(c["c"]["edge_from_est"].any() for c in cases) and any(not c["c"]["edge_from_est"].any() for c in cases)
        free = {int((c["c"]["fixed"] == 0).sum()) % EG.TILE_V for c in cases}
        assert free >= {EG.TILE_V - 1, 0, 1}
        assert all(len(c["c"]["edge_i"]) <= EG.MAX_EDGES and 0 <= c["P"]["iterations"] <= EG.MAX_ITERATIONS for c in cases)
