"""CPU: the restatement of SearchByProjection1 that the GPU tests compare against (tests/projection_search_ref.py) holds its
own definitions -- candidate lists against a brute-force statement, the parallel (fixpoint) form against the sequential loop -- the
contention case is not vacuous, and the drop-in header compiles and links."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import projection_search_ref as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2)
_cache = {}


def solved(oracle, seed):
    """case, lists, sequential result, Jacobi result and rounds of one seed, computed once per session"""
    if seed not in _cache:
        c = PS.make_case(seed)
        lists = PS.case_lists(c)
        seq = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists, c["skip"], c["observed"])
        jac, rounds = PS.search_by_projection_jacobi(oracle, c["q"], c["desc"], lists, c["skip"], c["observed"])
        _cache[seed] = (c, lists, seq, jac, rounds)
    return _cache[seed]


def test_round_is_half_away_from_zero():
    got = [float(PS.round_half_away(v)) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, 2.4999998, 31.5)]
    assert got == [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, 2.0, 32.0]


def brute_force(c, octave, pred_level, i):
    """the definition: in-grid features that pass the level gate and both strict window tests, ordered by (cell x, cell y, index)"""
    cell = PS.cells(c["kpts"], c["bounds"])
    px, py, r = c["proj"][i, 0], c["proj"][i, 1], c["radius"][i]
    L = 0 if pred_level is None else int(pred_level[i])
    keep = []
    for j in range(len(c["kpts"])):
        o = 0 if octave is None else int(octave[j])
        if cell[j, 0] < 0 or o < L - 1 or o > L:
            continue
        if abs(np.float32(c["kpts"][j, 0] - px)) < r and abs(np.float32(c["kpts"][j, 1] - py)) < r:
            keep.append((cell[j, 0], cell[j, 1], j))
    return [j for _, _, j in sorted(keep)]


@pytest.mark.parametrize("seed", SEEDS)
def test_candidate_lists_equal_brute_force(seed):
    c = PS.make_case(seed)
    rng = np.random.default_rng(100 + seed)
    for octave, level in ((None, None), (rng.integers(0, 3, len(c["kpts"])), rng.integers(0, 3, len(c["proj"])))):
        lists = PS.case_lists(c, octave, level)
        assert sum(len(l) for l in lists) > len(lists)
        for i, l in enumerate(lists):
            assert l == brute_force(c, octave, level, i), i
    # the visiting order is not the index order: some list is not ascending
    assert any(l != sorted(l) for l in PS.case_lists(c))


def test_window_edges():
    c = PS.make_case(0)
    grid = PS.build_grid(c["kpts"], c["bounds"])
    area = lambda px, py, r: PS.features_in_area(grid, c["kpts"], None, c["bounds"], px, py, r, 0)   # noqa: E731
    assert area(-500.0, 60.0, 12.0) == [] and area(80.0, 900.0, 12.0) == [] and area(1e30, 1e30, 5.0) == []
    assert area(np.nan, 60.0, 12.0) == [] and area(80.0, 60.0, np.inf) == [] and area(80.0, 60.0, 0.0) == [] and area(80.0, 60.0, -3.0) == []
    everything = area(80.0, 60.0, 1000.0)
    cell = PS.cells(c["kpts"], c["bounds"])
    assert sorted(everything) == [j for j in range(len(cell)) if cell[j, 0] >= 0] and len(everything) < len(cell)
    x, y = c["kpts"][everything[0]]
    assert everything[0] in area(x + 2.0, y, 2.5) and everything[0] not in area(x + 2.5, y, 2.5)     # the window test is strict


@pytest.mark.parametrize("seed", SEEDS)
def test_jacobi_equals_sequential(oracle, seed):
    _, _, seq, jac, rounds = solved(oracle, seed)
    for k in ("best_idx", "best_dist", "second_dist", "assign"):
        assert np.array_equal(seq[k], jac[k]), k
    assert seq["nmatches"] == jac["nmatches"] > 0
    assert rounds <= len(seq["best_idx"]) + 1


@pytest.mark.parametrize("seed", SEEDS)
def test_case_is_not_vacuous(oracle, seed):
    c, lists, seq, _, rounds = solved(oracle, seed)
    v = PS.vacuity(oracle, c, lists, seq, rounds)
    print(f"seed {seed}: {v}, nmatches {seq['nmatches']}")
    PS.check_vacuity(v, len(lists))


def test_chain_needs_one_round_per_map_point(oracle):
    """80 identical map points on 64 features at distinct distances: map point i gets the i-th nearest, the rest nothing"""
    c = chain_case()
    lists = PS.candidate_lists(c["kpts"], None, c["bounds"], c["proj"], c["radius"])
    assert all(len(l) == 64 for l in lists)
    seq = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists)
    jac, rounds = PS.search_by_projection_jacobi(oracle, c["q"], c["desc"], lists)
    assert np.array_equal(seq["best_idx"][:64], c["order"]) and (seq["best_idx"][64:] == -1).all() and (seq["best_dist"][64:] == 256).all()
    assert (seq["best_dist"][:64] <= PS.TH_HIGH).all() and seq["nmatches"] == 64
    for k in ("best_idx", "best_dist", "second_dist", "assign"):
        assert np.array_equal(seq[k], jac[k]), k
    assert rounds >= 64


def chain_case():
    """64 features on an 8 x 8 block of pixels inside one window, feature j at distance (1 + rank_j) * 0.01 of the one query descriptor"""
    rng = np.random.default_rng(5)
    e = np.zeros((2, 256), np.float32); e[0, 0] = 1; e[1, 1] = 1
    rank = rng.permutation(64)
    desc = np.zeros((64, 256), np.float32)
    desc[:, 0] = 1
    desc[:, 1] = (1 + rank) * np.float32(0.01)
    kxy = np.stack([76 + np.arange(64) % 8, 56 + np.arange(64) // 8], 1).astype(np.int32)
    return {"bounds": (0.0, 0.0, 160.0, 120.0), "kxy": kxy, "kpts": kxy.astype(np.float32), "desc": desc,
            "q": np.ascontiguousarray(np.repeat(e[:1], 80, axis=0)), "proj": np.tile(np.float32([79.5, 59.5]), (80, 1)),
            "radius": np.full((80,), 12, np.float32), "order": np.argsort(rank).astype(np.int32)}


def write_driver_case(path, c, th=3.0, nleft=-1):
    """the seed case as tests/cpp/projection_search_driver.cpp reads it: every fifth vpMapPoints entry is one the filters of
    SPmatcher.cc:1178-1190 drop (not in view / far / bad), skip becomes a prior map point WITH observations, and every tenth other
    feature gets a prior map point WITHOUT observations (not blocked, overwritten when matched).  Returns sel: vpMapPoints index of
    every map point of the case."""
    Nq, Nf = len(c["proj"]), len(c["kpts"])
    sel, inview, bad, depth = [], [], [], []
    for i in range(Nq):
        if i % 4 == 0:
            kind = (i // 4) % 3
            inview.append(0 if kind == 0 else 1); bad.append(1 if kind == 1 else 0); depth.append(99.0 if kind == 2 else 1.0)
        sel.append(len(inview)); inview.append(1); bad.append(0); depth.append(1.0)
    Nm = len(inview)
    sel = np.array(sel)

    def full(v, fill, dt):
        a = np.full((Nm,) + np.shape(v)[1:], fill, dt)
        a[sel] = v
        return a
    vcos = np.where(c["radius"] == np.float32(2.5 * th), np.float32(0.999), np.float32(0.9)).astype(np.float32)
    assert np.array_equal(np.where(vcos > 0.998, np.float32(2.5), np.float32(4.0)) * np.float32(th), c["radius"])
    prior = np.where(c["skip"] != 0, 3, -1).astype(np.int32)
    free = np.flatnonzero(c["skip"] == 0)[::10]
    prior[free] = 0
    with open(path, "wb") as f:
        np.array([Nm, Nf, nleft], np.int32).tofile(f); np.array([th], np.float32).tofile(f); np.array([1], np.int32).tofile(f)
        np.array([50.0, *c["bounds"], 1.0], np.float32).tofile(f)
        np.array(inview, np.uint8).tofile(f); np.array(bad, np.uint8).tofile(f)
        full(c["observed"].astype(np.int32) * 2, 1, np.int32).tofile(f)
        np.array(depth, np.float32).tofile(f)
        full(vcos, 0.9, np.float32).tofile(f)
        full(c["proj"], 80.0, np.float32).tofile(f)
        full(c["q"], 0.0625, np.float32).tofile(f)
        c["kpts"].astype(np.float32).tofile(f); np.zeros((Nf,), np.int32).tofile(f); prior.tofile(f); c["desc"].astype(np.float32).tofile(f)
    return sel, prior


def build_driver(tmp_path):
    exe = str(tmp_path / "projection_search_driver")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "projection_search_driver.cpp"), "-o", exe,
           "-L" + os.path.join(ROOT, "rover-slam_amd"), "-lrover_fe", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + os.path.join(ROOT, "rover-slam_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_header_compiles_and_links(tmp_path):
    exe = build_driver(tmp_path)
    assert subprocess.run([exe]).returncode == 0             # no arguments: nothing touches a device
