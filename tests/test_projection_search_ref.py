"""CPU: the restatement of SearchByProjection1 that the GPU tests compare against (tests/projection_search_ref.py) holds its
own definitions -- candidate lists against a brute-force statement, the parallel (fixpoint) form against the sequential loop -- the
contention case is not vacuous."""
import numpy as np
import pytest

import projection_search_ref as PS

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


def chain_1024_case():
    """chain_case() behind 1000 map points whose lists are empty: the 64 links of the chain are map points 1000..1063, so in the resolve
    kernel every blocker up to map point 1023 belongs to another trip of the 1024-thread loop than the map points it blocks from 1024 on"""
    c = chain_case()
    n = 1000
    return dict(c, q=np.ascontiguousarray(np.concatenate([np.repeat(c["q"][:1], n, axis=0), c["q"]])),
                proj=np.ascontiguousarray(np.concatenate([np.tile(np.float32([5.0, 5.0]), (n, 1)), c["proj"]])),
                radius=np.concatenate([np.full((n,), 2, np.float32), c["radius"]]))


# ---------------------------------------------------------------- past one pass of the 1024-thread loops ("Sizes covered")
PS_INFLIGHT = 8                 # proj_search.hip: candidate rows in flight per wave
BIG = {"A": dict(seed=0, Nf=1100, Nq=1100),       # a second trip of every 1024-stride loop; two map points per count thread, threads >= 550 idle
       "B": dict(seed=2, Nf=4093, Nq=2500),       # Nf odd and just under the limit; three per count thread, a partial last owner; off_origin
       "C": dict(seed=1, Nf=4096, Nq=16384)}      # both documented limits: sixteen per count thread, pick[] / minw[] / cell[] full


def big_case(name, moved=True):
    a = BIG[name]
    c = PS.make_case(a["seed"], W=640, H=480, Nf=a["Nf"], Nq=a["Nq"], src_hi=a["Nf"])
    return PS.off_origin(c, 202) if name == "B" and moved else c


def solved_big(oracle, name):
    """solved() for the cases of BIG; "chain-1024" gives (case, lists, sequential, Jacobi, rounds) of chain_1024_case()"""
    if name not in _cache:
        c = chain_1024_case() if name == "chain-1024" else big_case(name)
        lists = PS.case_lists(c)
        seq = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists, c.get("skip"), c.get("observed"))
        jac, rounds = PS.search_by_projection_jacobi(oracle, c["q"], c["desc"], lists, c.get("skip"), c.get("observed"))
        _cache[name] = (c, lists, seq, jac, rounds)
    return _cache[name]


def solved_levels(oracle):
    """B's geometry before off_origin with octaves and predicted levels: case, octave, level, gated lists, ungated lists, sequential result"""
    if "B-levels" not in _cache:
        c = big_case("B", moved=False)
        rng = np.random.default_rng(33)
        octave = rng.integers(0, 3, len(c["kpts"])).astype(np.int32)
        level = rng.integers(0, 3, len(c["proj"])).astype(np.int32)
        lists = PS.case_lists(c, octave, level)
        seq = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists, c["skip"], c["observed"])
        _cache["B-levels"] = (c, octave, level, lists, PS.case_lists(c), seq)
    return _cache["B-levels"]


@pytest.mark.parametrize("name", tuple(BIG))
def test_big_case_is_not_vacuous_and_jacobi_equals_sequential(oracle, name):
    c, lists, seq, jac, rounds = solved_big(oracle, name)
    v = PS.vacuity(oracle, c, lists, seq, rounds)
    print(f"{name}: {v}, nmatches {seq['nmatches']}, candidates {sum(len(l) for l in lists)}")
    PS.check_vacuity(v, len(lists))
    for k in ("best_idx", "best_dist", "second_dist", "assign"):
        assert np.array_equal(seq[k], jac[k]), k
    assert seq["nmatches"] == jac["nmatches"] > 0
    # the second trip of the 1024-stride loops carries results, not only work
    assert (np.flatnonzero(seq["assign"] >= 0) >= 1024).any()                       # pick[] holds a feature index >= 1024
    assert (seq["best_dist"][1024:] <= PS.TH_HIGH).any()                           # a map point >= 1024 is accepted
    if name != "A":
        assert max(len(l) for l in lists) > PS_INFLIGHT                            # proj_fill_kernel takes a second batch of rows


def test_off_origin_case_rounds_on_both_sides(oracle):
    c, lists, _, _, _ = solved_big(oracle, "B")
    Nf = len(c["kpts"])
    assert "kxy" not in c and c["bounds"][0] < 0 and c["bounds"][1] < 0
    assert (c["kpts"] != np.round(c["kpts"])).any()                                 # sub-pixel
    cell = PS.cells(c["kpts"], c["bounds"])
    member = np.bincount(np.array([j for l in lists for j in l], np.int64), minlength=Nf)
    for j, xy in zip(range(Nf - 5, Nf), PS.PLANTED):
        assert tuple(c["kpts"][j]) == xy
        if xy in PS.PLANTED_OUT:                                                    # round(-0.5) = -1: in no cell, in no list
            assert cell[j, 0] < 0 and member[j] == 0, (j, xy)
        else:                                                                       # round(-0.4875) = -0: cell 0 on that axis
            assert cell[j, 0] >= 0 and 0 in cell[j] and member[j] >= 1, (j, xy, cell[j], member[j])
    # half-to-even would have put the outside ones into cell 0 of the windows that look at them
    for i, (px, py) in zip(range(len(lists) - 3, len(lists)), PS.PLANTED_PROJ):
        assert tuple(c["proj"][i]) == (px, py) and c["radius"][i] == 12 and len(lists[i]) >= 1
    near = lambda j, i: (abs(c["kpts"][j] - c["proj"][i]) < c["radius"][i]).all()   # noqa: E731
    assert near(Nf - 5, len(lists) - 3) and near(Nf - 3, len(lists) - 2)            # the window test alone would keep them
    half = PS.on_half(c["kpts"], c["bounds"])
    print(f"B: {int(half.sum())} features on an exact half, {int((half & (member > 0)).sum())} of them in a list; planted in lists {member[-5:]}")
    assert (half & (member > 0) & (cell[:, 0] >= 0)).sum() >= 1
    # and for some of them the two roundings give different cells: the scaled coordinate is k + 0.5 with k even
    sx = (c["kpts"][:, 0] - np.float32(c["bounds"][0])) * np.float32(0.05)
    assert ((np.abs(sx - np.trunc(sx)) == 0.5) & (np.trunc(sx) % 2 == 0) & (member > 0)).any()


def test_big_candidate_lists_equal_brute_force(oracle):
    c, lists, _, _, _ = solved_big(oracle, "B")
    cl, octave, level, gated, _, _ = solved_levels(oracle)
    for case, oc, lv, ls, seed in ((c, None, None, lists, 7), (cl, octave, level, gated, 8)):
        cell = PS.cells(case["kpts"], case["bounds"])              # once per case, not per map point
        Nq = len(ls)
        sample = np.concatenate([np.random.default_rng(seed).choice(Nq - 3, 29, replace=False), [Nq - 3, Nq - 2, Nq - 1]])
        for i in sample:
            px, py, r = case["proj"][i, 0], case["proj"][i, 1], case["radius"][i]
            L = 0 if lv is None else int(lv[i])
            o = np.zeros(len(cell), np.int64) if oc is None else oc.astype(np.int64)
            keep = (cell[:, 0] >= 0) & (o >= L - 1) & (o <= L) & (np.abs(case["kpts"][:, 0] - px) < r) & (np.abs(case["kpts"][:, 1] - py) < r)
            want = sorted((cell[j, 0], cell[j, 1], j) for j in np.flatnonzero(keep))
            assert ls[i] == [j for _, _, j in want], i
        assert sum(len(ls[i]) for i in sample) > 32


def test_big_levels_gate_both_ways(oracle):
    c, octave, level, lists, ungated, seq = solved_levels(oracle)
    below = sum(1 for i, l in enumerate(ungated) for j in l if octave[j] < level[i] - 1)
    above = sum(1 for i, l in enumerate(ungated) for j in l if octave[j] > level[i])
    print(f"B-levels: {below} gated below, {above} above, {sum(len(l) for l in lists)} of {sum(len(l) for l in ungated)} kept, nmatches {seq['nmatches']}")
    assert below > 0 and above > 0 and sum(len(l) for l in lists) == sum(len(l) for l in ungated) - below - above
    assert seq["nmatches"] > 20 and (seq["best_dist"][1024:] <= PS.TH_HIGH).any()


def test_chain_1024_hands_over_between_trips(oracle):
    c, lists, seq, jac, rounds = solved_big(oracle, "chain-1024")
    assert all(l == [] for l in lists[:1000]) and all(len(l) == 64 for l in lists[1000:]) and len(lists) == 1080
    assert np.array_equal(seq["best_idx"][1000:1064], c["order"]) and seq["nmatches"] == 64
    assert (seq["best_idx"][:1000] == -1).all() and (seq["best_idx"][1064:] == -1).all() and (seq["best_dist"][1064:] == 256).all()
    for k in ("best_idx", "best_dist", "second_dist", "assign"):
        assert np.array_equal(seq[k], jac[k]), k
    assert rounds >= 64


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
