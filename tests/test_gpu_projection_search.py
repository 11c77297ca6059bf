"""GPU: SearchByProjection1 on the device (rfe_search_by_projection / _dev, SearchByProjection1_rfe) against the contract of DESIGN.md 6d
restated in tests/projection_search_ref.py.  Every comparison is exact (np.array_equal on every output)."""
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import projection_search_ref as PS
from test_projection_search_ref import chain_case, solved, solved_big, solved_levels, write_driver_case
from rover_slam_amd import capi

pytestmark = pytest.mark.gpu
KEYS = ("assign", "best_idx", "best_dist", "second_dist")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def same(got, ref, keys=KEYS):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (k, np.flatnonzero(got[k] != ref[k])[:8])
    assert got["nmatches"] == ref["nmatches"]


def host(ctx, c, **kw):
    a = dict(skip=c.get("skip"), observed=c.get("observed"))
    a.update({"kxy": c["kxy"]} if "kxy" in c else {"kpts": c["kpts"]})           # a case without kxy has float positions only
    a.update(kw)
    return ctx.search_by_projection(c["q"], c["proj"], c["radius"], c["desc"], c["bounds"], **a)


def dev(ctx, c, cand_cap, kxy=None, kpts=None, skip=None, observed=None, octave=None, pred_level=None, nf_dev=None, Nf=None, desc=None,
        th_high=1.4):
    """rfe_search_by_projection_dev on uploaded copies of host arrays; returns the host form's dict"""
    desc = c["desc"] if desc is None else desc
    Nq, Nf = len(c["proj"]), len(desc) if Nf is None else Nf
    bufs = []

    def up(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        bufs.append(ctx.alloc(max(a.nbytes, 4)).upload(a))
        return bufs[-1]
    out = {k: ctx.alloc(max(n, 1) * 4) for k, n in (("assign", Nf), ("best_idx", Nq), ("best_dist", Nq), ("second_dist", Nq), ("stats", 4))}
    try:
        ctx.search_by_projection_dev(up(c["q"], np.float32), up(c["proj"], np.float32), up(c["radius"], np.float32), Nq, up(desc, np.float32), Nf,
                                     c["bounds"], cand_cap, out["assign"], out["stats"], kpts=up(kpts, np.float32), kxy=up(kxy, np.int32),
                                     pred_level=up(pred_level, np.int32), observed=up(observed, np.uint8), octave=up(octave, np.int32),
                                     skip=up(skip, np.uint8), nf_dev=up(nf_dev, np.int32), th_high=th_high, best_idx=out["best_idx"],
                                     best_dist=out["best_dist"], second_dist=out["second_dist"])
        ctx.synchronize()
        r = {"assign": out["assign"].download((Nf,), np.int32), "best_idx": out["best_idx"].download((Nq,), np.int32),
             "best_dist": out["best_dist"].download((Nq,), np.float32), "second_dist": out["second_dist"].download((Nq,), np.float32),
             "stats": out["stats"].download((4,), np.int32)}
        r["nmatches"] = int(r["stats"][0])
        return r
    finally:
        for b in bufs + list(out.values()):
            b.free()


# ---------------------------------------------------------------- 1. host form against the restatement
@pytest.mark.parametrize("seed", (0, 1))
def test_host_form_vs_restatement(ctx, oracle, seed):
    c, lists, seq, jac, rounds = solved(oracle, seed)
    PS.check_vacuity(PS.vacuity(oracle, c, lists, seq, rounds), len(lists))
    got = host(ctx, c)
    same(got, seq)
    st = got["stats"]
    print(f"seed {seed}: nmatches {st[0]}, candidates {st[1]}, rounds {st[2]} (restatement {rounds})")
    assert st[0] == seq["nmatches"] and st[1] == sum(len(l) for l in lists) and st[2] >= 3 and st[2] == rounds and st[3] == 0
    sbi, _, _ = PS.static_scan(oracle, c["q"], c["desc"], lists, c["skip"])
    assert (sbi != got["best_idx"]).sum() >= len(lists) // 4          # the sequence matters: not what one bulk scan gives


# ---------------------------------------------------------------- 2. device form
def test_device_form(ctx, oracle):
    c, lists, seq, _, _ = solved(oracle, 0)
    total = sum(len(l) for l in lists)
    h = host(ctx, c)
    d = dev(ctx, c, total, kxy=c["kxy"], skip=c["skip"], observed=c["observed"])          # exactly the slots the lists need
    same(d, h)
    assert np.array_equal(d["stats"], h["stats"])
    k = dev(ctx, c, total + 100, kpts=c["kpts"], skip=c["skip"], observed=c["observed"])  # f32 positions
    same(k, h)
    # the feature count from the device: 32 zero rows behind the 300 features, *nf_dev = 300
    Nf = len(c["kxy"])
    pad = lambda a: np.concatenate([a, np.zeros((32,) + a.shape[1:], a.dtype)])   # noqa: E731
    p = dev(ctx, c, total, kxy=pad(c["kxy"]), skip=pad(c["skip"]), observed=c["observed"], nf_dev=np.array([Nf], np.int32), Nf=Nf + 32,
            desc=pad(c["desc"]))
    assert (p["assign"][Nf:] == -1).all()
    p["assign"] = p["assign"][:Nf]
    same(p, h)
    assert np.array_equal(p["stats"], h["stats"])
    # without nf_dev the zero rows ARE features at (0, 0): a different problem (and a count above Nf is clamped to Nf)
    big = dev(ctx, c, 4 * total, kxy=pad(c["kxy"]), skip=pad(c["skip"]), observed=c["observed"], nf_dev=np.array([10 ** 6], np.int32),
              Nf=Nf + 32, desc=pad(c["desc"]))
    lists32 = PS.candidate_lists(pad(c["kpts"]), None, c["bounds"], c["proj"], c["radius"])
    ref32 = PS.search_by_projection_seq(oracle, c["q"], pad(c["desc"]), lists32, pad(c["skip"]), c["observed"])
    same(big, ref32)


# ---------------------------------------------------------------- 3. levels
def test_levels(ctx, oracle):
    c = PS.make_case(3)
    rng = np.random.default_rng(33)
    octave = rng.integers(0, 3, len(c["kxy"])).astype(np.int32)
    level = rng.integers(0, 3, len(c["proj"])).astype(np.int32)
    lists = PS.case_lists(c, octave, level)
    ungated = PS.candidate_lists(c["kpts"], None, c["bounds"], c["proj"], c["radius"])
    below = sum(1 for i, l in enumerate(ungated) for j in l if octave[j] < level[i] - 1)
    above = sum(1 for i, l in enumerate(ungated) for j in l if octave[j] > level[i])
    assert below > 0 and above > 0 and sum(len(l) for l in lists) == sum(len(l) for l in ungated) - below - above
    ref = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists, c["skip"], c["observed"])
    assert ref["nmatches"] > 20
    same(host(ctx, c, octave=octave, pred_level=level), ref)
    same(dev(ctx, c, 8000, kpts=c["kpts"], skip=c["skip"], observed=c["observed"], octave=octave, pred_level=level), ref)
    # a level the device form cannot refuse gives that map point an empty list
    bad = level.copy(); bad[::2] = 99; bad[1::4] = -1
    lists_bad = [[] if (bad[i] < 0 or bad[i] > 15) else l for i, l in enumerate(lists)]
    ref_bad = PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists_bad, c["skip"], c["observed"])
    same(dev(ctx, c, 8000, kpts=c["kpts"], skip=c["skip"], observed=c["observed"], octave=octave, pred_level=bad), ref_bad)


# ---------------------------------------------------------------- 4. the chain: one round per map point
def test_chain(ctx, oracle):
    c = chain_case()
    got = host(ctx, c)
    assert np.array_equal(got["best_idx"][:64], c["order"])
    assert (got["best_idx"][64:] == -1).all() and (got["best_dist"][64:] == 256).all() and (got["second_dist"][64:] == 256).all()
    assert got["stats"][2] >= 64 and got["nmatches"] == 64
    assert np.array_equal(got["assign"][c["order"]], np.arange(64))
    lists = PS.candidate_lists(c["kpts"], None, c["bounds"], c["proj"], c["radius"])
    same(got, PS.search_by_projection_seq(oracle, c["q"], c["desc"], lists))


# ---------------------------------------------------------------- 5. no contention: the existing scan kernel
def test_unobserved_map_points_equal_search_candidates(ctx, oracle):
    c, lists, _, _, _ = solved(oracle, 1)
    got = host(ctx, c, observed=np.zeros(len(lists), np.uint8))
    off, cand = PS.to_csr(lists)
    bi, bd, sd = ctx.search_candidates(c["q"], c["desc"], off, cand, c["skip"])
    assert np.array_equal(got["best_idx"], bi) and np.array_equal(got["best_dist"], bd) and np.array_equal(got["second_dist"], sd)
    assert got["stats"][2] <= 2 and got["nmatches"] == int((bd <= PS.TH_HIGH).sum())
    last = np.full(len(c["kxy"]), -1, np.int32)
    for i in np.flatnonzero(bd <= PS.TH_HIGH):
        last[bi[i]] = i
    assert np.array_equal(got["assign"], last)


# ---------------------------------------------------------------- 6. overflow of the caller's slots
def test_overflow_is_reported_and_harmless(ctx, oracle):
    c, lists, seq, _, _ = solved(oracle, 0)
    total = sum(len(l) for l in lists)
    o = dev(ctx, c, 10, kxy=c["kxy"], skip=c["skip"], observed=c["observed"])
    assert o["stats"][3] == 1 and o["stats"][1] == total and o["stats"][0] == 0
    assert (o["assign"] == -1).all() and (o["best_idx"] == -1).all() and (o["best_dist"] == 256).all() and (o["second_dist"] == 256).all()
    o = dev(ctx, c, total - 1, kxy=c["kxy"], skip=c["skip"], observed=c["observed"])
    assert o["stats"][3] == 1 and (o["assign"] == -1).all()
    g = dev(ctx, c, total, kxy=c["kxy"], skip=c["skip"], observed=c["observed"])
    same(g, seq)
    assert g["stats"][3] == 0 and g["stats"][1] == total
    # the host form sizes the slots itself, also when it first guesses too few (16 per map point): every window holds every feature
    wide = dict(c, radius=np.full_like(c["radius"], 500.0))
    lw = PS.case_lists(wide)
    assert sum(len(l) for l in lw) > 16 * len(lw)
    hw = ctx.search_by_projection(c["q"][:40], c["proj"][:40], wide["radius"][:40], c["desc"], c["bounds"], kxy=c["kxy"], skip=c["skip"],
                                  observed=c["observed"][:40])
    same(hw, PS.search_by_projection_seq(oracle, c["q"][:40], c["desc"], lw[:40], c["skip"], c["observed"][:40]))
    assert hw["stats"][3] == 0 and hw["stats"][1] == sum(len(l) for l in lw[:40])


# ---------------------------------------------------------------- 7. empty shapes and refusals
def test_empty_and_refusals(ctx, oracle):
    c, lists, seq, _, _ = solved(oracle, 0)
    Nf = len(c["kxy"])
    e = ctx.search_by_projection(c["q"][:0], c["proj"][:0], c["radius"][:0], c["desc"], c["bounds"], kxy=c["kxy"])
    assert e["nmatches"] == 0 and len(e["best_idx"]) == 0 and (e["assign"] == -1).all() and len(e["assign"]) == Nf
    e = ctx.search_by_projection(c["q"], c["proj"], c["radius"], c["desc"][:0], c["bounds"], kxy=c["kxy"][:0])
    assert e["nmatches"] == 0 and (e["best_idx"] == -1).all() and (e["best_dist"] == 256).all() and (e["second_dist"] == 256).all()
    far = dict(c, proj=c["proj"] + np.float32([1000.0, 0.0]))
    e = host(ctx, far)
    assert e["nmatches"] == 0 and (e["best_idx"] == -1).all() and (e["assign"] == -1).all() and e["stats"][1] == 0
    # a NaN / infinite projection or radius in the device form: an empty list for that map point, everything else as the restatement
    nan = dict(c, proj=c["proj"].copy(), radius=c["radius"].copy())
    nan["proj"][0, 0] = np.nan; nan["proj"][5, 1] = np.inf; nan["radius"][9] = np.nan; nan["radius"][11] = np.inf; nan["proj"][13] = -3e38
    ln = [[] if i in (0, 5, 9, 11, 13) else l for i, l in enumerate(lists)]
    same(dev(ctx, nan, 8000, kxy=c["kxy"], skip=c["skip"], observed=c["observed"]),
         PS.search_by_projection_seq(oracle, c["q"], c["desc"], ln, c["skip"], c["observed"]))

    def refused(msg, fn):
        with pytest.raises(capi.RfeError) as ex:
            fn()
        assert "error -1" in str(ex.value) and msg in str(ex.value), str(ex.value)
    refused("non-finite", lambda: host(ctx, nan))
    refused("pred_level", lambda: host(ctx, c, pred_level=np.full(len(lists), 16, np.int32)))
    refused("pred_level", lambda: host(ctx, c, pred_level=np.full(len(lists), -1, np.int32)))
    refused("exactly one", lambda: host(ctx, c, kpts=c["kpts"]))
    refused("exactly one", lambda: host(ctx, c, kxy=None))
    refused("bounds", lambda: ctx.search_by_projection(c["q"], c["proj"], c["radius"], c["desc"], (0, 0, 0, 120), kxy=c["kxy"]))
    refused("bounds", lambda: ctx.search_by_projection(c["q"], c["proj"], c["radius"], c["desc"], (0, 130, 160, 120), kxy=c["kxy"]))
    z = np.zeros((4097, 256), np.float32)
    refused("Nf", lambda: ctx.search_by_projection(c["q"], c["proj"], c["radius"], z, c["bounds"], kxy=np.zeros((4097, 2), np.int32)))
    zq = np.zeros((16385, 256), np.float32)
    refused("Nq", lambda: ctx.search_by_projection(zq, np.zeros((16385, 2), np.float32), np.ones(16385, np.float32), c["desc"], c["bounds"],
                                                    kxy=c["kxy"]))
    # the device form validates the same scalars before it touches a pointer
    lib, h = capi.lib, ctx.h
    o = np.zeros((16,), np.float32).ctypes.data
    call = lambda Nq=4, Nf=4, q=o, f=o, kp=o, kx=None, b=(0.0, 0.0, 160.0, 120.0), cap=64, asg=o, st=o: lib.rfe_search_by_projection_dev(   # noqa: E731
        h, q, o, o, None, None, Nq, f, kp, kx, None, None, Nf, None, *b, 1.4, cap, asg, None, None, None, st)
    for kw, m in ((dict(Nq=-1), "Nq"), (dict(Nq=16385), "Nq"), (dict(Nf=-1), "Nf"), (dict(Nf=4097), "Nf"), (dict(b=(5.0, 0.0, 5.0, 120.0)), "bounds"),
                  (dict(b=(0.0, 9.0, 160.0, 9.0)), "bounds"), (dict(b=(0.0, 0.0, float("nan"), 120.0)), "bounds"), (dict(cap=-1), "cand_cap"),
                  (dict(kx=o), "exactly one"), (dict(kp=None), "exactly one"), (dict(q=None), "null"), (dict(f=None), "null"),
                  (dict(asg=None), "null"), (dict(st=None), "null")):
        assert call(**kw) == -1 and m in lib.rfe_last_error(h).decode(), (kw, lib.rfe_last_error(h).decode())
    same(host(ctx, c), seq)                                  # the ctx is still usable


# ---------------------------------------------------------------- 8. per-kernel profile stages
def test_profile_names_every_kernel(ctx, oracle):
    c, _, _, _, _ = solved(oracle, 0)
    ctx.profile(True); ctx.profile_reset()
    try:
        host(ctx, c)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False); ctx.profile_reset()
    for name in ("ps_grid", "ps_count", "ps_fill", "ps_resolve"):
        assert name in prof and prof[name][1] >= 1 and prof[name][0] > 0, prof


# ---------------------------------------------------------------- 9. the drop-in helper
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_helper(tmp_path, oracle):
    c, lists, seq, _, _ = solved(oracle, 0)
    exe = DD.build(tmp_path, "projection_search_driver")
    sel, prior = write_driver_case(str(tmp_path / "case.bin"), c)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    out = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    assert out[0] == seq["nmatches"] and len(out) == 1 + len(c["kxy"])
    want = np.where(seq["assign"] >= 0, sel[np.maximum(seq["assign"], 0)], np.where(prior >= 0, -2, -1))
    assert np.array_equal(out[1:], want)
    assert (out[1:][prior == 3] == -2).all()                 # a feature that had an observed map point keeps it
    assert ((out[1:] >= 0) & (prior == 0)).any()             # one without observations is overwritten
    # a two-camera rig is refused, nothing is touched
    write_driver_case(str(tmp_path / "rig.bin"), c, nleft=150)
    DD.run(exe, str(tmp_path / "rig.bin"), str(tmp_path / "rig_out.bin"))
    out = np.fromfile(str(tmp_path / "rig_out.bin"), np.int32)
    assert out[0] == -1 and np.array_equal(out[1:], np.where(prior >= 0, -2, -1))


# ================================================================ past one pass of the 1024-thread loops ("Sizes covered")
# A, B, C, B-levels and chain-1024 of tests/test_projection_search_ref.py: every 1024-stride loop takes further trips, a count thread
# owns several map points (or none), the LDS arrays are full, the bounds do not start at (0, 0) and the rounding of PosInGrid decides.
def pos(c):
    return {"kxy": c["kxy"]} if "kxy" in c else {"kpts": c["kpts"]}


def empty(o):
    return (o["assign"] == -1).all() and (o["best_idx"] == -1).all() and (o["best_dist"] == 256).all() and (o["second_dist"] == 256).all()


# ---------------------------------------------------------------- 10. host form against the restatement
@pytest.mark.parametrize("name", ("A", "B", "C", "chain-1024"))
def test_big_host_form_vs_restatement(ctx, oracle, name):
    c, lists, seq, _, rounds = solved_big(oracle, name)
    got = host(ctx, c)
    st = got["stats"]
    print(f"{name}: nmatches {st[0]}, candidates {st[1]}, rounds {st[2]} (restatement {rounds}), overflow {st[3]}")
    same(got, seq)
    assert st[0] == seq["nmatches"] and st[1] == sum(len(l) for l in lists) and st[3] == 0
    if name == "chain-1024":
        assert st[2] >= 64 and np.array_equal(got["best_idx"][1000:1064], c["order"])
    else:
        assert st[2] == rounds


# ---------------------------------------------------------------- 11. device form: exactly the slots, one too few, the count from the device
@pytest.mark.parametrize("name", ("B", "C"))
def test_big_device_form(ctx, oracle, name):
    c, lists, seq, _, rounds = solved_big(oracle, name)
    total, Nf = sum(len(l) for l in lists), len(c["kpts"])
    if name == "C":
        assert Nf == 4096
        d = dev(ctx, c, total, skip=c["skip"], observed=c["observed"], nf_dev=np.array([4096], np.int32), **pos(c))
    else:                            # 4093 features and three zero rows behind them: *nf_dev = 4093 keeps the rows at (0, 0) out of the grid
        assert Nf == 4093
        pad = lambda a: np.concatenate([a, np.zeros((3,) + a.shape[1:], a.dtype)])   # noqa: E731
        d = dev(ctx, c, total, kpts=pad(c["kpts"]), skip=pad(c["skip"]), observed=c["observed"], nf_dev=np.array([Nf], np.int32), Nf=4096,
                desc=pad(c["desc"]))
        assert (d["assign"][Nf:] == -1).all()
        d["assign"] = d["assign"][:Nf]
    same(d, seq)
    assert list(d["stats"]) == [seq["nmatches"], total, rounds, 0]
    o = dev(ctx, c, total - 1, skip=c["skip"], observed=c["observed"], **pos(c))
    assert o["stats"][3] == 1 and o["stats"][1] == total and o["stats"][0] == 0 and empty(o)


# ---------------------------------------------------------------- 12. the level gate with every octave slot in use
def test_big_levels(ctx, oracle):
    c, octave, level, lists, _, ref = solved_levels(oracle)
    total = sum(len(l) for l in lists)
    h = host(ctx, c, octave=octave, pred_level=level)
    same(h, ref)
    assert h["stats"][1] == total and h["stats"][3] == 0
    d = dev(ctx, c, total, kxy=c["kxy"], skip=c["skip"], observed=c["observed"], octave=octave, pred_level=level)
    same(d, ref)
    assert np.array_equal(d["stats"], h["stats"])


# ---------------------------------------------------------------- 13. one ctx across sizes: ws_ps after growth, the remembered ps_cap
def test_big_workspace_reuse(oracle):
    c = capi.Context(0)
    try:
        first = None
        for name in ("C", 0, "B", "C"):
            case, lists, seq, _, rounds = solved(oracle, name) if name == 0 else solved_big(oracle, name)
            got = host(c, case)
            same(got, seq)
            assert list(got["stats"]) == [seq["nmatches"], sum(len(l) for l in lists), rounds, 0], name
            if name == "C" and first is None:
                first = got
        for k in KEYS + ("stats",):
            assert np.array_equal(got[k], first[k]), k           # the second C, bit for bit
    finally:
        c.close()


# ---------------------------------------------------------------- 14. no contention at B: the existing scan kernel
def test_big_unobserved_map_points_equal_search_candidates(ctx, oracle):
    c, lists, _, _, _ = solved_big(oracle, "B")
    got = host(ctx, c, observed=np.zeros(len(lists), np.uint8))
    off, cand = PS.to_csr(lists)
    bi, bd, sd = ctx.search_candidates(c["q"], c["desc"], off, cand, c["skip"])
    assert np.array_equal(got["best_idx"], bi) and np.array_equal(got["best_dist"], bd) and np.array_equal(got["second_dist"], sd)
    assert got["stats"][2] <= 2 and got["nmatches"] == int((bd <= PS.TH_HIGH).sum())
    last = np.full(len(c["kpts"]), -1, np.int32)
    for i in np.flatnonzero(bd <= PS.TH_HIGH):
        last[bi[i]] = i
    assert np.array_equal(got["assign"], last)


# ---------------------------------------------------------------- 15. the drop-in helper at B: off-origin bounds through the Frame members
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_big_drop_in_helper(tmp_path, oracle):
    c, lists, seq, _, _ = solved_big(oracle, "B")
    exe = DD.build(tmp_path, "projection_search_driver")
    sel, prior = write_driver_case(str(tmp_path / "case.bin"), c)
    DD.run(exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin"))
    out = np.fromfile(str(tmp_path / "out.bin"), np.int32)
    assert out[0] == seq["nmatches"] and len(out) == 1 + len(c["kpts"])
    want = np.where(seq["assign"] >= 0, sel[np.maximum(seq["assign"], 0)], np.where(prior >= 0, -2, -1))
    assert np.array_equal(out[1:], want)
    assert (out[1:][prior == 3] == -2).all()                 # a feature that had an observed map point keeps it
    assert ((out[1:] >= 0) & (prior == 0)).any()             # one without observations is overwritten
