"""LightGlue's assignment stage alone (rfe_k_lightglue_assign = the forward's lg_assign_stage: matchability head, row / column log-sum-exp, both
argmaxes, mutual check, filter, ordered compaction) against the float64 reference of tests/lg_assign_ref.py, in every form launch_lg_assign takes.

The form is a function of (P, L) alone and the profile has one stage name ("lg_assign") for all of them, so the dispatch is restated here
(lg_assign_ref.form_of, from lg_kernels.hip launch_lg_assign) and every row of the table is held to the form it is meant for:

    few pairs   P * ceil(L / 32) < 128     column in registers  (L <= 1024)   lg_rowlse_z + lg_col_kernel<16, 64, CACHE>
                                           walking form         (L >  1024)   lg_rowlse_z + lg_col_kernel<16, 64>
    otherwise   L <= 1024, L % 32 == 0, P * (L / 32) >= 256    stripe in LDS  lg_matchability + lg_rowlse + lg_col_lds_kernel
                anything else                                                 lg_matchability + lg_rowlse + lg_col_kernel<32, 8>
    all of them: lg_rowarg_kernel, lg_mutual_kernel.

    form   P     L     pairs (m, n); unnamed pairs are seeded mixes of full, nearly full and arbitrary lengths
    regs   1     36    (36, 33)
    regs   2     200   (1, 200), (200, 1)
    regs   1     1024  (1024, 1021)
    regs   3     1000  (1000, 997), (3, 1000), (640, 70)
    regs   3     1024  (1024, 1024), (1023, 15), (17, 1024)
    regs   127   32    (0, 32), (32, 0), (0, 0), (5, 31), ...                  127 < 128
    walk   1     1028  (1028, 1025)                                            rows past 16 x 64
    walk   1     2052  (1500, 2049)
    lds    64    128   (5, 128), (33, 31), (128, 1), (0, 64), (64, 0), (127, 97), ...     64 * 4 = 256
    lds    16    512   (512, 512), (509, 33), (7, 512), (131, 130), ...                   16 * 16 = 256
    lds    8     1024  (1024, 1024), (1021, 40), (9, 1000), (1000, 9), ...                8 * 32 = 256
    32x8   128   32    the 127 above and (32, 32)                              128: not few; 128 * 1 < 256
    32x8   4     1000  the 3 above and (1000, 1000)                            4 * 32 = 128: not few; 1000 % 32 != 0
    32x8   43    100   (100, 100), (1, 100), (100, 1), (0, 7), ...
    32x8   2     2052  (2052, 2049), (2052, 2052)                              2 * 65 = 130; L > 1024
    32x8   1     4096  (4096, 4093)                                            1 * 128 = 128: the one-pair boundary

Exact checks (no tolerance, no exemption): the dumped scores are lg_score of the device's own z / rowlse / collse bit for bit; a0 / mx0 / a1 are
np.argmax (first maximum) / max of that dump; every planted exact tie reports its lowest index; S / pairs / ms are the ascending-i compaction of the
device's a0 / a1 / mx0; nothing outside the live block is written.  Against float64: z, rowlse, collse, scores within LG_ASSIGN_TOL (tolerances.py).

What the stage does at the edges, asserted as found in the kernels: z is written for EVERY padded row (lg_matchability_kernel has no lengths; pad rows of
x are NaN here, so those z are not looked at); a pair with n == 0 gets rowlse = mx0 = -inf and a0 = 0 on its m rows, one with m == 0 collse = -inf and
a1 = 0 on its n columns (log-sum-exp and argmax of nothing), S = 0 either way."""
import ctypes as C

import numpy as np
import pytest

import lg_assign_ref as R
from tolerances import LG_ASSIGN_TOL

SENT = 0x7FC5A5A5          # the sentinel word: a NaN as float32, 2143659429 as int32 -- neither can be a result
F32 = np.float32
ONE_PER_FORM = ["regs-3x1000", "walk-1x1028", "lds-16x512", "32x8-43x100"]


@pytest.fixture(scope="module")
def ctx():
    from rover_slam_amd import capi
    c = capi.Context(0)     # no weights: the hook needs a ctx alone
    yield c
    c.close()


def _run(ctx, c, thr=0.1, cap=None, scores_pair=-1, want_scores=True):
    """one call of the hook on case c; every output as a host array, words the stage left alone still SENT"""
    from rover_slam_amd import capi
    P, L = c["P"], c["L"]
    cap = L if cap is None else cap
    shapes = dict(z=((2, P, L), F32), rowlse=((P, L), F32), collse=((P, L), F32), mx0=((P, L), F32), a0=((P, L), np.int32), a1=((P, L), np.int32),
                  S=((P,), np.int32), pairs=((P, cap, 2), np.int32), ms=((P, cap), F32))
    if want_scores:
        shapes["scores"] = ((P, L, L) if scores_pair < 0 else (L, L), F32)
    bufs = []
    try:
        def up(a):
            b = ctx.alloc(a.nbytes); bufs.append(b); b.upload(a); return b
        ins = [up(c[k]) for k in ("sim", "x", "wm", "bm", "lens")]
        outs = {}
        for k, (shape, dt) in shapes.items():
            outs[k] = ctx.alloc(int(np.prod(shape)) * 4); bufs.append(outs[k])
        ptr = lambda k: outs[k].ptr if k in outs else None   # noqa: E731
        ctx._chk(capi.lib.rfe_k_lightglue_assign(ctx.h, *[b.ptr for b in ins], P, L, thr, cap, scores_pair, C.c_int32(SENT),
                                                 *[ptr(k) for k in ("z", "rowlse", "collse", "mx0", "a0", "a1", "S", "pairs", "ms", "scores")]))
        return {k: outs[k].download(shape, dt) for k, (shape, dt) in shapes.items()}
    finally:
        for b in bufs:
            b.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _is_sent(a):
    return bool((_bits(a) == SENT).all())


def _lens(c, p):
    return int(c["lens"][p]), int(c["lens"][c["P"] + p])


def _expected_list(a0, a1, mx0, m, n, thr, listed):
    """the ascending-i compaction of the device's own a0 / a1 / mx0.  Membership is free only where |exp(mx0) - thr| is within 4 ulp of thr (the
    device's expf against float64's); `listed` decides those rows and nothing else."""
    if m == 0 or n == 0:
        return []
    e = np.exp(mx0[:m].astype(np.float64))
    mutual = a1[a0[:m]] == np.arange(m)
    slack = 4 * float(np.spacing(F32(thr)))
    out = []
    for i in np.flatnonzero(mutual):
        if e[i] > thr + slack or (abs(e[i] - thr) <= slack and i in listed):
            out.append((int(i), int(a0[i])))
    return out


def check_exact(c, o, thr, cap, scores_pair=-1):
    """checks 1-4 and 6 of the issue on one call's outputs: nothing here has a tolerance"""
    P, L = c["P"], c["L"]
    for p in range(P):
        m, n = _lens(c, p)
        mt = c["meta"][p]
        tag = f"{c['id']} pair {p} ({m}, {n})"
        z0, z1, lr, lc = o["z"][0, p, :m], o["z"][1, p, :n], o["rowlse"][p, :m], o["collse"][p, :n]
        # 6. padding: everything past m / n is untouched
        for k, live in (("rowlse", m), ("mx0", m), ("a0", m), ("collse", n), ("a1", n)):
            assert _is_sent(o[k][p, live:]), f"{tag}: {k} written past its live length"
        S = int(o["S"][p])
        assert 0 <= S <= min(cap, m, n), tag
        assert _is_sent(o["pairs"][p, S:]) and _is_sent(o["ms"][p, S:]), f"{tag}: match list written past S"
        dump = None
        if "scores" in o and (scores_pair < 0 or scores_pair == p):
            dump = o["scores"][p] if scores_pair < 0 else o["scores"]
            pad = np.ones((L, L), bool)
            pad[:m, :n] = False
            assert (_bits(dump)[pad] == SENT).all(), f"{tag}: score dump written outside the live block"
        if m == 0 or n == 0:        # an empty pair: log-sum-exp and argmax of nothing, no match
            assert S == 0, tag
            assert (lr == -np.inf).all() and (o["mx0"][p, :m] == -np.inf).all() and (o["a0"][p, :m] == 0).all(), tag
            assert (lc == -np.inf).all() and (o["a1"][p, :n] == 0).all(), tag
            continue
        for k, v in (("z0", z0), ("z1", z1), ("rowlse", lr), ("collse", lc), ("mx0", o["mx0"][p, :m])):
            assert np.isfinite(v).all(), f"{tag}: {k} not finite"
        a0, a1, mx0 = o["a0"][p], o["a1"][p], o["mx0"][p]
        assert (a0[:m] >= 0).all() and (a0[:m] < n).all() and (a1[:n] >= 0).all() and (a1[:n] < m).all(), tag
        # 3. every planted tie reports its lowest index, by name (first, so that a broken tie rule is reported as one)
        if mt["col_tie"]:
            cols, row = mt["col_tie"]["cols"], mt["col_tie"]["row"]
            assert a0[row] == cols[0], f"{tag}: row {row} ties over columns {cols}; a0 = {a0[row]}, the first is {cols[0]}"
            assert a1[cols[0]] == row, tag
        if mt["row_tie"]:
            rows, col = mt["row_tie"]["rows"], mt["row_tie"]["col"]
            assert a1[col] == rows[0], f"{tag}: column {col} ties over rows {rows}; a1 = {a1[col]}, the first is {rows[0]}"
            assert (a0[rows] == col).all(), tag
        if dump is not None:
            live = dump[:m, :n]
            assert np.isfinite(live).all(), f"{tag}: score dump not finite"
            # 1. the dump is lg_score (adds and subtracts only) of the device's own quantities, bit for bit
            s = c["sim"][p, :m, :n]
            mine = ((s - lr[:, None]) + (s - lc[None, :])) + (z0[:, None] + z1[None, :])
            assert mine.dtype == F32 and np.array_equal(_bits(mine), _bits(live)), f"{tag}: dump is not lg_score(sim, rowlse, collse, z)"
            # 2. argmaxes: the FIRST maximum, and the maximum itself bitwise
            assert np.array_equal(a0[:m], live.argmax(1)), f"{tag}: a0 is not the first row maximum at rows {np.flatnonzero(a0[:m] != live.argmax(1))[:8]}"
            assert np.array_equal(_bits(mx0[:m]), _bits(live.max(1))), f"{tag}: mx0"
            assert np.array_equal(a1[:n], live.argmax(0)), f"{tag}: a1 is not the first column maximum at columns {np.flatnonzero(a1[:n] != live.argmax(0))[:8]}"
            # ... and the planted ties are exact ties on the device, not near ties
            if mt["col_tie"]:
                assert len(set(_bits(live[mt["col_tie"]["row"], mt["col_tie"]["cols"]]).tolist())) == 1, f"{tag}: planted identical columns do not tie"
            if mt["row_tie"]:
                assert len(set(_bits(live[mt["row_tie"]["rows"], mt["row_tie"]["col"]]).tolist())) == 1, f"{tag}: planted identical rows do not tie"
        # 4. the match list is the ascending-i compaction of a0 / a1 / mx0
        got = [tuple(int(v) for v in q) for q in o["pairs"][p, :S]]
        want = _expected_list(a0, a1, mx0, m, n, thr, {i for i, _ in got})
        assert got == want[:cap], f"{tag}: match list is not the ordered compaction (S = {S}, expected {min(len(want), cap)})"
        e = np.exp(mx0[[i for i, _ in got]].astype(np.float64))
        assert (np.abs(o["ms"][p, :S] - e) <= 2 * np.spacing(e.astype(F32))).all(), f"{tag}: ms is not exp(mx0) within 2 ulp"


def check_reference(c, o, refs, thr, cap):
    """check 5: against float64, and the planted matches.  Returns the largest distances (for profiles/lg_assign.md)."""
    P = c["P"]
    worst = {}
    for p in range(P):
        m, n = _lens(c, p)
        r, mt = refs[p], c["meta"][p]
        got = dict(z0=o["z"][0, p, :m], z1=o["z"][1, p, :n])
        if m and n:
            got.update(rowlse=o["rowlse"][p, :m], collse=o["collse"][p, :n])
            if "scores" in r and "scores" in o:
                got["scores"] = o["scores"][p, :m, :n]
        for k, v in R.distances(got, r).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if "pairs" in r and thr <= 0.1 and cap >= min(m, n):
            S = int(o["S"][p])
            listed = {tuple(int(v) for v in q) for q in o["pairs"][p, :S]}
            planted_rows = {int(i) for i, _ in mt["planted"]}
            for i, j in mt["planted"]:
                assert (int(i), int(j)) in listed, f"{c['id']} pair {p}: planted match ({i}, {j}) is missing"
            if thr == 0.1:
                assert {q for q in listed if q[0] in planted_rows} == {tuple(int(v) for v in q) for q in r["pairs"] if int(q[0]) in planted_rows}
    print(f"{c['id']}: max |GPU - float64|", {k: f"{v:.3g}" for k, v in sorted(worst.items())})
    for k, v in worst.items():
        assert v <= LG_ASSIGN_TOL[k], f"{c['id']}: {k} is {v:.3g} from float64, bar {LG_ASSIGN_TOL[k]:.3g}"
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(R.CASES))
def test_assign_stage_every_form(ctx, cid):
    c = R.case(cid)
    assert R.form_of(c["P"], c["L"]) == c["form"]
    o = _run(ctx, c)
    check_exact(c, o, 0.1, c["L"])
    if cid in R.NO_SCORE_REFERENCE:
        o = {k: v for k, v in o.items() if k != "scores"}
    check_reference(c, o, R.case_reference(cid), 0.1, c["L"])


@pytest.mark.gpu
@pytest.mark.parametrize("thr", [0.0, 1.5])
@pytest.mark.parametrize("cid", ONE_PER_FORM)
def test_thresholds(ctx, cid, thr):
    c = R.case(cid)
    o = _run(ctx, c, thr=thr)
    check_exact(c, o, thr, c["L"])
    if thr > 1:
        assert (o["S"] == 0).all()               # a probability never exceeds 1
    else:
        check_reference(c, o, R.case_reference(cid), thr, c["L"])
        assert all(int(o["S"][p]) >= len(c["meta"][p]["planted"]) for p in range(c["P"]))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["regs-1x1024", "lds-16x512"])
def test_list_capacity(ctx, cid):
    """cap = min(m, n) of the first pair, and a short cap = 7: S == 7 and the first seven matches of the full list, in order"""
    c = R.case(cid)
    m, n = _lens(c, 0)
    full = _run(ctx, c, cap=min(m, n), want_scores=False)
    check_exact(c, full, 0.1, min(m, n))
    assert int(full["S"][0]) >= len(c["meta"][0]["planted"]) > 7
    short = _run(ctx, c, cap=7, want_scores=False)
    check_exact(c, short, 0.1, 7)
    for p in range(c["P"]):
        S = min(int(full["S"][p]), 7)
        assert int(short["S"][p]) == S
        assert np.array_equal(short["pairs"][p, :S], full["pairs"][p, :S]) and np.array_equal(_bits(short["ms"][p, :S]), _bits(full["ms"][p, :S]))
    assert int(short["S"][0]) == 7
    for k in ("z", "rowlse", "collse", "mx0", "a0", "a1"):
        assert np.array_equal(_bits(short[k]), _bits(full[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ONE_PER_FORM)
def test_one_pair_dump_and_repeatability(ctx, cid):
    """scores_pair = k: the [L, L] buffer holds slice k of the all-pairs dump bit for bit; and the same call twice is bit-for-bit equal"""
    c = R.case(cid)
    a, b = _run(ctx, c), _run(ctx, c)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{cid}: {k} differs between two identical calls"
    k = c["P"] - 1 if c["P"] < 3 else 2
    one = _run(ctx, c, scores_pair=k)
    assert one["scores"].shape == (c["L"], c["L"])
    assert np.array_equal(_bits(one["scores"]), _bits(a["scores"][k]))
    check_exact(c, one, 0.1, c["L"], scores_pair=k)
    for q in ("z", "rowlse", "collse", "mx0", "a0", "a1", "S", "pairs", "ms"):
        assert np.array_equal(_bits(one[q]), _bits(a[q])), q


@pytest.mark.gpu
def test_two_forms_agree_on_shared_pairs(ctx):
    """3 x 1000 (column in registers) and 4 x 1000 (<32, 8>) share their first three pairs: the two forms agree within the tolerance, and exactly on
    a0 / a1 at the planted rows and columns"""
    c3, c4 = R.case("regs-3x1000"), R.case("32x8-4x1000")
    assert np.array_equal(_bits(c3["sim"]), _bits(c4["sim"][:3])) and np.array_equal(_bits(c3["x"]), _bits(c4["x"][:, :3]))
    o3, o4 = _run(ctx, c3), _run(ctx, c4)
    for p in range(3):
        m, n = _lens(c3, p)
        assert _lens(c4, p) == (m, n)
        d = dict(z=max(np.abs(o3["z"][0, p, :m] - o4["z"][0, p, :m]).max(), np.abs(o3["z"][1, p, :n] - o4["z"][1, p, :n]).max()),
                 rowlse=np.abs(o3["rowlse"][p, :m] - o4["rowlse"][p, :m]).max(), collse=np.abs(o3["collse"][p, :n] - o4["collse"][p, :n]).max(),
                 scores=np.abs(o3["scores"][p, :m, :n] - o4["scores"][p, :m, :n]).max())
        print(f"pair {p}: regs vs 32x8", {k: f"{float(v):.3g}" for k, v in d.items()})
        for k, v in d.items():
            assert v <= LG_ASSIGN_TOL[k], (p, k, v)
        pl = c3["meta"][p]["planted"]
        assert np.array_equal(o3["a0"][p, pl[:, 0]], o4["a0"][p, pl[:, 0]]) and np.array_equal(o3["a0"][p, pl[:, 0]], pl[:, 1])
        assert np.array_equal(o3["a1"][p, pl[:, 1]], o4["a1"][p, pl[:, 1]]) and np.array_equal(o3["a1"][p, pl[:, 1]], pl[:, 0])
