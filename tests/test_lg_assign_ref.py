"""CPU: the float64 reference of LightGlue's assignment stage (tests/lg_assign_ref.py) against the oracle on real pairs, the promises of its case
builder against that reference, and the fp32 yardstick behind LG_ASSIGN_TOL.  The GPU side is test_gpu_lg_assign.py."""
import numpy as np
import pytest

import lg_assign_ref as R
from tolerances import LG_ASSIGN_TOL, LG_ASSIGN_YARDSTICK


def _linear(a, W, b):
    """rfo_linear's accumulation order, column by column"""
    return np.stack([R.dot_f32_fma(a, W[j], 0.0 if b is None else b[j]) for j in range(W.shape[0])], 1)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_agrees_with_the_oracle_on_a_real_pair(oracle, golden_dir, tag):
    """sim and x rebuilt with numpy from the oracle's final token states (final_proj / 256^(1/4), md0 md1^T -- rfe_oracle.c:545-552), then
    `reference` against the oracle's own log-assignment matrix and match list.  Calibrated weights: log-scores of O(40), the range the bars are for."""
    from rover_slam_amd import weights as Wt
    g = np.load(f"{golden_dir}/lg_{tag}.npz")
    w = Wt.make_lightglue(seed=int(g["seed"]), calibrated=True)
    r = oracle.lightglue(w, g["k0n"], g["k1n"], g["d0"], g["d1"], debug=True)
    off = {name: (o, shape) for name, o, shape in Wt.lg_manifest()[0]}
    get = lambda name: w[off[name][0]:off[name][0] + int(np.prod(off[name][1]))].reshape(off[name][1])   # noqa: E731
    M, N = r["x0"].shape[0], r["x1"].shape[0]
    md0 = _linear(r["x0"], get("final_proj.W"), get("final_proj.b")) * np.float32(0.25)
    md1 = _linear(r["x1"], get("final_proj.W"), get("final_proj.b")) * np.float32(0.25)
    sim = _linear(md0, md1, None)
    x = np.zeros((2, max(M, N), 256), np.float32)
    x[0, :M], x[1, :N] = r["x0"], r["x1"]
    ref = R.reference(sim, x, get("matchability.w"), get("matchability.b"), M, N, 0.1)
    d = np.abs(r["scores"] - ref["scores"]).max()
    print(f"lg_{tag}: oracle vs reference, log-assignment {d:.3g} (bar {LG_ASSIGN_TOL['scores']:.3g}), {r['S']} matches")
    assert d <= LG_ASSIGN_TOL["scores"]
    assert r["S"] > 20 and np.array_equal(r["pairs"], ref["pairs"])
    assert np.abs(r["ms"] - ref["ms"]).max() <= LG_ASSIGN_TOL["scores"]      # probabilities <= 1: d exp(s) <= d s


def test_dispatch_table_reaches_every_form_from_both_sides():
    """every case names the form launch_lg_assign takes for it, every form has cases, and each inequality has a case on either side"""
    forms = {cid: c[0] for cid, c in R.CASES.items()}
    for cid, (form, P, L, lens, _) in R.CASES.items():
        assert R.form_of(P, L) == form and L % 4 == 0 and 4 <= L <= 4096 and len(lens) == P, cid
    assert set(forms.values()) == {"regs", "walk", "lds", "32x8"}
    few = lambda P, L: P * ((L + 31) // 32)   # noqa: E731
    assert few(127, 32) == 127 and few(128, 32) == 128 and few(3, 1000) < 128 <= few(4, 1000) and few(1, 2052) < 128 <= few(2, 2052) and few(1, 4096) == 128
    assert R.form_of(1, 1024) == "regs" and R.form_of(1, 1028) == "walk"
    assert all(P * (L // 32) == 256 for _, P, L, _, _ in (R.CASES[c] for c in ("lds-64x128", "lds-16x512", "lds-8x1024")))
    assert R.form_of(128, 32) == "32x8" and R.form_of(4, 1000) == "32x8" and R.form_of(2, 2052) == "32x8"


@pytest.mark.parametrize("cid", list(R.CASES))
def test_make_case_keeps_its_promises_and_the_yardstick_its_figures(cid):
    c, refs = R.case(cid), R.case_reference(cid)
    P, L, thr = c["P"], c["L"], 0.1
    with_scores = cid not in R.NO_SCORE_REFERENCE
    ties = 0
    for p in range(P):
        m, n, mt, r = int(c["lens"][p]), int(c["lens"][P + p]), c["meta"][p], refs[p]
        # padding is poison, the live block is finite
        pad = np.ones((L, L), bool)
        pad[:m, :n] = False
        assert not np.isfinite(c["sim"][p][pad]).any() and np.isfinite(c["sim"][p][:m, :n]).all()
        if pad.any():
            assert np.isnan(c["sim"][p][pad]).any() and np.isinf(c["sim"][p][pad]).any()
        assert np.isnan(c["x"][0, p, m:]).all() and np.isnan(c["x"][1, p, n:]).all()
        assert np.isfinite(c["x"][0, p, :m]).all() and np.isfinite(c["x"][1, p, :n]).all()
        wm64 = c["wm"].astype(np.float64)
        for side, toks in enumerate(mt["special"]):
            for t, v in toks:
                assert c["x"][side, p, t].astype(np.float64) @ wm64 + float(c["bm"][0]) == v      # exact: one non-zero component
        if len(mt["planted"]):
            assert (c["x"][0, p, mt["planted"][:, 0]].astype(np.float64) @ wm64 + R.BM >= 5).all()
            assert (c["x"][1, p, mt["planted"][:, 1]].astype(np.float64) @ wm64 + R.BM >= 5).all()
        assert len(mt["planted"]) >= min(m, n) // 2 - 8          # about half of min(m, n); the tie rows / columns are kept clear
        if not with_scores or m == 0 or n == 0:
            continue
        sc = r["scores"]
        listed = {tuple(q) for q in r["pairs"]}
        for i, j in mt["planted"]:
            assert (i, j) in listed and np.exp(sc[i, j]) > thr + 0.01, (cid, p, i, j)
        if mt["col_tie"]:
            ties += 1
            cols, row = mt["col_tie"]["cols"], mt["col_tie"]["row"]
            assert cols[0] == min(cols) and len(set(cols)) == 6 and max(cols) == n - 1
            assert len(set(sc[row, cols])) == 1 and sc[row, cols[0]] == sc[row].max()        # an exact tie of the float64 scores, at the row's maximum
            assert r["a0"][row] == cols[0] and r["a1"][cols[0]] == row                       # and the reference reports the first index
        if mt["row_tie"]:
            ties += 1
            rows, col = mt["row_tie"]["rows"], mt["row_tie"]["col"]
            assert rows[0] == min(rows) and len(set(rows)) == 6 and max(rows) == m - 1
            assert len(set(sc[rows, col])) == 1 and sc[rows[0], col] == sc[:, col].max()
            assert r["a1"][col] == rows[0] and (r["a0"][rows] == col).all()
            assert (rows[0], col) in listed and not any((i, col) in listed for i in rows[1:])
    assert ties > 0 or max(int(v) for v in c["lens"]) < 130 or not with_scores
    # the yardstick: plain sequential fp32 is never further from the reference than the figures the GPU bars are four times of
    worst = {}
    for p in range(P):
        m, n = int(c["lens"][p]), int(c["lens"][P + p])
        y = R.yardstick_f32(c["sim"][p], c["x"][:, p], c["wm"], c["bm"], m, n, with_scores)
        for k, v in R.distances(y, refs[p]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(cid, {k: f"{v:.3g}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1.25 * LG_ASSIGN_YARDSTICK[k], (k, v)     # 1.25: np.exp / np.log in float32 differ by an ulp between numpy builds


def test_yardstick_figures_are_reached():
    """the stated figures are measurements, not ceilings: the case named beside each in tolerances.py comes within a factor of two of it"""
    for k, cid in (("z", "lds-64x128"), ("scores", "32x8-2x2052"), ("rowlse", "32x8-1x4096"), ("collse", "32x8-1x4096")):
        c, refs = R.case(cid), R.case_reference(cid)
        P = c["P"]
        worst = max(R.distances(R.yardstick_f32(c["sim"][p], c["x"][:, p], c["wm"], c["bm"], int(c["lens"][p]), int(c["lens"][P + p]),
                                                cid not in R.NO_SCORE_REFERENCE), refs[p]).get(k, 0.0) for p in range(P))
        assert worst >= 0.5 * LG_ASSIGN_YARDSTICK[k], (k, cid, worst)
