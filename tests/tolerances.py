"""Stated fp32 tolerances of the parity tests, in one place (profiles/r02_lg_tolerance.md).

SuperPoint has none: keypoints, scores and descriptors are bit-exact against the oracle.

LightGlue match scores are probabilities exp(log-assignment); the log-assignment is a difference of O(30-100)
similarity logits and their log-sum-exps, so a few fp32 ulps there (6e-6 each at 50) are 1e-4-level in the score.
Measured at K = 1024 over 40 (weight seed, input) cases (tools/lg_tolerance_study.py -> profiles/r02_lg_tolerance.md),
max |score difference| over common matches, match lists identical in every case and variant:
  oracle (fp32) vs float64 evaluation of the same graph   2.6e-4
  HIP path vs oracle                                       3.2e-4 (Wo folded into ffn.0, the default) / 2.0e-4 (unfolded)
  HIP path vs float64                                      2.4e-4 (folded) / 1.8e-4 (unfolded)
  HF transformers (fp32, torch CPU) vs float64             1.2e-4 (the two full-size fixtures)
Round 3 (profiles/r03_lg_tolerance.md, final kernels; every case also inside a 16-pair call = the THROUGHPUT tiling the benchmark times):
  HIP single pair vs oracle / vs float64                   2.8e-4 / 2.3e-4        HIP 16-pair batch vs oracle / vs float64   3.2e-4 / 1.8e-4
  randomised sweep, 29 weight seeds, 1216 ragged pairs inside 16-20-pair calls (profiles/r03_fuzz_fp16x2.md): HIP vs oracle <= 3.5e-4 (fp32) / 4.0e-4 (RFE_OPT_LG_FP16X2)
i.e. any two fp32 evaluation orders of this graph differ by 1-3e-4 (the case with the largest HIP-vs-oracle figure is the
one where the ORACLE sits 2.6e-4 from float64 and the HIP path 7e-5): 1e-4 is below the noise floor of fp32 itself at this
size, and the fold does not change the picture.  Final token states agree to 1e-5 (bar 1e-4).
"""
LG_SCORE_TOL_CALIBRATED = 1e-4   # north_star's figure, on the CALIBRATED weight set (weights.make_lightglue(calibrated=True): token norms O(1), log-assignment
                            # peaks at 52-63 -- the range trained LightGlue logits live in).  Measured there: oracle vs torch modules vs graph execution
                            # 5-7e-6, HIP vs oracle 1.3-1.5e-5 (profiles/r04_weight_scale.md rows ffn.3 x 0.25 / final_proj x 0.25).  Every bar below
                            # is for the ILL-CONDITIONED seeded default set (log-assignment up to |850|, one fp32 ulp there = 6e-5 in the log domain).
LG_SCORE_TOL = 5e-4         # |match score difference|, any keypoint count up to 1024
LG_SCORE_TOL_SMALL = 2e-4   # <= 256 keypoints per side.  Round 4 (profiles/r04_lg_tolerance_k256.md, 20 cases at K <= 256): the ORACLE sits up to 1.19e-4
                            # from the float64 evaluation of the same graph, the HIP path 1.27e-4 from the oracle and 1.54e-4 from float64 (match lists
                            # identical in every case) -- a 1e-4 bar against the oracle was below the noise floor of fp32 here too; it held in rounds
                            # 1-3 only because the one-pair GEMM tiles happened to sum k in the oracle's order (bit-identical Linears), which the
                            # 16x16x4 latency tiling (gemm_lat.hip: k permuted inside 16-k groups, LayerNorm + GELU fused) no longer does
LG_STATE_TOL = 1e-4         # final token states x0 / x1
LG_LOGSCORE_RTOL = 1e-5     # log-domain assignment matrix relative to its largest magnitude (|values| up to ~450, one fp32
                            # ulp there is 3e-5; measured 2.4e-3 absolute = 5.4e-6 relative)
LG_LOGSCORE_ATOL = 1e-2     # the same matrix, absolute (used where the largest magnitude is small, e.g. two identical frames: the error of a
                            # log-score is a sum of fp32 roundings of O(100) similarity logits and does not shrink with the largest entry; measured 3.8e-3);
                            # every entry is ALSO compared as a probability, exp(score), within LG_SCORE_TOL


def lists_agree(pairs_a, ms_a, pairs_b, ms_b, filter_thr=0.1, slack=5e-4):
    """Two match lists are the same up to matches whose score sits within `slack` of the 0.1 filter (either side may
    drop them).  Returns (ok, max |score difference| over the common matches)."""
    da = {(int(i), int(j)): float(s) for (i, j), s in zip(pairs_a, ms_a)}
    db = {(int(i), int(j)): float(s) for (i, j), s in zip(pairs_b, ms_b)}
    only = [(k, da.get(k, db.get(k))) for k in da.keys() ^ db.keys()]
    ok = all(abs(s - filter_thr) <= slack for _, s in only)
    dev = max((abs(da[k] - db[k]) for k in da.keys() & db.keys()), default=0.0)
    return ok, dev


def _top2_gap(logscores):
    """difference of the two largest match probabilities of a row / column of the log-assignment matrix"""
    import numpy as np
    t = np.sort(logscores)[-2:]
    return float(np.exp(t[-1]) - np.exp(t[0])) if len(t) == 2 else float("inf")


def borderline(sc, i, j, keypoints, filter_thr=0.1, tol=None):
    """A match that only one side reports is legitimate when fp32 noise can produce it: match probabilities agree to
    tol = LG_SCORE_TOL_SMALL (<= 256 keypoints) / LG_SCORE_TOL, so the filter can flip within tol of its threshold and a
    row / column argmax can flip when the two best probabilities are closer than 2 tol (each moves by up to tol).
    sc: the reference's log-assignment matrix [M,N]."""
    import numpy as np
    if tol is None:
        tol = LG_SCORE_TOL_SMALL if keypoints <= 256 else LG_SCORE_TOL
    return abs(float(np.exp(sc[i, j])) - filter_thr) < tol or _top2_gap(sc[i]) < 2 * tol or _top2_gap(sc[:, j]) < 2 * tol


def lists_agree_borderline(pairs_a, ms_a, pairs_b, ms_b, scores_ref, keypoints, filter_thr=0.1, tol=None):
    """Match lists equal up to borderline flips (see `borderline`).  Returns (ok, max |score difference| over the common
    matches, number of one-sided matches)."""
    da = {(int(i), int(j)): float(s) for (i, j), s in zip(pairs_a, ms_a)}
    db = {(int(i), int(j)): float(s) for (i, j), s in zip(pairs_b, ms_b)}
    only = da.keys() ^ db.keys()
    ok = all(borderline(scores_ref, i, j, keypoints, filter_thr, tol) for (i, j) in only)
    dev = max((abs(da[k] - db[k]) for k in da.keys() & db.keys()), default=0.0)
    return ok, dev, len(only)


# LightGlue's assignment stage ALONE against float64 (tests/lg_assign_ref.py, tests/test_gpu_lg_assign.py): absolute bars in the log domain.
# Yardstick: the stage's formulas evaluated sequentially in np.float32 in the oracle's order (lg_assign_ref.yardstick_f32, rfe_oracle.c:553-576) on the
# sixteen cases of lg_assign_ref.CASES (1 x 36 ... 1 x 4096 keypoints, every form of launch_lg_assign), largest distance from lg_assign_ref.reference:
#   z 2.59e-6 (lds-64x128)   row log-sum-exp 2.26e-5 (32x8-1x4096)   column log-sum-exp 2.09e-5 (32x8-1x4096)   scores 2.74e-5 (32x8-2x2052)
# The GPU bar is FOUR times the yardstick's figure: its reduction trees differ from the sequential order (and are normally closer to float64).
# test_lg_assign_ref.py re-measures the yardstick on every case, so the bars cannot drift away from what they were derived from.
LG_ASSIGN_YARDSTICK = dict(z=2.59e-6, rowlse=2.26e-5, collse=2.09e-5, scores=2.74e-5)
LG_ASSIGN_TOL = {k: 4 * v for k, v in LG_ASSIGN_YARDSTICK.items()}
