"""LightGlue's assignment stage on its own ("Assignment"; rfe_k_lightglue_assign = the forward's lg_assign_stage): a float64
reference of the stage, the fp32 yardstick the tolerances come from, the dispatch conditions of launch_lg_assign restated, and the builder of the
test cases with their planted matches, planted exact ties and poisoned padding.  Shared by test_lg_assign_ref.py (CPU) and test_gpu_lg_assign.py."""
import functools

import numpy as np

F32 = np.float32
K0, BM = 37, 0.25          # make_case: wm[K0] = 0.5 and bm = 0.25 exactly, so a token with one non-zero component has an exactly representable logit
SPECIAL_LOGITS = (0.0, 40.0, -40.0, 100.0, -100.0)
TIE_COL_STEPS = (0, 1, 64, 65)      # + 16 k and the last live column: another lane, the same lane one pass of the wave later, another stripe of either width
TIE_ROW_STEPS = (0, 1, 8, 32, 64)   # + the last live row: another row group of every form (8, 32 and 64 groups) and the SAME group of each of them


# ------------------------------------------------------------------------------------------------ dispatch (lg_kernels.hip: launch_lg_assign)
def form_of(P, L):
    """The three inequalities of launch_lg_assign, restated: which column kernel (P, L) runs."""
    if P * ((L + 31) // 32) < 128:                                  # lg_assign_few_pairs: matchability inside the row log-sum-exp launch
        return "regs" if L <= 1024 else "walk"                      # lg_col_kernel<16, 64, CACHE> / lg_col_kernel<16, 64>
    if L <= 1024 and L % 32 == 0 and P * (L // 32) >= 256:
        return "lds"                                                # lg_col_lds_kernel
    return "32x8"                                                   # lg_col_kernel<32, 8>


# ------------------------------------------------------------------------------------------------ float64 reference
def logsigmoid(t):
    """log sigmoid in the stable two-branch form, in the precision of t"""
    t = np.asarray(t)
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, -np.log1p(e), t - np.log1p(e))


def _lse(v, axis):
    mx = v.max(axis=axis, keepdims=True)
    return (mx + np.log(np.exp(v - mx).sum(axis=axis, keepdims=True))).squeeze(axis)


def match_list(scores, thr):
    """first-maximum argmaxes, mutual check, exp, strict > thr, ascending i"""
    a0, a1 = scores.argmax(1), scores.argmax(0)
    mx0 = scores.max(1)
    keep = [i for i in range(scores.shape[0]) if a1[a0[i]] == i and np.exp(mx0[i]) > thr]
    return a0, mx0, a1, np.array([(i, a0[i]) for i in keep], np.int64).reshape(-1, 2), np.exp(mx0[keep])


def reference(sim, x, wm, bm, m, n, thr, with_scores=True):
    """One pair in float64 from the float32 inputs: sim [>= m, >= n], x [2, >= max(m, n), 256] (side 0 / side 1 token states), wm [256], bm [1].
    Returns z0 [m], z1 [n], rowlse [m], collse [n] and, with_scores, scores [m, n], a0, mx0, a1, pairs [S, 2], ms [S]."""
    s = np.asarray(sim, F32)[:m, :n].astype(np.float64)
    w, b = np.asarray(wm, F32).astype(np.float64), float(np.asarray(bm, F32).reshape(-1)[0])
    r = dict(z0=logsigmoid(np.asarray(x[0][:m], F32).astype(np.float64) @ w + b), z1=logsigmoid(np.asarray(x[1][:n], F32).astype(np.float64) @ w + b))
    if m == 0 or n == 0:
        r.update(rowlse=np.full(m, -np.inf), collse=np.full(n, -np.inf))
        if with_scores:
            r.update(scores=np.zeros((m, n)), a0=np.zeros(m, np.int64), mx0=np.full(m, -np.inf), a1=np.zeros(n, np.int64),
                     pairs=np.zeros((0, 2), np.int64), ms=np.zeros(0))
        return r
    r.update(rowlse=_lse(s, 1), collse=_lse(s, 0))
    if with_scores:
        sc = ((s - r["rowlse"][:, None]) + (s - r["collse"][None, :])) + (r["z0"][:, None] + r["z1"][None, :])
        a0, mx0, a1, pairs, ms = match_list(sc, thr)
        r.update(scores=sc, a0=a0, mx0=mx0, a1=a1, pairs=pairs, ms=ms)
    return r


# ------------------------------------------------------------------------------------------------ the fp32 yardstick
def dot_f32_fma(a, w, b):
    """a [R, K] . w [K] + b the way the oracle's rfo_linear accumulates it: acc = b, then acc = fmaf(a_k, w_k, acc) for ascending k, every step one
    fp32 rounding (the product of two fp32 values is exact in float64)"""
    a64, w64 = np.asarray(a, F32).astype(np.float64), np.asarray(w, F32).astype(np.float64)
    acc = np.full(a64.shape[0], F32(b), F32)
    for k in range(a64.shape[1]):
        acc = (a64[:, k] * w64[k] + acc.astype(np.float64)).astype(F32)
    return acc


def _lse_seq_f32(v):
    """log-sum-exp along axis 1, sequentially in np.float32: m = max, s += exp(v_j - m) for ascending j, m + log(s) (rfe_oracle.c:557-562)"""
    mx = v.max(axis=1)
    s = np.zeros(v.shape[0], F32)
    for j in range(v.shape[1]):
        s = s + np.exp(v[:, j] - mx)
    return mx + np.log(s)


def yardstick_f32(sim, x, wm, bm, m, n, with_scores=True):
    """The same formulas evaluated plainly and sequentially in np.float32, in the oracle's order (rfe_oracle.c:553-576).  Its distance from
    `reference` is what fp32 costs at these shapes; the GPU bars in tests/tolerances.py are four times that."""
    s = np.ascontiguousarray(np.asarray(sim, F32)[:m, :n])
    b = np.asarray(bm, F32).reshape(-1)[0]
    r = dict(z0=logsigmoid(dot_f32_fma(x[0][:m], wm, b)).astype(F32), z1=logsigmoid(dot_f32_fma(x[1][:n], wm, b)).astype(F32))
    if m == 0 or n == 0:
        return r
    r.update(rowlse=_lse_seq_f32(s), collse=_lse_seq_f32(np.ascontiguousarray(s.T)))
    if with_scores:
        r["scores"] = ((s - r["rowlse"][:, None]) + (s - r["collse"][None, :])) + (r["z0"][:, None] + r["z1"][None, :])
    assert all(v.dtype == F32 for v in r.values())
    return r


def distances(got, ref):
    """max |got - ref| per quantity (z over both sides); quantities either side lacks are left out"""
    d = {}
    for k in ("rowlse", "collse", "scores"):
        if k in got and k in ref and np.size(ref[k]):
            d[k] = float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max())
    zs = [np.abs(np.asarray(got[k], np.float64) - ref[k]).max() for k in ("z0", "z1") if np.size(ref[k])]
    if zs:
        d["z"] = float(max(zs))
    return d


# ------------------------------------------------------------------------------------------------ cases
def _set_logit(tok, wm, target):
    """move component K0 of a token (in place) so that tok . wm + bm = target up to the rounding of that one component"""
    cur = tok.astype(np.float64) @ wm.astype(np.float64) + BM
    tok[K0] = F32(tok[K0] + (target - cur) / float(wm[K0]))


def _make_pair(rng, L, m, n, wm):
    sim = np.empty((L, L), F32)
    ii, jj = np.indices((L, L), sparse=True)
    sim[...] = np.where((ii + jj) % 2 == 0, F32(np.nan), F32(np.inf))                   # everything outside the live block is poison
    x = np.full((2, L, 256), np.nan, F32)                                               # and so is every pad row of x
    meta = dict(m=m, n=n, planted=np.zeros((0, 2), np.int64), col_tie=None, row_tie=None, special=([], []))
    x[0, :m] = rng.standard_normal((m, 256)).astype(F32)
    x[1, :n] = rng.standard_normal((n, 256)).astype(F32)
    if m == 0 or n == 0:
        return sim, x, meta
    live = (3.0 * rng.standard_normal((m, n))).astype(F32)
    free_r, free_c = np.ones(m, bool), np.ones(n, bool)
    ct = rt = None
    if n >= 130:       # identical COLUMNS: exact ties inside a row of the score matrix (the row argmax's rule)
        j0 = int(rng.integers(0, 48))
        cols = [j0 + d for d in TIE_COL_STEPS] + [j0 + 16 * int(rng.integers(1, 4)), n - 1]
        free_c[cols] = False
    if m >= 130:       # identical ROWS: exact ties inside a column (the column kernels' rule, one piece of code per form)
        i0 = int(rng.integers(0, 48))
        rows = [i0 + d for d in TIE_ROW_STEPS] + [m - 1]
        free_r[rows] = False
    if n >= 130:
        r_star = int(rng.choice(np.flatnonzero(free_r)))    # the row whose maximum the tied columns hold
        free_r[r_star] = False
        ct = dict(cols=cols, row=r_star)
    if m >= 130:
        c_star = int(rng.choice(np.flatnonzero(free_c)))    # the column whose maximum the tied rows hold
        free_c[c_star] = False
        rt = dict(rows=rows, col=c_star)
    # planted partial permutation over about half of min(m, n), clear of the tie rows / columns
    fr, fc = np.flatnonzero(free_r), np.flatnonzero(free_c)
    k = min(min(m, n) // 2, len(fr), len(fc))
    pr, pc = np.sort(rng.choice(fr, k, replace=False)), rng.choice(fc, k, replace=False)
    live[pr, pc] += F32(25.0)
    free_r[pr] = False
    free_c[pc] = False
    strong0, strong1 = list(pr), list(pc)
    if ct:
        live[ct["row"], ct["cols"][0]] = F32(20.0)
        strong0.append(ct["row"]); strong1.append(ct["cols"][0])
    if rt:
        live[rt["rows"][0], rt["col"]] = F32(20.0)
        strong0.append(rt["rows"][0]); strong1.append(rt["col"])
    for side, toks in ((0, strong0), (1, strong1)):          # planted tokens are matchable: logit >= 5 (6 .. 8 before the rounding of one component)
        for t in toks:
            _set_logit(x[side, t], wm, 6.0 + 2.0 * rng.random())
    special = []
    for side, free in ((0, free_r), (1, free_c)):            # logits at exactly 0, +-40, +-100 through the one component whose weight is 0.5
        toks = [int(t) for t in rng.permutation(np.flatnonzero(free))[:len(SPECIAL_LOGITS)]]
        for t, v in zip(toks, SPECIAL_LOGITS):
            x[side, t] = 0
            x[side, t, K0] = F32((v - BM) / 0.5)
        special.append(list(zip(toks, SPECIAL_LOGITS)))
    if ct:
        live[:, ct["cols"][1:]] = live[:, [ct["cols"][0]]]
        x[1, ct["cols"][1:]] = x[1, ct["cols"][0]]
    if rt:                                                   # after the columns: the tied rows are identical across the tied columns too
        live[rt["rows"][1:], :] = live[[rt["rows"][0]], :]
        x[0, rt["rows"][1:]] = x[0, rt["rows"][0]]
    sim[:m, :n] = live
    meta.update(planted=np.stack([pr, pc], 1).astype(np.int64), col_tie=ct, row_tie=rt, special=tuple(special))
    return sim, x, meta


def make_case(P, L, lens, seed):
    """sim [P, L, L], x [2, P, L, 256], wm [256], bm [1], lens [2P] (all m, then all n) and one `meta` per pair:
      planted  [k, 2]: sim + 25 on a partial permutation (rows ascending), both tokens with a matchability logit >= 5;
      col_tie  (n >= 130) cols: identical live columns (sim and x), the first one lowest; row: a row whose maximum they hold -> a0[row] must be cols[0];
      row_tie  (m >= 130) rows: identical live rows; col: a column whose maximum they hold -> a1[col] must be rows[0], and a0 of every tied row is col;
      special  per side, (token, logit) with the logit exact.
    Pair p depends on (seed, p, L, lens[p]) alone, so two cases with the same seed share their common pairs."""
    lens = [(int(a), int(b)) for a, b in lens]
    assert len(lens) == P and L % 4 == 0 and all(0 <= a <= L and 0 <= b <= L for a, b in lens)
    wm = (np.random.default_rng([seed, 1 << 20]).standard_normal(256) / 16).astype(F32)
    wm[K0] = 0.5
    sim, x, meta = np.empty((P, L, L), F32), np.empty((2, P, L, 256), F32), []
    for p, (m, n) in enumerate(lens):
        sim[p], xp, mt = _make_pair(np.random.default_rng([seed, p]), L, m, n, wm)
        x[:, p] = xp
        meta.append(mt)
    return dict(P=P, L=L, sim=sim, x=x, wm=wm, bm=np.array([BM], F32), lens=np.array([a for a, _ in lens] + [b for _, b in lens], np.int32), meta=meta)


def _mixed(P, L, named, seed):
    """the named (m, n) first, then seeded lengths: full, just short of full, and anything in [1, L]"""
    rng = np.random.default_rng([seed, P, L])
    out = list(named)
    while len(out) < P:
        out.append(tuple(int(rng.choice([L, L - 1, L - 3, rng.integers(1, L + 1), rng.integers(1, L + 1)])) for _ in range(2)))
    return out


def _full(P, L, named):
    return list(named) + [(L, L)] * (P - len(named))


_SMALL32 = [(0, 32), (32, 0), (0, 0), (5, 31)]
# id: (form, P, L, lens, seed) -- the smallest shapes that reach each form of launch_lg_assign, and both sides of each of its three inequalities:
#   P ceil(L/32) < 128 : 127 x 32 | 128 x 32,  3 x 1000 | 4 x 1000,  1 x 2052 | 2 x 2052,  and 1 x 4096 (= 128) on the far side
#   L <= 1024          : 1 x 1024 | 1 x 1028 among few pairs;  8 x 1024 | 2 x 2052 among many
#   P (L/32) >= 256, L % 32 == 0 : 64 x 128, 16 x 512, 8 x 1024 (= 256 each) | 128 x 32 (= 128);  43 x 100 and 4 x 1000 fail L % 32 alone
CASES = {
    "regs-1x36": ("regs", 1, 36, [(36, 33)], 101),
    "regs-2x200": ("regs", 2, 200, [(1, 200), (200, 1)], 102),
    "regs-1x1024": ("regs", 1, 1024, [(1024, 1021)], 103),
    "regs-3x1000": ("regs", 3, 1000, [(1000, 997), (3, 1000), (640, 70)], 104),
    "regs-3x1024": ("regs", 3, 1024, [(1024, 1024), (1023, 15), (17, 1024)], 105),
    "regs-127x32": ("regs", 127, 32, _mixed(127, 32, _SMALL32, 106), 106),
    "walk-1x1028": ("walk", 1, 1028, [(1028, 1025)], 107),                      # rows past 16 x 64
    "walk-1x2052": ("walk", 1, 2052, [(1500, 2049)], 108),
    "lds-64x128": ("lds", 64, 128, _mixed(64, 128, [(5, 128), (33, 31), (128, 1), (0, 64), (64, 0), (127, 97)], 109), 109),
    "lds-16x512": ("lds", 16, 512, _mixed(16, 512, [(512, 512), (509, 33), (7, 512), (131, 130)], 110), 110),
    "lds-8x1024": ("lds", 8, 1024, _mixed(8, 1024, [(1024, 1024), (1021, 40), (9, 1000), (1000, 9)], 111), 111),
    "32x8-128x32": ("32x8", 128, 32, _mixed(127, 32, _SMALL32, 106) + [(32, 32)], 106),   # regs-127x32 and one pair more
    "32x8-4x1000": ("32x8", 4, 1000, [(1000, 997), (3, 1000), (640, 70), (1000, 1000)], 104),   # regs-3x1000 and one pair more
    "32x8-43x100": ("32x8", 43, 100, _mixed(43, 100, [(100, 100), (1, 100), (100, 1), (0, 7)], 112), 112),
    "32x8-2x2052": ("32x8", 2, 2052, _full(2, 2052, [(2052, 2049)]), 113),
    "32x8-1x4096": ("32x8", 1, 4096, [(4096, 4093)], 114),                      # the one-pair boundary: 1 x 128 stripes is not "few"
}
NO_SCORE_REFERENCE = ("32x8-1x4096",)     # float64 z and log-sum-exps only: the [4096, 4096] float64 score matrix would take the test past a few seconds


@functools.lru_cache(maxsize=3)
def case(cid):
    form, P, L, lens, seed = CASES[cid]
    c = make_case(P, L, lens, seed)
    c.update(id=cid, form=form)
    return c


@functools.lru_cache(maxsize=3)
def case_reference(cid, thr=0.1):
    """`reference` of every pair of a case (computed once per case and threshold, shared by the tests, never modified)"""
    c = case(cid)
    P = c["P"]
    return [reference(c["sim"][p], c["x"][:, p], c["wm"], c["bm"], int(c["lens"][p]), int(c["lens"][P + p]), thr, cid not in NO_SCORE_REFERENCE)
            for p in range(P)]
