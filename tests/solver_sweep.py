"""The randomised sweep of the seven device-resident solver stages: draw(stage, seed) is the list of cases of one (stage, seed), a pure
function of the two, built from each stage's own generator (scene / graph / pattern / params of the *_ref.py modules) and stacked, padded
and poisoned by the helpers of that stage's tests/test_gpu_<stage>.py.  Shared by test_gpu_solver_sweep.py (kernel against restatement,
exact) and test_solver_sweep_draws.py (CPU: the draws are not tame).

A case is one call of the entry: a dict with `tag` (one line that rebuilds it: `solver_sweep.draw(stage, seed)[k]` plus what was drawn),
`stage`, and what reference() / forms() / check() need.  A batched stage's case holds B problems.  The sizes are the smallest at which
each kernel's structure changes (lanes, waves, chunks, tiles, one workgroup's rows), not the workload's; every size list is covered over
the four seeds by construction: seed s takes every fourth value from the s-th on and places them at random among its problems, the
rest is drawn.  Nothing here is redrawn until it "looks good"."""
import numpy as np

import essential_graph_ref as EG
import global_ba_ref as GB
import local_ba_ref as LB
import optimize_sim3_ref as OS
import pose_opt_ref as PO
import sim3_solver_ref as S3
import two_view_ref as TV

STAGES = ("pose_opt", "optimize_sim3", "sim3_solver", "two_view", "local_ba", "global_ba", "essential_graph")
SEEDS = (0, 1, 2, 3)
# calls per (stage, seed): as many as fit in a few seconds of one pytest case, restatement included (profiles/solver_sweep.md)
CALLS = {"pose_opt": 12, "optimize_sim3": 6, "sim3_solver": 12, "two_view": 6, "local_ba": 12, "global_ba": 12, "essential_graph": 12}
# per problem sizes; a pair is a uniform draw in lo .. hi
SIZES = {"pose_opt": (0, 1, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, (258, 600)),
         "optimize_sim3": (0, 1, 9, 10, 11, 255, 256, 257, (258, 500)),
         "sim3_solver": (0, 2, 3, 4, 63, 64, 65, 257, (258, 400)),
         "two_view": (8, 9, 63, 64, 65, 100, 257),
         "local_ba.P": (0, 1, 2, 10, 11, 42, 43, 63, 64),           # 6 P against the 256 threads of lba_ldlt_kernel: 252, 258
         "local_ba.L": (0, 1, 5, 85, 86, 255, 256, 257, 300),       # 3 L: 255, 258
         # K in 2 .. 70 and N in 1 .. 40: both ends, the small counts, and either side of the 64 free poses of rfe_local_ba's workgroup
         "global_ba": (2, 3, 5, 8, 9, (10, 40), (41, 63), 64, 65, 66, (67, 69), 70),
         "essential_graph": (1, 2, 3, 4, 5, 6, 9, 13, (14, 29), (30, 39), 40)}
MAX_B = {"pose_opt": 12, "optimize_sim3": 20, "sim3_solver": 20, "two_view": 16}
# the B of a seed's first calls: past one launch's chunk (OS_CHUNK = 8: three launches, then two, each with a partial last chunk;
# S3_FRONT_CHUNK = 16: two launches); pose_opt and two_view run every problem in one launch, there it is the upper end of the range
FIRST_B = {"pose_opt": ((9, 12),), "optimize_sim3": ((17, 20), (9, 15)), "sim3_solver": ((17, 20),), "two_view": ((16, 16),)}
TV_KINDS = ("general", "plane", "rotation", "low_parallax")
GB_PATTERNS = ("chain", "loop", "star", "hub", "dense", "pairs5")
EG_KINDS = ("chain", "star", "arrowhead")


def _mods():
    """the stages' GPU test modules, for their batch / padded / host / dev / both helpers; imported late: they are test files"""
    import test_gpu_essential_graph as eg
    import test_gpu_global_ba as gb
    import test_gpu_local_ba as lb
    import test_gpu_optimize_sim3 as osim
    import test_gpu_pose_opt as po
    import test_gpu_sim3_solver as s3
    import test_gpu_two_view as tv
    return {"pose_opt": po, "optimize_sim3": osim, "sim3_solver": s3, "two_view": tv, "local_ba": lb, "global_ba": gb, "essential_graph": eg}


def _size(rng, v):
    return int(rng.integers(v[0], v[1] + 1)) if isinstance(v, tuple) else int(v)


def _sizes(rng, key, seed, count, large=0.5):
    """`count` sizes: the seed's share of SIZES[key] at random positions; of the rest, a share `large` from the upper half of the list"""
    vals = SIZES[key]
    out = [_size(rng, v) for v in vals[seed % 4::4]][:count]
    half = len(vals) // 2
    while len(out) < count:
        pick = vals[half + int(rng.integers(0, len(vals) - half))] if rng.random() < large else vals[int(rng.integers(0, len(vals)))]
        out.append(_size(rng, pick))
    return [out[i] for i in rng.permutation(count)]


def _batches(rng, stage, calls):
    Bs = [int(rng.integers(lo, hi + 1)) for lo, hi in FIRST_B[stage]][:calls]
    return Bs + [int(rng.integers(1, MAX_B[stage] + 1)) for _ in range(calls - len(Bs))]


def _split(sizes, Bs):
    out, at = [], 0
    for B in Bs:
        out.append(sizes[at:at + B])
        at += B
    return out


# ---------------------------------------------------------------- the draws, one function per stage
def _draw_pose_opt(rng, seed, calls):
    Bs = _batches(rng, "pose_opt", calls)
    cases = []
    for k, ns in enumerate(_split(_sizes(rng, "pose_opt", seed, sum(Bs), large=0.7), Bs)):
        sub = int(rng.integers(0, 1 << 30))
        kinds = [str(rng.choice(("mono", "stereo", "mixed"))) for _ in ns]
        its = tuple(int(v) for v in rng.integers(1, 7, 4)) if rng.random() < 0.5 else (0, 0, 0, 0)
        mt = int(rng.choice((0, 0, 1, 2, 3)))
        pad = 0 if k == seed else int(rng.integers(1, 41))   # one call per seed without a spare row
        octave, uright = bool(rng.random() < 0.75), bool(rng.random() < 0.75)
        scenes = [PO.scene(sub + b, n, kd, has=1.0 if n < 20 else 0.9) for b, (n, kd) in enumerate(zip(ns, kinds))]
        cases.append({"P": dict(scenes[0]["P"], iterations=its, max_trials=mt), "scenes": scenes, "N": max(ns) + pad, "octave": octave,
                      "uright": uright, "poison_seed": sub & 0xFFFF,
                      "tag": f"n={ns} kinds={kinds} iterations={its} max_trials={mt} N={max(ns) + pad} octave={octave} uright={uright}"})
    return cases


def _draw_optimize_sim3(rng, seed, calls):
    Bs = _batches(rng, "optimize_sim3", calls)
    cases = []
    for ns in _split(_sizes(rng, "optimize_sim3", seed, sum(Bs), large=0.6), Bs):
        sub = int(rng.integers(0, 1 << 30))
        flags = [(bool(rng.random() < 0.4), bool(rng.random() < 0.5), bool(rng.random() < 0.7), int(rng.choice((0, 0, 1, 2)))) for _ in ns]
        padN, padN2 = (int(v) for v in rng.choice(np.arange(1, 40), 2, replace=False))
        scenes = []
        for b, (n, (fs, mx, ap, mt)) in enumerate(zip(ns, flags)):
            c = OS.scene(sub + b, n, fix_scale=fs, mixed=mx, pixel=False, all_points=ap)
            c["P"] = dict(c["P"], max_trials=mt)
            scenes.append(c)
        cases.append({"scenes": scenes, "N": max(ns) + padN, "N2": max(ns) + padN2,
                      "tag": f"n={ns} (fix_scale, mixed, all_points, max_trials)={flags} N={max(ns) + padN} N2={max(ns) + padN2}"})
    return cases


def _draw_sim3_solver(rng, seed, calls):
    Bs = _batches(rng, "sim3_solver", calls)
    long_at = int(rng.integers(0, sum(Bs)))                   # the seed's one problem with 300 hypotheses
    cases, at = [], 0
    for ns in _split(_sizes(rng, "sim3_solver", seed, sum(Bs), large=0.6), Bs):
        sub = int(rng.integers(0, 1 << 30))
        scenes, spec = [], []
        for b, n in enumerate(ns):
            its = 300 if at == long_at else int(rng.integers(1, 41))
            at += 1
            fs, share = bool(rng.random() < 0.4), float(rng.choice((0.0, 0.2, 0.4, 0.6)))
            # min_inliers: the scene's own (three quarters of the planted inliers: a good hypothesis passes it), one above every
            # count (no hypothesis passes: all `its` run), or 3
            mn = (None, n, 3)[int(rng.choice((0, 0, 1, 2)))]
            scenes.append(S3.scene(sub + b, n, outliers=share, its=its, min_inliers=mn, fix_scale=fs))
            spec.append((its, fs, share, scenes[-1]["P"]["min_inliers"]))
        padN, padH = int(rng.integers(0, 9)), int(rng.integers(0, 5))
        N, H = max(ns) + padN, min(max(s[0] for s in spec) + padH, 1024)
        cases.append({"scenes": scenes, "N": N, "H": H, "tag": f"n={ns} (its, fix_scale, outliers, min_inliers)={spec} N={N} H={H}"})
    return cases


def _draw_two_view(rng, seed, calls):
    Bs = _batches(rng, "two_view", calls)
    long_at = int(rng.integers(0, sum(Bs)))                   # the seed's one problem with its = 0, which means 200
    cases, at = [], 0
    for ns in _split(_sizes(rng, "two_view", seed, sum(Bs), large=0.6), Bs):
        sub = int(rng.integers(0, 1 << 30))
        scenes, spec = [], []
        for b, n in enumerate(ns):
            its = 0 if at == long_at else int(rng.integers(1, 25))
            at += 1
            kind = TV_KINDS[int(rng.choice((0, 0, 0, 1, 1, 2, 3)))]
            e1, e2 = (int(v) for v in rng.choice(np.arange(1, 40), 2, replace=False))
            sigma = float(rng.choice((0.0, 1.0, 1.5)))
            # the default of 50 triangulated points is out of reach of the small sizes: half the problems ask for n / 4
            mt = 0 if rng.random() < 0.5 else max(n // 4, 1)
            scenes.append(TV.scene(sub + b, n, kind=kind, its=its, extra1=e1, extra2=e2, sigma=sigma, min_triangulated=mt))
            spec.append((kind, its, e1, e2, sigma, mt))
        pad = tuple(int(v) for v in rng.integers(0, 8, 4))
        cases.append({"scenes": scenes, "pad": pad, "tag": f"n={ns} (kind, its, extra1, extra2, sigma, min_triangulated)={spec} pad={pad}"})
    return cases


def _draw_local_ba(rng, seed, calls):
    Ps, Ls = _sizes(rng, "local_ba.P", seed, calls), _sizes(rng, "local_ba.L", seed, calls)
    cases = []
    for P, L in zip(Ps, Ls):
        sub = int(rng.integers(0, 1 << 30))
        F = int(rng.integers(1 if P == 0 else 0, 6))
        kind, gross = str(rng.choice(("mono", "stereo", "mixed"))), float(rng.choice((0.0, 0.1, 0.2)))
        its, mt = int(rng.integers(1, 5)), int(rng.choice((0, 0, 1, 2)))
        all_see = bool(L <= 5 and rng.random() < 0.5)
        # one case per seed starts far off with a Gauss-Newton-sized first step (6l's forced "one_trial"): rejected trials
        far = len(cases) == seed % calls
        rot, trans, noise, lam = (1.0, 2.0, 2.0, 1e-9) if far else (0.02, 0.05, 0.05, 0.0)
        c = LB.scene(sub, P, F, L, kind=kind, gross=gross, all_see=all_see, rot=rot, trans=trans, pt_noise=noise)
        c["params"] = LB.params(iterations=its, max_trials=mt, user_lambda_init=lam)
        cases.append({"c": c, "tag": f"P={P} F={F} L={L} kind={kind} gross={gross} iterations={its} max_trials={mt} all_see={all_see} rot={rot}"})
    return cases


def _draw_global_ba(rng, seed, calls):
    cases = []
    names = [GB_PATTERNS[(seed + k) % len(GB_PATTERNS)] for k in range(calls)]      # every name within two seeds
    Ks = _sizes(rng, "global_ba", seed, calls)
    for k, name in enumerate(names):
        sub = int(rng.integers(0, 1 << 30))
        K = max(Ks[k], 5) if name == "pairs5" else Ks[k]
        ppk = int(rng.integers(1, 7)) * (10 if name == "pairs5" else 1)
        fixed = sorted(int(v) for v in rng.choice(K, min(int(rng.integers(0, 4)), K), replace=False))
        ring, robust = bool(name == "loop" or rng.random() < 0.3), bool(rng.random() < 0.5)
        its, mt, kind = int(rng.integers(1, 5)), int(rng.choice((0, 0, 1, 2))), str(rng.choice(("mono", "stereo", "mixed")))
        # one case per seed starts far off with a Gauss-Newton-sized first step (6n's forced "ended_rejected"): rejected trials
        far = k == seed % calls
        rot, trans, noise, lam = (1.0, 2.0, 2.0, 1e-9) if far else (0.02, 0.05, 0.05, 0.0)
        c = GB.scene(sub, K, fixed, GB.pattern(name, K, ppk=ppk, seed=sub & 0xFF), kind, ring=ring, gross=0.1 if robust else 0.0, rot=rot, trans=trans,
                     pt_noise=noise)
        c["params"] = GB.params(iterations=its, max_trials=mt, user_lambda_init=lam, robust=robust)
        cases.append({"c": c, "tag": f"pattern={name} K={K} ppk={ppk} fixed={fixed} ring={ring} robust={robust} kind={kind} iterations={its} "
                                     f"max_trials={mt} rot={rot}"})
    return cases


def _draw_essential_graph(rng, seed, calls):
    cases = []
    Ns = _sizes(rng, "essential_graph", seed, calls)
    for k, N in enumerate(Ns):
        sub = int(rng.integers(0, 1 << 30))
        kind = EG_KINDS[(seed + k) % 3]
        band, loops = int(rng.integers(0, min(N, 5))), int(rng.integers(0, N // 2 + 1) if N < 8 else rng.integers(0, 4))
        corrected, dup = int(rng.integers(0, min(N, 4))), int(rng.integers(0, 7))
        fixed = (None, 0, int(rng.integers(0, N)))[int(rng.choice((0, 1, 2, 2)))]
        shuffle, fs = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
        L = int(rng.choice((0, 1, 257)))
        # a converged run ends on the noise of the numeric Jacobian, in rejected trials: one case in three runs that long
        its, mt = (int(rng.integers(1, 5)), int(rng.choice((0, 1, 2)))) if k % 3 else (12, 2)
        lam = float(rng.choice((1e-16, 0.0)))
        drift = float(rng.choice((0.01, 0.05)))
        c = EG.graph(sub, N, kind=kind, band=band, loops=loops, fixed=fixed, drift=drift, dscale=0.0 if fs else 0.005, corrected=corrected, L=L, dup=dup,
                     shuffle=shuffle)
        cases.append({"c": c, "P": EG.params(iterations=its, max_trials=mt, user_lambda_init=lam, fix_scale=fs),
                      "tag": f"N={N} kind={kind} band={band} loops={loops} fixed={fixed} corrected={corrected} dup={dup} shuffle={shuffle} "
                             f"fix_scale={fs} L={L} iterations={its} max_trials={mt} lambda={lam} drift={drift}"})
    return cases


_DRAW = {"pose_opt": _draw_pose_opt, "optimize_sim3": _draw_optimize_sim3, "sim3_solver": _draw_sim3_solver, "two_view": _draw_two_view,
         "local_ba": _draw_local_ba, "global_ba": _draw_global_ba, "essential_graph": _draw_essential_graph}
_DRAWN = {}


def draw(stage, seed, calls=None):
    """the cases of one (stage, seed); built once per process, and left unchanged by everything that uses them"""
    key = (stage, seed, calls)
    if key not in _DRAWN:
        rng = np.random.default_rng([STAGES.index(stage), seed])
        cases = _DRAW[stage](rng, seed, CALLS[stage] if calls is None else calls)
        for k, c in enumerate(cases):
            c["stage"] = stage
            c["tag"] = f"solver_sweep.draw({stage!r}, {seed})[{k}]: {c['tag']}"
            _stack(c)
        _DRAWN[key] = cases
    return _DRAWN[key]


# ---------------------------------------------------------------- a case through the stage's own helpers
def _stack(case):
    """the arrays of a batched stage's call, by the stage's own batch()"""
    T, st = _mods()[case["stage"]], case["stage"]
    if st == "pose_opt":
        case["a"] = T.batch(case["scenes"], N=case["N"], seed=case["poison_seed"])
    elif st == "optimize_sim3":
        case["a"] = T.batch(case["scenes"], N=case["N"], N2=case["N2"])
    elif st == "sim3_solver":
        case["a"] = T.batch(case["scenes"], N=case["N"], H=case["H"])
    elif st == "two_view":
        case["a"] = T.batch(case["scenes"], pad=case["pad"])


def problems(case):
    return len(case["scenes"]) if "scenes" in case else 1


def reference(case):
    """the restatement's result of a case, computed once"""
    if "ref" in case:
        return case["ref"]
    T, st = _mods()[case["stage"]], case["stage"]
    if st == "pose_opt":
        a = case["a"]
        eff = dict(a, octave=a["octave"] if case["octave"] else np.zeros_like(a["octave"]),
                   uright=a["uright"] if case["uright"] else np.full_like(a["uright"], -1))
        ref = T.reference(case["P"], eff)
    elif st in ("optimize_sim3", "sim3_solver", "two_view"):
        ref = T.reference(case["a"])
    elif st == "local_ba":
        ref = LB.local_ba(case["c"], case["c"]["params"])
    elif st == "global_ba":
        ref = GB.global_ba(case["c"], GB.run_params(case["c"]))
    else:
        ref = EG.essential_graph(case["c"], case["P"])
    case["ref"] = ref
    return ref


def forms(ctx, case):
    """(host, dev): two functions without arguments that run the case through rfe_<stage> and rfe_<stage>_dev on ctx and return the
    outputs"""
    T, st = _mods()[case["stage"]], case["stage"]
    if st == "pose_opt":
        kw = dict(octave=case["octave"], uright=case["uright"])
        return (lambda: T.host(ctx, case["P"], case["a"], **kw)), (lambda: T.dev(ctx, case["P"], case["a"], **kw))
    if st in ("optimize_sim3", "sim3_solver", "two_view"):
        return (lambda: T.host(ctx, case["a"])), (lambda: T.dev(ctx, case["a"]))
    if st in ("local_ba", "global_ba"):
        return (lambda: T.host(ctx, case["c"])), (lambda: T.dev(ctx, case["c"]))
    return (lambda: T.host(ctx, case["c"], case["P"])), (lambda: T.dev(ctx, case["c"], case["P"]))


def compare(case, got, ref, form):
    """every output exactly equal, by the stage's own same(); the message carries the case's tag"""
    T, st = _mods()[case["stage"]], case["stage"]
    try:
        if st in ("local_ba", "global_ba", "essential_graph"):
            T.same(got, ref, T.REQUIRED + T.OPTIONAL)
            assert got["ret"] == ref["ret"], ("ret", got["ret"], ref["ret"])
        else:
            T.same(got, ref)
    except AssertionError as e:
        raise AssertionError(f"{case['tag']} [{form} form]: {e}") from e


def check(ctx, case):
    """host form and _dev form of one case against the restatement"""
    ref = reference(case)
    for form, run in zip(("host", "dev"), forms(ctx, case)):
        try:
            got = run()
        except AssertionError as e:                           # a guard word of the stage's dev()
            raise AssertionError(f"{case['tag']} [{form} form]: {e}") from e
        compare(case, got, ref, form)


# ---------------------------------------------------------------- what a case did, for test_solver_sweep_draws.py
def outcomes(case):
    """per problem of a batched stage: True for the stage's success exit.  pose_opt: all four rounds ran and the pose is finite;
    optimize_sim3: both rounds ran (no early exit) with inliers left; sim3_solver: a hypothesis passed min_inliers; two_view:
    reconstructed"""
    ref, st = reference(case), case["stage"]
    s = ref["stats"]
    if st == "pose_opt":
        return [bool(r[3] == 4 and not r[7] & (PO.FLAG_SOLVE_FAILED | PO.FLAG_NONFINITE)) for r in s]
    if st == "optimize_sim3":
        return [bool(r[3] == 2 and r[0] > 0 and not r[7] & (OS.FLAG_EARLY | OS.FLAG_NONFINITE)) for r in s]
    if st == "sim3_solver":
        return [bool(r[0] == 1) for r in s]
    if st == "two_view":
        return [bool(r[0] == 1 and r[11] == TV.EXIT_OK) for r in s]
    raise KeyError(st)


def steps(case):
    """(accepted, rejected) LM trials of a graph stage's case"""
    s = reference(case)["stats"]
    return int(s[1]) - int(s[2]), int(s[2])
