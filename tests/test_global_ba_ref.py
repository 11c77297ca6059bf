"""CPU: the contract of DESIGN.md 6n.  tests/global_ba_ref.py against tests/local_ba_ref.py bit for bit where the two contracts meet; its
non-robust quadratic form against a sequential transcription of base_binary_edge.hpp:75-90, one object per vertex and edge; the tiled
solve against the dense one; what the departures cost against g2o's own choices; that it optimises; the forced paths; the refusals; the
exports and the drop-in's compile and link."""
import os

import numpy as np
import pytest

import dropin_driver as DD
import essential_graph_ref as EG
import global_ba_ref as G
import local_ba_ref as LR
import pose_opt_ref as R6
import test_local_ba_ref as TL

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. robust, fixed keyframes last, P <= 64: 6l's bits
@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("F", [0, 1, 3])
@pytest.mark.parametrize("seed", [1, 2])
def test_equals_local_ba_ref(seed, F, kind):
    P = 4 + seed
    c = LR.scene(100 * seed + F, P, F, 40 * seed, kind=kind, gross=0.1)
    a = LR.local_ba(c, c["params"])
    g = G.from_local(c)
    b = G.global_ba(g, g["params"])
    for k in ("pose", "pose_f32"):
        assert np.array_equal(a[k], b[k][:P]), k
    for k in ("point", "point_f32", "chi2", "trace"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["stats"][:4], b["stats"][:4]) and b["stats"][5] == P and b["ret"] == a["stats"][0]
    q = np.asarray(c["kf_pose"], F32)[P:].astype(F64)           # a fixed keyframe's row is its widened, normalised input
    for k in range(F):
        q[k, :4] = R6.normalize_rotation(list(q[k, :4]))
    assert np.array_equal(b["pose"][P:], q)


# ---------------------------------------------------------------- 2. the non-robust quadratic form, lines 75-90 as written
def construct_plain(ed):
    """base_binary_edge.hpp:73-90 with robustKernel() == 0; vertex 0 (`from`, A) the point, vertex 1 (`to`, B) the pose"""
    D, A, B, isg = ed.D, ed.Xi, ed.Xj, ed.isg
    omr = [-(isg * ed.e[r]) for r in range(D)]                  # omega_r = - omega * _error

    def dot(u, v):
        s = u[0] * v[0] + u[1] * v[1]
        return s + u[2] * v[2] if D == 3 else s
    AtO = [[A[k][a] * isg for k in range(D)] for a in range(3)]  # AtO = A.transpose() * omega
    for a in range(3):
        ed.vi.b[a] = ed.vi.b[a] + dot([A[k][a] for k in range(D)], omr)
        for b in range(a, 3):
            ed.vi.H[a][b] = ed.vi.H[a][b] + dot(AtO[a], [A[k][b] for k in range(D)])
    if not ed.vj.fixed:
        for a in range(6):                                       # _hessianTransposed += B.transpose() * AtO.transpose()
            for b in range(3):
                ed.hpl[a][b] = ed.hpl[a][b] + dot([B[k][a] for k in range(D)], AtO[b])
        BtO = [[B[k][a] * isg for k in range(D)] for a in range(6)]
        for a in range(6):
            ed.vj.b[a] = ed.vj.b[a] + dot([B[k][a] for k in range(D)], omr)
            for b in range(a, 6):
                ed.vj.H[a][b] = ed.vj.H[a][b] + dot(BtO[a], [B[k][b] for k in range(D)])


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_plain_quadratic_form_equals_transcription(kind):
    K = 6
    c = G.scene(11, K, [1, 4], G.pattern("dense", K, ppk=5, seed=1), kind)
    S = G.Structure(c)
    L, E = S.L, S.E
    I = LR.edge_inputs({**c, "P": K, "F": 0})
    poses = [TL.VPose(np.asarray(c["kf_pose"], F32)[k], bool(c["fixed"][k])) for k in range(K)]
    points = [TL.VPoint(np.asarray(c["xw"], F32)[p]) for p in range(L)]
    edges = []
    for e in range(E):
        st = bool(I["stereo"][e])
        edges.append(TL.Edge(points[c["edge_point"][e]], poses[c["edge_kf"][e]], [float(I["u"][e]), float(I["v"][e]), float(I["ur"][e])],
                             float(I["isg"][e]), st, [float(I[k][e]) for k in ("fx", "fy", "cx", "cy", "bf")], 0.0, 0.0))
    for v in poses + points:
        v.clear()
    for ed in edges:
        ed.hpl = [[0.0] * 3 for _ in range(6)]
        ed.compute_error()
        ed.linearize()
        construct_plain(ed)
    pose = np.array([v.est for v in poses], F64)
    pt = np.asarray(c["xw"], F32).astype(F64)
    with np.errstate(all="ignore"):
        chi2, rho0, lin = G.edge_linearise(I, None, pose[S.ek, :4], pose[S.ek, 4:], pt[S.ep], False)
    assert np.array_equal(chi2, np.array([ed.chi2() for ed in edges])) and np.array_equal(rho0, chi2)
    pl = LR.seq_sum_groups(lin[:, :9], S.ep, S.pt_rank, L)
    pp = LR.seq_sum_groups(lin[S.fe, 9:36], S.fk, S.pose_rank, S.P)
    ups, up6 = [(a, b) for a in range(3) for b in range(a, 3)], [(a, b) for a in range(6) for b in range(a, 6)]
    for p in range(L):
        assert np.array_equal(pl[p, :6], [points[p].H[a][b] for a, b in ups]) and np.array_equal(pl[p, 6:], points[p].b)
    for i, k in enumerate(S.free_list):
        assert np.array_equal(pp[i, :21], [poses[k].H[a][b] for a, b in up6]) and np.array_equal(pp[i, 21:], poses[k].b)
    for e in S.fe:
        assert np.array_equal(lin[e, 36:].reshape(6, 3), np.array(edges[e].hpl))
    # and it is not the robust form with rho' = 1: the stored block rounds in another order wherever invSigma2 is not 1 (level 0)
    with np.errstate(all="ignore"):
        _, _, lin_r = LR.edge_linearise(I, G.NO_HUBER, pose[S.ek, :4], pose[S.ek, 4:], pt[S.ep])
    assert np.array_equal(lin_r[:, :36], lin[:, :36]) and np.array_equal(lin_r[S.fe, 36:], lin[S.fe, 36:]) == (kind != "mixed")


# ---------------------------------------------------------------- 3. the tiled solve against the dense one
def pattern_matrix(seed, P, blocks):
    """a symmetric positive definite 6 P x 6 P matrix whose 6 x 6 blocks off the diagonal are those listed, and a right-hand side"""
    rng = np.random.default_rng(seed)
    n = 6 * P
    A = np.zeros((n, n))
    for i1, i2 in blocks:
        A[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6] = rng.standard_normal((6, 6))
    A = np.triu(A, 1)
    A = A + A.T + np.diag(40.0 + rng.random(n))
    return A, rng.standard_normal(n)


@pytest.mark.parametrize("name,P,sparse", [("chain", 23, True), ("loop", 23, True), ("star", 22, True), ("hub", 22, False), ("dense", 13, False)])
def test_tiled_solve_equals_dense(name, P, sparse):
    vis = G.pattern(name, P, ppk=1, seed=3)
    blocks = sorted({(a, b) for ks in vis for a in ks for b in ks if a < b})
    A, b = pattern_matrix(5, P, blocks)
    fill, tiles = G.tile_fill([i for i, _ in blocks], [j for _, j in blocks], P)
    NT = fill.shape[0]
    assert (tiles < NT * (NT + 1) // 2) == sparse
    ok, x = G.ldlt_tiled(np.triu(A), b, fill)
    ok6l, x6l = LR.ldlt_dense(A, b)
    ok6m, x6m = EG.ldlt_dense(A, b)
    assert ok and ok6l and ok6m and np.array_equal(x, x6l) and np.array_equal(x, x6m)
    assert np.max(np.abs(A @ x - b)) < 1e-12
    # 6m(g)'s failure rule: a zero pivot, a pivot that is not finite
    for bad in (0.0, np.nan):
        A2 = A.copy()
        A2[7, 7] = bad
        A2[7, 8:] = 0.0
        A2[:7, 7] = 0.0
        with np.errstate(all="ignore"):
            assert G.ldlt_tiled(np.triu(A2), b, fill) == (False, None) and EG.ldlt_dense(A2, b) == (False, None)


# ---------------------------------------------------------------- 4. what the departures cost
def test_departure_cost():
    """the contract, which keeps an edge-less point in the index space, against g2o's own choices on the problem with that point removed
    (sequential global sums, numpy.linalg.solve, numpy.linalg.inv): the largest difference of any pose or point number, measured.  The maxima are recorded in global_ba_ref.DEPARTURE_MAX"""
    worst_pose = worst_point = 0.0
    for seed, K, name, kind, robust in ((201, 6, "dense", "stereo", False), (202, 12, "loop", "mixed", False), (203, 9, "chain", "mono", True),
                                        (204, 10, "star", "mixed", True)):
        c = G.scene(seed, K, [0], G.pattern(name, K, ppk=4, seed=seed), kind, ring=name == "loop", gross=0.1 if robust else 0.0, edgeless=(3,))
        P = G.params(robust=robust)
        keep, removed = G.without_points(c, (3,))
        a, b = G.global_ba(c, P), G.global_ba(removed, P, g2o=True)
        assert np.array_equal(a["stats"][:4], b["stats"][:4]) and a["included"][3] == 0 and np.array_equal(a["point_f32"][3], c["xw"][3])
        worst_pose = max(worst_pose, float(np.max(np.abs(a["pose"] - b["pose"]))))
        worst_point = max(worst_point, float(np.max(np.abs(a["point"][keep] - b["point"]))))
    print("departure cost: pose %.3g point %.3g" % (worst_pose, worst_point))
    assert worst_pose <= 8 * G.DEPARTURE_MAX[0] and worst_point <= 8 * G.DEPARTURE_MAX[1]


# ---------------------------------------------------------------- 5. it optimises
def test_it_optimises():
    """a planted ring of keyframes closed by shared points, one fixed, robust = 0, 10 iterations: the gain in pose and point error
    (measured, global_ba_ref.OPTIMISES_GAIN) of which a sixteenth is asked; currentChi never rises"""
    c = G.optimises_scene()
    r = G.global_ba(c, c["params"])
    out, inp = G.errors_to_truth(c, r)
    gains = [inp[i] / out[i] for i in range(3)]
    print("errors before", inp, "after", out, "gains", gains)
    for g, m in zip(gains, G.OPTIMISES_GAIN):
        assert m > 1 and g >= m / 16
    chi = r["trace"][:r["stats"][0], 2]
    assert np.all(np.diff(chi) <= 0) and r["stats"][6] < r["stats"][7]


# ---------------------------------------------------------------- 6. forced paths
def run_forced(name):
    c = G.forced(name)
    return c, G.global_ba(c, G.run_params(c))


def normalised_input(c):
    q = np.asarray(c["kf_pose"], F32).astype(F64)
    for k in range(len(q)):
        q[k, :4] = R6.normalize_rotation(list(q[k, :4]))
    return q


def test_stop():
    c, r = run_forced("stop")
    assert r["stats"][0] == 0 and r["stats"][4] == (G.FLAG_STOPPED | G.FLAG_NO_ITERATION)
    r0 = G.global_ba(c, G.params(iterations=0))
    for k in ("pose", "point", "chi2"):
        assert np.array_equal(r[k], r0[k])
    c, r = run_forced("stop_after_trial")              # set after the first trial: that iteration is the last
    assert list(r["stats"][:2]) == [1, 1] and r["stats"][4] & G.FLAG_STOPPED
    full = G.global_ba(c, dict(c["params"], stop=False))
    for n in (2, 3):                                   # set after a later trial: the hook is asked after every trial until it says yes
        r = G.global_ba(c, G.run_params(dict(c, params=dict(c["params"], stop=("after", n)))))
        assert list(r["stats"][:2]) == [n, n] and r["stats"][4] & G.FLAG_STOPPED and full["stats"][1] > n
        assert np.array_equal(r["trace"][:n - 1], full["trace"][:n - 1]) and not r["trace"][n:].any()
    c, _ = run_forced("stale")                         # after a rejected trial the inner loop would have gone on: the flag ends it
    r = G.global_ba(c, G.run_params(dict(c, params=dict(c["params"], stop=("after", 1)))))
    assert list(r["stats"][:3]) == [1, 1, 1] and r["stats"][4] == (G.FLAG_STOPPED | G.FLAG_ENDED_REJECTED)


def test_rejected_trials():
    c, r = run_forced("ended_rejected")
    assert list(r["stats"][:3]) == [1, 1, 1] and r["stats"][4] & G.FLAG_ENDED_REJECTED
    assert np.array_equal(r["pose"], normalised_input(c))        # pop: the estimate stays
    c, r = run_forced("stale")
    assert list(r["stats"][:3]) == [1, 2, 2] and r["stats"][4] & G.FLAG_ENDED_REJECTED
    with np.errstate(all="ignore"):
        fresh = G.edge_error(LR.edge_inputs({**c, "P": len(c["fixed"]), "F": 0}), None, r["pose"][c["edge_kf"], :4], r["pose"][c["edge_kf"], 4:],
                             r["point"][c["edge_point"]], False)[2]
    assert not np.array_equal(fresh, r["chi2"])                  # the edges keep the rejected trial's errors


def test_exact_data_ends_on_rho_zero():
    c, r = run_forced("rho_zero")
    assert list(r["stats"][:4]) == [1, 1, 1, 0] and r["trace"][0, 2] == 0.0 and np.array_equal(r["point_f32"], c["xw"])


def test_nan_position():
    c, r = run_forced("nan")
    assert r["stats"][4] & G.FLAG_NONFINITE and r["stats"][4] & G.FLAG_SOLVE_FAILED and r["stats"][3] == r["stats"][1]
    assert np.array_equal(r["pose"], normalised_input(c)) and np.array_equal(r["point"], c["xw"].astype(F64), equal_nan=True)


def test_no_iteration_no_free_pose_no_fixed_pose():
    c, r = run_forced("iterations0")
    assert r["stats"][4] == G.FLAG_NO_ITERATION and np.array_equal(r["pose"], normalised_input(c)) and r["chi2"].any()
    c, r = run_forced("all_fixed")                     # P = 0: nothing to solve, and the points still move
    assert r["stats"][5] == 0 and r["stats"][6] == 0 and r["stats"][7] == 0 and r["stats"][0] >= 1
    assert np.array_equal(r["pose"], normalised_input(c)) and not np.array_equal(r["point_f32"], c["xw"])
    c, r = run_forced("no_fixed")                      # F = 0: every keyframe moves
    assert r["stats"][5] == len(c["fixed"]) and r["stats"][3] == 0
    assert all(not np.array_equal(r["pose"][k], normalised_input(c)[k]) for k in range(len(c["fixed"])))


def test_fixed_keyframe_in_the_middle():
    c, r = run_forced("fixed_middle")
    q = normalised_input(c)
    assert r["stats"][5] == 4 and np.array_equal(r["pose"][[2, 3]], q[[2, 3]])
    assert all(not np.array_equal(r["pose"][k], q[k]) for k in (0, 1, 4, 5))


def test_edgeless_point_and_point_on_fixed_keyframes():
    c, r = run_forced("edgeless")
    sp = c["special"]
    assert r["included"][sp] == 0 and r["included"].sum() == len(c["xw"]) - 2 and np.array_equal(r["point"][sp], c["xw"][sp].astype(F64))
    # its terms in every sum are +0.0.  Under g2o's sequential sums that changes no bit of any other output: the problem without the two
    # points.  The 256-partial sums of 6l(a) regroup when entries leave the middle of the index space, so under the contract the same holds
    # when the edge-less points are the last ones
    keep, d = G.without_points(c, (sp, len(c["xw"]) - 1))
    ra, rb = G.global_ba(c, G.run_params(c), g2o=True), G.global_ba(d, G.run_params(c), g2o=True)
    for k in ("pose", "chi2", "trace", "stats"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(ra["point"][keep], rb["point"])
    L = len(c["xw"])
    c2 = G.scene(89, len(c["fixed"]), [0], G.pattern("dense", len(c["fixed"]), ppk=8, seed=3), edgeless=(L - 2, L - 1))
    keep, d = G.without_points(c2, (L - 2, L - 1))
    ra, rb = G.global_ba(c2, G.params()), G.global_ba(d, G.params())
    for k in ("pose", "chi2", "trace", "stats"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(ra["point"][keep], rb["point"]) and ra["included"][-2:].sum() == 0
    c, r = run_forced("fixed_only")
    sp = c["special"]
    assert r["included"][sp] == 1 and not np.array_equal(r["point_f32"][sp], c["xw"][sp])


def test_huber_parameters():
    """5.99 is not LocalBundleAdjustment's 5.991: the parameter reaches the kernel"""
    c, r = run_forced("robust")
    r2 = G.global_ba(c, G.params(robust=True, huber2_mono=5.991))
    r3 = G.global_ba(c, G.params(robust=False))
    assert not np.array_equal(r["pose"], r2["pose"]) and not np.array_equal(r["pose"], r3["pose"])
    assert G.huber(5.99)[0] == F64(F32(np.sqrt(5.99)))


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    K = 5
    base = G.scene(10, K, [0], G.pattern("dense", K, ppk=6, seed=5))
    n = len(base["edge_point"])
    ep, ek = base["edge_point"].copy(), base["edge_kf"].copy()
    ep[[4, 5]], ek[[4, 5]] = ep[[5, 4]], ek[[5, 4]]
    at = lambda i, v, a: np.where(np.arange(n) == i, v, a).astype(np.int32)
    off = base["kf_feat_off"].copy()
    off[2] = off[1] - 1
    bad = [dict(base, edge_point=ep, edge_kf=ek), dict(base, edge_kf=at(1, base["edge_kf"][0], base["edge_kf"])),
           dict(base, edge_point=at(n - 1, len(base["xw"]), base["edge_point"])), dict(base, edge_kf=at(n - 1, K, base["edge_kf"])),
           dict(base, edge_feat=at(3, 1 << 20, base["edge_feat"])), dict(base, edge_feat=at(3, -1, base["edge_feat"])),
           dict(base, kf_feat_off=off), dict(base, kf_nlevels=np.full(K, 17, np.int32)), dict(base, fixed=np.zeros(0, np.uint8)),
           dict(base, fixed=np.zeros(G.MAX_KF + 1, np.uint8)), dict(base, xw=np.zeros((G.MAX_POINTS + 1, 3), F32)),
           dict(base, edge_point=np.zeros(G.MAX_EDGES + 1, np.int32), edge_kf=np.zeros(G.MAX_EDGES + 1, np.int32),
                edge_feat=np.zeros(G.MAX_EDGES + 1, np.int32))]
    for c in bad:
        with pytest.raises(G.Invalid):
            G.global_ba(c, G.params())
    for P in (G.params(iterations=-1), G.params(iterations=65), G.params(max_trials=-1), G.params(huber2_mono=np.nan),
              G.params(huber2_stereo=np.inf), G.params(user_lambda_init=np.nan)):
        with pytest.raises(G.Invalid):
            G.global_ba(base, P)
    # the pair cap, counted from the edge table before anything is built: 520 free keyframes all seeing 250 points are 33.9 million pairs
    big = G.over_pairs_case()
    assert G.schur_pairs(big) == 250 * 520 * 521 // 2 > G.MAX_PAIRS and len(big["edge_point"]) <= G.MAX_EDGES
    with pytest.raises(G.Invalid, match="pairs"):
        G.global_ba(big, big["params"])
    small = G.scene(10, K, [0, 2], G.pattern("dense", K, ppk=6, seed=5))
    assert G.schur_pairs(small) == G.Structure(small).n_pairs          # the count is the number of pairs the structure holds


# ---------------------------------------------------------------- 8. the exports and the drop-in's compile and link
def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "rover_fe.h")).read()
    for name in ("rfe_global_ba_dev(", "rfe_global_ba(", "rfe_global_ba_params"):
        assert name in hdr
    for macro, v in (("RFE_GBA_MAX_KF", "1024"), ("RFE_GBA_MAX_POINTS", "(1 << 18)"), ("RFE_GBA_MAX_EDGES", "(1 << 21)"),
                     ("RFE_GBA_MAX_ITERATIONS", "64"), ("RFE_GBA_MAX_PAIRS", "(1 << 25)")):
        assert "#define %s %s\n" % (macro, v) in hdr
    assert (G.MAX_KF, G.MAX_POINTS, G.MAX_EDGES, G.MAX_ITERATIONS, G.MAX_PAIRS) == (1024, 1 << 18, 1 << 21, 64, 1 << 25)
    src = open(os.path.join(ROOT, "rover-slam_amd", "capi.py")).read()
    assert '"rfe_global_ba", "rfe_global_ba_dev"' in src and "class GlobalBaParams" in src
    from rover_slam_amd import capi
    assert (capi.GBA_MAX_KF, capi.GBA_MAX_POINTS, capi.GBA_MAX_EDGES, capi.GBA_MAX_PAIRS, capi.GBA_TILE_V) == (G.MAX_KF, G.MAX_POINTS, G.MAX_EDGES,
                                                                                                               G.MAX_PAIRS, G.TILE_V)
    for sym in ("rfe_global_ba", "rfe_global_ba_dev"):
        assert sym in capi.EXPORTS and getattr(capi.lib, sym)
    kmk = open(os.path.join(ROOT, "rover-slam_amd", "csrc", "Makefile")).read()
    assert " global_ba.hip" in kmk and "api_global_ba.hip" in kmk


def test_dropin_compiles_and_links(tmp_path):
    """include/rfe/global_ba.h over the stand-ins of tests/cpp/global_ba_driver.cpp, -std=c++14 -Wall -Werror, linked against the library;
    the run with no case file touches no device"""
    exe = DD.build(tmp_path, "global_ba_driver")
    DD.run(exe)
