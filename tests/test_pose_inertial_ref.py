"""CPU: the numpy restatement of PoseInertialOptimizationLastKeyFrame / LastFrame (tests/pose_inertial_ref.py, the contract of DESIGN.md
6p) -- its building blocks against numpy's own (eigh, svd, inv, libm), its Jacobians against central differences of errors stated on
their own, a planted scene in both modes and over a chain of frames that hand the prior on, and every forced path by stats and by the
branches taken."""
import os
import shutil

import numpy as np
import pytest

import dropin_driver as DD
import pose_inertial_ref as R
import pose_inertial_seq as Q

F32, F64 = np.float32, np.float64
KF, LF = R.MODE_LAST_KEYFRAME, R.MODE_LAST_FRAME
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the stated replacements against numpy's own
@pytest.mark.parametrize("n", [3, 9, 15])
def test_jacobi_against_eigh(n):
    rng = np.random.default_rng(n)
    for scale in (1e-6, 1.0, 1e9):
        M = rng.standard_normal((n, n))
        M = (M @ M.T - 0.3 * np.eye(n)) * scale              # indefinite
        lam, V = R.jacobi_eig(M, n)
        assert np.abs(np.sort(lam) - np.linalg.eigvalsh(M)).max() <= 1e-13 * np.abs(lam).max()
        assert np.abs(R.recompose(V, lam) - M).max() <= 1e-13 * np.abs(M).max() and np.abs(V.T @ V - np.eye(n)).max() <= 1e-14 * n
    # only the lower triangle is read
    M2 = M.copy(); M2[np.triu_indices(n, 1)] = 77.0
    assert np.array_equal(R.jacobi_eig(M2, n)[0], lam)


def test_nearest_rotation_against_svd():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A = R._rot(rng.standard_normal(3)) + rng.standard_normal((3, 3)) * 1e-3
        U, _, Vt = np.linalg.svd(A)
        assert np.abs(R.nearest_rotation(A) - U @ Vt).max() <= 1e-15 * 8


def test_inverses_against_inv():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((3, 3))
    assert np.abs(R.inv3(A) - np.linalg.inv(A)).max() <= 1e-13 * np.abs(np.linalg.inv(A)).max()
    M = rng.standard_normal((9, 9))
    C = M @ M.T + np.eye(9)
    assert np.abs(R.ldlt_inverse(C, 9) - np.linalg.inv(C)).max() <= 1e-13 * np.abs(np.linalg.inv(C)).max()
    pre = R.unpack_preint(R.scene(3, 10, KF)["args"]["preint"])     # a covariance of the size the scenes use
    Cd = pre["C"].astype(F64)
    assert np.abs(R.ldlt_inverse(Cd, 9) @ Cd - np.eye(9)).max() <= 1e-9


def test_ldlt_solve_against_solve():
    rng = np.random.default_rng(3)
    for D in (15, 30):
        M = rng.standard_normal((D, D))
        H = M @ M.T + np.eye(D)
        b = rng.standard_normal(D)
        ok, x = R.ldlt_solve(H, b, D)
        assert ok and np.abs(x - np.linalg.solve(H, b)).max() <= 1e-10 * np.abs(x).max()
        H[4, 4] = -1e6                                         # a negative pivot: not positive
        assert R.ldlt_solve(H, b, D) == (False, None)


def test_so3_against_libm():
    rng = np.random.default_rng(4)
    for mag in (1e-7, 1e-3, 0.5, 3.0):
        w = rng.standard_normal(3); w = w / np.linalg.norm(w) * mag
        E = R.exp_so3(w)
        assert np.abs(E - R._rot(w)).max() <= 1e-14 and np.abs(R.log_so3(E) - w).max() <= 1e-9 * max(mag, 1e-3)
        Jr, iJr = R.right_jacobian(w), R.inv_right_jacobian(w)
        assert np.abs(Jr @ iJr - np.eye(3)).max() <= 1e-12
        # Sophus::SO3f::exp in float against the double rotation
        assert np.abs(R.so3f_exp_matrix(w.astype(F32)).astype(F64) - R._rot(w.astype(F32).astype(F64))).max() <= 4e-7
    for x in (-1.0, -0.7, -0.2, 0.0, 1e-20, 0.3, 0.9, 1.0 - 1e-12, 1.0):
        assert abs(float(R.acos(x)) - np.arccos(x)) <= 4e-16 * max(np.arccos(x), 1e-8) + 1e-300 or x == 1.0 and R.acos(x) == 0.0
    assert np.isnan(R.acos(1.0 + 1e-12))


# ---------------------------------------------------------------- Jacobians against central differences of errors stated on their own
def _oplus_pose(st, d):
    """VertexPose::oplusImpl on a copy: twb += Rwb d[3:6], Rwb = Rwb Exp(d[0:3]) (libm's rotation)"""
    out = {k: np.array(v, F64) for k, v in st.items()}
    out["twb"] = st["twb"] + st["Rwb"] @ d[3:6]
    out["Rwb"] = st["Rwb"] @ R._rot(d[0:3])
    return out


def _log(Rm):
    w = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]]) / 2
    s = np.linalg.norm(w)
    return w if s < 1e-12 else w * np.arctan2(s, (np.trace(Rm) - 1) / 2) / s


def _inertial_error(pre, prev, cur):
    """EdgeInertial's error written from its definition, in double: the bias-corrected deltas with libm's rotation"""
    dt, g = float(pre["dT"]), np.array([0, 0, -float(R.GRAVITY)])
    dbg, dba = prev["bg"] - pre["bg"].astype(F64), prev["ba"] - pre["ba"].astype(F64)
    c = {k: pre[k].astype(F64) for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa")}
    dR = c["dR"] @ R._rot(c["JRg"] @ dbg)
    dV = c["dV"] + c["JVg"] @ dbg + c["JVa"] @ dba
    dP = c["dP"] + c["JPg"] @ dbg + c["JPa"] @ dba
    R1 = prev["Rwb"]
    return np.concatenate([_log(dR.T @ R1.T @ cur["Rwb"]), R1.T @ (cur["v"] - prev["v"] - g * dt) - dV,
                           R1.T @ (cur["twb"] - prev["twb"] - prev["v"] * dt - 0.5 * g * dt * dt) - dP])


def _states(seed, dT):
    c = R.scene(seed, 10, LF, dT=dT)
    a = c["args"]
    return R.unpack_preint(a["preint"]), R.unpack_state(a["prev_state"]), R.unpack_state(a["state"]), a


def _fd(err, prev, cur, h=1e-6):
    """central differences over VPk 6, VVk 3, VGk 3, VAk 3, VP 6, VV 3"""
    cols = []
    for which, st in (("prev", prev), ("cur", cur)):
        keys = [("pose", i) for i in range(6)] + [("v", i) for i in range(3)] + ([("bg", i) for i in range(3)] + [("ba", i) for i in range(3)]
                                                                                 if which == "prev" else [])
        for key, i in keys:
            es = []
            for sgn in (1.0, -1.0):
                d = np.zeros(6 if key == "pose" else 3); d[i] = sgn * h
                s2 = _oplus_pose(st, d) if key == "pose" else dict(st, **{key: st[key] + d})
                es.append(err(s2, cur) if which == "prev" else err(prev, s2))
            cols.append((es[0] - es[1]) / (2 * h))
    return np.stack(cols, 1)


@pytest.mark.parametrize("dT", [0.05, 0.5])
def test_inertial_jacobian_against_central_differences(dT):
    pre, prev, cur, _ = _states(5, dT)
    prev["bg"] = prev["bg"] + np.array([2e-3, -1e-3, 1.5e-3])      # a bias estimate away from the preintegration's
    e, J = R.inertial_edge(pre, prev, cur)
    e0 = _inertial_error(pre, prev, cur)
    assert np.abs(e - e0).max() <= 2e-6                               # the float bias correction against the double one
    fd = _fd(lambda p, c: _inertial_error(pre, p, c), prev, cur)
    gap = np.abs(J - fd)
    scale = np.abs(fd).max()
    # the exact blocks; d er / d bg (rows 0:3, columns 9:12) is first order in the bias change
    exact = np.ones((9, 24), bool); exact[0:3, 9:12] = False
    assert gap[exact].max() <= 2e-6 * scale, gap[exact].max() / scale
    g_bg = gap[0:3, 9:12].max() / np.abs(fd[0:3, 9:12]).max()
    print(f"dT={dT}: exact blocks within {gap[exact].max() / scale:.2e} of the scale; d er / d bg gap {g_bg:.2e} (an approximation: it is recorded)")
    assert g_bg <= R.INERTIAL_DER_DBG_GAP[dT] * 8


def test_prior_jacobian_against_central_differences():
    pre, prev, cur, a = _states(6, 0.05)
    pri = R.unpack_state(a["prior_in"][:21], F64)
    pri["H"] = a["prior_in"][21:].reshape(15, 15)
    prev = _oplus_pose(prev, np.array([0.02, -0.01, 0.015, 0.03, 0.01, -0.02]))
    prev["v"] = prev["v"] + 0.05

    def err(p, _c):
        return np.concatenate([_log(pri["Rwb"].T @ p["Rwb"]), pri["Rwb"].T @ (p["twb"] - pri["twb"]), p["v"] - pri["v"], p["bg"] - pri["bg"],
                               p["ba"] - pri["ba"]])
    e, J = R.prior_edge(pri, prev)
    # the states' rotations are float matrices, orthonormal to 6e-8: LogSO3's trace-based angle and the arctan2 one differ by that much
    assert np.abs(e - err(prev, None)).max() <= 2e-7 * 0.03
    fd = _fd(err, prev, cur)[:, :15]
    assert np.abs(J - fd).max() <= 2e-7


# ---------------------------------------------------------------- planted scenes
@pytest.mark.parametrize("mode", [KF, LF])
@pytest.mark.parametrize("kind,N,dT", [("mono", 400, 0.05), ("stereo", 40, 0.5), ("mixed", 150, 0.05), ("mixed", 150, 0.5)])
def test_planted_scene_is_recovered(mode, kind, N, dT):
    """from 2 degrees / 5 cm off with biases off by 10 % and 20 % gross outliers: the outliers are flagged, the pose comes back"""
    c = R.scene(90 + N, N, mode, kind, dT=dT)
    r = R.solve(c)
    ed = c["args"]["has_mp"] != 0
    assert (r["outlier"][ed][c["planted"][ed]] == 1).all()
    assert (r["outlier"][ed][~c["planted"][ed]] == 0).mean() > 0.85
    d0, d1 = R.state_distance(c["args"]["state"], c["truth"]), R.state_distance(r["state"], c["truth"])
    print(f"mode {mode} {kind} N={N} dT={dT}: rotation {d0[0]:.2e} -> {d1[0]:.2e} rad, position {d0[1]:.2e} -> {d1[1]:.2e} m")
    assert d1[0] * 10 <= d0[0] and d1[1] * 10 <= d0[1]
    # the residual is recorded (pose_inertial_ref.PLANTED_RESIDUAL, profiles/pose_inertial.md): the worst over these scenes per mode
    assert d1[0] <= R.PLANTED_RESIDUAL[mode][0] and d1[1] <= R.PLANTED_RESIDUAL[mode][1]
    assert r["stats"][5] == 4 and r["stats"][6] == 40 and r["stats"][7] == 0 and r["ret"] == r["stats"][1] - r["stats"][2]
    H = r["prior_out"][21:].reshape(15, 15)
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max() and np.linalg.eigvalsh((H + H.T) / 2).min() >= -1e-9 * np.abs(H).max()
    assert np.array_equal(r["prior_out"][:21], r["state"]) and np.array_equal(r["state_f32"], r["state"].astype(F32))


def test_chain_hands_the_prior_on():
    ch = R.chain(10, 120, [LF, LF, KF, LF, LF])
    for k, (c, r) in enumerate(ch):
        d = R.state_distance(r["state"], c["truth"])
        assert d[0] < 2e-3 and d[1] < 2e-2, (k, d)
        if k:
            assert np.array_equal(c["args"]["prev_state"], ch[k - 1][1]["state_f32"])
            if c["args"]["mode"] == LF:
                assert np.array_equal(c["args"]["prior_in"], ch[k - 1][1]["prior_out"])
    # the prior matters: the same frame with an empty prior ends elsewhere
    c, r = ch[3]
    assert not np.array_equal(R.solve(c, prior_in=np.concatenate([c["args"]["prior_in"][:21], np.zeros(225)]))["state"], r["state"])


def test_cov_rw_is_taken_separately():
    """InfoG / InfoA come from cov_rw, not from the preintegration the edge is built from (Optimizer.cc:1213 against :1233, :1246)"""
    c = R.scene(11, 80, LF)
    r = R.solve(c)
    assert not np.array_equal(R.solve(c, cov_rw=c["args"]["cov_rw"] * F32(4.0))["state"], r["state"])


# ---------------------------------------------------------------- against the sequential transcription of the reference's lines
OUTPUTS = ("state", "state_f32", "outlier", "chi2", "prior_out", "trace", "stats", "chi2_rounds")
OURS, THEIRS = Q.Choices(True), Q.Choices(False)


def _cases():
    c = [(f"scene-{mode}-{kind}-{N}-{dT}", (lambda mode=mode, kind=kind, N=N, dT=dT: R.scene(600 + N, N, mode, kind, dT=dT)))
         for mode in (KF, LF) for kind, N, dT in (("mono", 120, 0.05), ("stereo", 40, 0.5), ("mixed", 150, 0.5))]
    return c + [(name, (lambda name=name: R.forced(name))) for name in R.FORCED]


@pytest.mark.parametrize("name,make", _cases(), ids=[n for n, _ in _cases()])
def test_restatement_equals_the_transcription_bit_for_bit(name, make):
    """tests/pose_inertial_seq.py -- one object per vertex and edge, the g2o loop as written -- given the contract's departures: every
    output bit of the restatement, on planted scenes in both modes and on every forced path"""
    c = make()
    a, b = R.solve(c), Q.solve(OURS, c)
    for k in OUTPUTS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (name, k)
    assert a["ret"] == b["ret"]


def test_chain_equals_the_transcription_bit_for_bit():
    prev = None
    for k, mode in enumerate((LF, LF, KF, LF)):
        c = R.scene(820 + k, 100, mode, prev=prev)
        a, b = R.solve(c), Q.solve(OURS, c)
        for key in OUTPUTS:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), (k, key)
        prev = (b["state_f32"], b["prior_out"])


# ---------------------------------------------------------------- the cost of the departures, against the reference's own numeric choices
def _cost(a, b):
    sa, sb, Ha, Hb = a["state"], b["state"], a["prior_out"][21:], b["prior_out"][21:]
    d = {k: float(np.abs(sa[i:j] - sb[i:j]).max()) for k, (i, j) in (("rotation", (0, 9)), ("position", (9, 12)), ("velocity", (12, 15)),
                                                                  ("bg", (15, 18)), ("ba", (18, 21)))}
    d["H"] = float(np.linalg.norm(Ha - Hb) / np.linalg.norm(Hb))
    return d


def _chi2_room(c, a, b):
    """over every round that ran and the recovery pass: (the smallest relative distance of a chi2 to the threshold it was compared with,
    the largest chi2 difference between the two runs relative to that threshold)"""
    x = c["args"]
    ed = x["has_mp"] != 0
    st = ~(x["uright"] < 0)
    close = x["track_depth"] < F32(10.0)
    gap, diff = np.inf, 0.0
    for r in range(5):
        ca, cb = a["chi2_rounds"][r].astype(F64), b["chi2_rounds"][r].astype(F64)
        if np.isnan(cb[ed]).all():
            continue
        if r < 4:
            tm = (R.CHI2_MONO_F if x["mode"] == LF else R.CHI2_MONO_KF)[r]
            thr = np.where(st, R.CHI2_STEREO[r], np.where(close, F32(1.5 * float(tm)), tm)).astype(F64)
        else:
            thr = np.where(st, R.CHI2_STEREO_OUT, R.CHI2_MONO_OUT).astype(F64)
        gap = min(gap, float((np.abs(cb - thr) / thr)[ed].min()))
        diff = max(diff, float((np.abs(ca - cb) / thr)[ed].max()))
    return gap, diff


def test_cost_of_the_departures():
    """the restatement against the sequential transcription run with the reference's own choices (edge after edge, libm, eigh, svd, inv,
    a dense solve, BLAS): measured on planted scenes in both modes and over a chain of four frames where each side hands its own prior on.
    The measured values are recorded in pose_inertial_ref.DEPARTURE_COST and profiles/pose_inertial.md; each must stay within 8 times its
    record (the margin covers the case-to-case spread of last-bit effects, it is not a tolerance on the kernel, which is held to exact
    equality), and no outlier flag may differ.  A case -- a chain frame too -- whose chi2 values, in any round or in the recovery pass, leave
    less room to their thresholds than 100 times the measured chi2 difference is regenerated."""
    worst = {k: 0.0 for k in R.DEPARTURE_COST}
    room = []

    def one(make_a, make_b=None):
        for attempt in range(8):
            ca = make_a(attempt)
            cb = ca if make_b is None else make_b(attempt)
            a, b = R.solve(ca), Q.solve(THEIRS, cb)
            gap, diff = _chi2_room(cb, a, b)
            if gap >= 100 * diff:
                break
        else:
            raise AssertionError("no case leaves the room")
        assert np.array_equal(a["outlier"], b["outlier"]) and a["ret"] == b["ret"]
        room.append(gap / max(diff, 1e-300))
        for k, v in _cost(a, b).items():
            worst[k] = max(worst[k], v)
        return a, b
    for mode in (KF, LF):
        for kind, N, dT in (("mono", 400, 0.05), ("stereo", 40, 0.5), ("mixed", 150, 0.05), ("mixed", 150, 0.5)):
            one(lambda attempt: R.scene(700 + N + 1000 * attempt, N, mode, kind, dT=dT))
    prev_a = prev_b = None                      # the chain: each side hands its own prior on
    for k, mode in enumerate((LF, LF, KF, LF)):
        a, b = one(lambda attempt: R.scene(800 + k + 1000 * attempt, 120, mode, prev=prev_a),
                   lambda attempt: R.scene(800 + k + 1000 * attempt, 120, mode, prev=prev_b))
        prev_a, prev_b = (a["state_f32"], a["prior_out"]), (b["state_f32"], b["prior_out"])
    print("cost of the departures:", {k: f"{v:.2e}" for k, v in worst.items()}, f"; chi2 room / difference at least {min(room):.0f}")
    for k, v in worst.items():
        assert v <= 8 * R.DEPARTURE_COST[k], (k, v)


# ---------------------------------------------------------------- forced paths
@pytest.mark.parametrize("name", R.FORCED)
def test_forced_paths(name):
    R.PATHS = set()
    try:
        c = R.forced(name)
        r = R.solve(c)
        paths = set(R.PATHS)
    finally:
        R.PATHS = None
    st, tr = r["stats"], r["trace"]
    fl = int(st[8])
    if name == "failed_solve":                 # the non-positive pivot: the stale x (zeros) applied, each round ended after one iteration
        assert fl & R.FLAG_SOLVE_FAILED and st[7] == 4 and st[6] == 4 and (tr[:, 0] == 1).all() and (tr[:, 3] == 0).all()
        assert np.array_equal(r["state_f32"], c["args"]["state"]) and "exp_small" in paths
    elif name == "log_outside":
        assert "log_outside" in paths and {"exp_small", "exp_large", "invjr_small", "invjr_large"} <= paths
    elif name == "log_small":
        assert "log_small" in paths
    elif name == "info_clipped":
        assert fl & R.FLAG_INFO_CLIPPED and st[7] == 0
    elif name == "marg_cut":
        assert fl & R.FLAG_MARG_CUT
    elif name == "huber_above":
        assert fl & R.FLAG_PRIOR_HUBER
    elif name == "huber_below":
        assert not fl & R.FLAG_PRIOR_HUBER
    elif name in ("few_edges_kf", "few_edges_f"):                      # 6 + 3 and 5 + 4 edges
        assert fl & R.FLAG_FEW_EDGES and st[5] == 1 and st[6] == 10 and (tr[1:] == 0).all()
    elif name in ("enough_edges_kf", "enough_edges_f"):                # 7 + 3 and 6 + 4
        assert not fl & R.FLAG_FEW_EDGES and st[5] == 4
    elif name == "recovery":
        assert fl & R.FLAG_RECOVERY and st[9] < 30 and st[0] > st[9] and r["outlier"].sum() < st[1] - st[9]
    elif name == "recovery_rec_init":
        assert not fl & R.FLAG_RECOVERY and st[9] < 30 and st[0] == st[9]
    elif name == "nan":
        assert fl & R.FLAG_NONFINITE and np.isnan(r["state"]).any()


def test_info_clipping_and_so3f_branches():
    H, n = R.clip_information(np.diag([1e-13, 1.0, 2.0]), 3)
    assert n == 1 and np.array_equal(np.diag(H), [0.0, 1.0, 2.0])
    R.PATHS = set()
    try:
        R.so3f_exp_matrix(np.array([1e-6, 0, 0], F32)); R.so3f_exp_matrix(np.array([1e-3, 0, 0], F32))
        assert {"so3f_small", "so3f_large"} <= R.PATHS
    finally:
        R.PATHS = None


def test_exports_and_header():
    from rover_slam_amd import capi
    for sym in ("rfe_pose_inertial_optimization", "rfe_pose_inertial_optimization_dev"):
        assert sym in capi.EXPORTS and getattr(capi.lib, sym)
    text = open(os.path.join(ROOT, "include", "rover_fe.h")).read()
    for k, v in (("RFE_PIO_CAM_FLOATS", R.CAM_FLOATS), ("RFE_PIO_STATE_FLOATS", R.STATE_FLOATS), ("RFE_PIO_PREINT_FLOATS", R.PREINT_FLOATS),
                 ("RFE_PIO_COV_RW_FLOATS", R.COV_RW_FLOATS), ("RFE_PIO_PRIOR_DOUBLES", R.PRIOR_DOUBLES)):
        assert f"#define {k} {v}" in text
    assert (capi.PIO_CAM_FLOATS, capi.PIO_STATE_FLOATS, capi.PIO_PREINT_FLOATS, capi.PIO_COV_RW_FLOATS, capi.PIO_PRIOR_DOUBLES) == \
        (R.CAM_FLOATS, R.STATE_FLOATS, R.PREINT_FLOATS, R.COV_RW_FLOATS, R.PRIOR_DOUBLES)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_drop_in_driver_compiles_links_and_runs_without_arguments(tmp_path):
    """include/rfe/pose_inertial_optimization.h with its driver, -std=c++14 -Wall -Werror; the run without arguments touches no device"""
    DD.run(DD.build(tmp_path, "pose_inertial_driver"))
