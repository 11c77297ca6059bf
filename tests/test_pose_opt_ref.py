"""CPU: the restatement tests/pose_opt_ref.py against a scalar transcription of the reference's PoseOptimization: one
Python object per g2o edge, the Levenberg-Marquardt step of optimization_algorithm_levenberg.cpp:61-169 and the rounds of
src/Optimizer.cc:270-400 statement by statement.  With the contract's sums, sincos and LDLT every output is equal; with g2o's own choices
(sequential sums, libm's sin / cos, a general solve) the three departures are measured and held to the bounds of profiles/pose_opt.md."""
import math

import numpy as np
import pytest

import pose_opt_ref as R

F32, F64 = np.float32, np.float64
KINDS = ("mono", "stereo", "mixed")


def f32(x):
    return float(F32(x))


# ---------------------------------------------------------------- the transcription
class SE3Quat:
    """Thirdparty/g2o/g2o/types/se3quat.h on Python floats; r = [x, y, z, w]"""

    def __init__(self, r, t):
        self.r, self.t = list(r), list(t)
        self.normalizeRotation()

    def normalizeRotation(self):
        if self.r[3] < 0:
            self.r = [-c for c in self.r]
        x, y, z, w = self.r
        n = math.sqrt(x * x + y * y + z * z + w * w)
        self.r = [x / n, y / n, z / n, w / n]

    @staticmethod
    def rot(r, v):                                  # Eigen: QuaternionBase::_transformVector
        qv = r[:3]
        cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]   # noqa: E731
        uv = cr(qv, v)
        uv = [c + c for c in uv]
        c2 = cr(qv, uv)
        return [v[i] + r[3] * uv[i] + c2[i] for i in range(3)]

    def map(self, xyz):
        p = SE3Quat.rot(self.r, xyz)
        return [p[i] + self.t[i] for i in range(3)]

    def __mul__(self, tr2):
        p = SE3Quat.rot(self.r, tr2.t)
        t = [self.t[i] + p[i] for i in range(3)]
        a, b = self.r, tr2.r
        r = [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
             a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
             a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
             a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]
        return SE3Quat(r, t)

    @staticmethod
    def exp(update, sincos):
        omega, upsilon = update[:3], update[3:]
        theta = math.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
        Omega = [[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]]
        mm = lambda A, B: [[A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]   # noqa: E731
        Eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        Omega2 = mm(Omega, Omega)
        if theta < 0.00001:
            Rm = [[Eye[r][c] + Omega[r][c] + Omega2[r][c] for c in range(3)] for r in range(3)]
            V = Rm
        else:
            s, co = sincos(theta)
            s, co = float(s), float(co)
            Rm = [[Eye[r][c] + s / theta * Omega[r][c] + (1 - co) / (theta * theta) * Omega2[r][c] for c in range(3)] for r in range(3)]
            V = [[Eye[r][c] + (1 - co) / (theta * theta) * Omega[r][c] + (theta - s) / (theta * theta * theta) * Omega2[r][c] for c in range(3)]
                 for r in range(3)]
        t = [V[r][0] * upsilon[0] + V[r][1] * upsilon[1] + V[r][2] * upsilon[2] for r in range(3)]
        return SE3Quat(SE3Quat.from_matrix(Rm), t)

    @staticmethod
    def from_matrix(m):                             # Eigen: quaternionbase_assign_impl<Other, 3, 3>
        t = m[0][0] + m[1][1] + m[2][2]
        q = [0.0] * 4
        if t > 0:
            t = math.sqrt(t + 1.0)
            q[3] = 0.5 * t
            t = 0.5 / t
            q[0], q[1], q[2] = (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t
        else:
            i = 0
            if m[1][1] > m[0][0]:
                i = 1
            if m[2][2] > m[i][i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
            q[i] = 0.5 * t
            t = 0.5 / t
            q[3] = (m[k][j] - m[j][k]) * t
            q[j] = (m[j][i] + m[i][j]) * t
            q[k] = (m[k][i] + m[i][k]) * t
        return q


class Edge:
    """EdgeSE3ProjectXYZOnlyPose (stereo False) / EdgeStereoSE3ProjectXYZOnlyPose (True) with a RobustKernelHuber"""

    def __init__(self, idx, stereo, obs, Xw, inv_sigma2, cam):
        self.idx, self.stereo, self.obs, self.Xw, self.info = idx, stereo, obs, Xw, inv_sigma2
        self.fx, self.fy, self.cx, self.cy, self.bf = cam
        self.delta = f32(math.sqrt(7.815)) if stereo else f32(math.sqrt(5.991))
        self.dsqr = f32(self.delta * self.delta)    # float dsqr (robust_kernel_impl.h:84)
        self.level, self.robust = 0, True
        self.error = [0.0] * (3 if stereo else 2)

    def computeError(self, est):
        x, y, z = est.map(self.Xw)
        if self.stereo:                             # types_six_dof_expmap.cpp:339-346
            invz = f32(1.0 / z)
            u = x * invz * self.fx + self.cx
            v = y * invz * self.fy + self.cy
            proj = [u, v, u - self.bf * invz]
        else:                                       # Pinhole.cpp:47-54
            proj = [self.fx * x / z + self.cx, self.fy * y / z + self.cy]
        self.error = [o - p for o, p in zip(self.obs, proj)]

    def chi2(self):
        c = 0.0
        for k, e in enumerate(self.error):
            c = e * (self.info * e) if k == 0 else c + e * (self.info * e)
        return c

    def robustify(self, e):                         # robust_kernel_impl.cpp:78-91
        if e <= self.dsqr:
            return e, 1.0
        sqrte = math.sqrt(e)
        return 2 * sqrte * self.delta - self.dsqr, self.delta / sqrte

    def linearizeOplus(self, est):
        x, y, z = est.map(self.Xw)
        if self.stereo:                             # types_six_dof_expmap.cpp:375-404
            fx, fy, bf = self.fx, self.fy, self.bf
            invz = 1.0 / z
            invz_2 = invz * invz
            J = [[x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, 0.0, x * invz_2 * fx],
                 [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, 0.0, -invz * fy, y * invz_2 * fy]]
            J.append([J[0][0] - bf * y * invz_2, J[0][1] + bf * x * invz_2, J[0][2], J[0][3], 0.0, J[0][5] - bf * invz_2])
        else:                                       # OptimizableTypes.cpp:58-73, Pinhole.cpp:119-130
            SE3deriv = [[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]]
            Jac = [[self.fx / z, 0.0, -self.fx * x / (z * z)], [0.0, self.fy / z, -self.fy * y / (z * z)]]
            J = [[sum_lr([-Jac[r][k] * SE3deriv[k][c] for k in range(3)]) for c in range(6)] for r in range(2)]
        self.J = J

    def constructQuadraticForm(self):
        """the edge's addends to A (upper triangle, row by row) and to -b (base_unary_edge.hpp:56-66)"""
        A, D = self.J, len(self.J)
        rho1 = self.robustify(self.chi2())[1] if self.robust else 1.0
        w = rho1 * self.info
        Hc = [sum_lr([(A[r][j] * w) * A[r][k] for r in range(D)]) for j in range(6) for k in range(j, 6)]
        if self.robust:
            bc = [sum_lr([((rho1 * A[r][j]) * self.info) * self.error[r] for r in range(D)]) for j in range(6)]
        else:
            bc = [sum_lr([(A[r][j] * self.info) * self.error[r] for r in range(D)]) for j in range(6)]
        return Hc + bc


def sum_lr(v):
    s = v[0]
    for a in v[1:]:
        s = s + a
    return s


def contract_sum(n):
    def summer(items, width):
        vals, act = np.zeros((n, width), F64), np.zeros(n, bool)
        for i, v in items:
            vals[i], act[i] = v, True
        return [float(v) for v in R.tree_sum(vals, act)]
    return summer


def sequential_sum(items, width):
    tot = [0.0] * width
    for _, v in items:
        tot = [a + b for a, b in zip(tot, v)]
    return tot


def contract_solve(M, b):
    ok, x = R.ldlt_solve(M, b)
    return ok, None if x is None else [float(v) for v in x]


def general_solve(M, b):
    M = np.array(M, F64)
    try:
        np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return False, None
    return True, [float(v) for v in np.linalg.solve(M, np.array(b, F64))]


def libm_sincos(theta):
    return math.sin(theta), math.cos(theta)


def transcription(c, summer=None, sincos=R.sincos, solve=contract_solve):
    """Optimizer::PoseOptimization on the case c (pose_opt_ref.scene).  Returns the outputs of pose_opt_ref.pose_optimization and the final
    chi2 of every edge in float64."""
    P = c["P"]
    N = len(c["kpts"])
    summer = summer or contract_sum(N)
    cam = tuple(float(P[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    outlier, chi2_out = np.zeros(N, np.uint8), np.zeros(N, F32)
    chi2_d = np.full(N, np.nan)
    trace, stats = np.zeros((4, 8), F64), np.zeros(8, np.int32)
    pose0 = [float(v) for v in c["pose0"]]
    vSE3 = SE3Quat(pose0[:4], pose0[4:])
    edges = []
    nInitialCorrespondences = 0
    for i in range(N):
        if c["has_mp"][i]:
            nInitialCorrespondences += 1
            outlier[i] = 0
            octave = int(c["octave"][i])
            invSigma2 = float(P["inv_level_sigma2"][octave if 0 <= octave < P["nlevels"] else 0])
            ur = float(c["uright"][i])
            obs = [float(c["kpts"][i, 0]), float(c["kpts"][i, 1])]
            if not ur < 0:
                obs.append(ur)
            edges.append(Edge(i, not ur < 0, obs, [float(v) for v in c["xw"][i]], invSigma2, cam))
    stats[1] = nInitialCorrespondences
    res = {"outlier": outlier, "chi2": chi2_out, "trace": trace, "stats": stats, "chi2_f64": chi2_d}
    if nInitialCorrespondences < 3:
        res.update(pose=np.array(pose0, F64), pose_f32=c["pose0"].copy(), ret=0)
        return res
    its = [v if v > 0 else 10 for v in P["iterations"]]
    maxTrials = P["max_trials"] if P["max_trials"] > 0 else 10
    x = [0.0] * 6
    flags = nBad = 0
    for it in range(4):
        vSE3 = SE3Quat(pose0[:4], pose0[4:])
        active = [e for e in edges if e.level == 0]                 # initializeOptimization(0)

        def computeActiveErrors():
            for e in active:
                e.computeError(vSE3)

        def activeRobustChi2():
            return summer([(e.idx, [e.robustify(e.chi2())[0] if e.robust else e.chi2()]) for e in active], 1)[0]

        # SparseOptimizer::optimize -> OptimizationAlgorithmLevenberg::solve
        iters = trials = 0
        lam, ni, lm_nBad = 0.0, 2.0, 0
        rejected_last = False
        currentChi = 0.0
        for iteration in range(its[it]):
            iters += 1
            computeActiveErrors()
            currentChi = activeRobustChi2()
            tempChi = currentChi
            iniChi = currentChi
            quad = []
            for e in active:                                        # buildSystem
                e.linearizeOplus(vSE3)
                quad.append((e.idx, e.constructQuadraticForm()))
            S = summer(quad, 27)
            H = [[0.0] * 6 for _ in range(6)]
            col = 0
            for j in range(6):
                for k in range(j, 6):
                    H[j][k] = H[k][j] = S[col]
                    col += 1
            b = [-v for v in S[21:]]
            if iteration == 0:
                maxDiagonal = 0.0
                for j in range(6):
                    a = abs(H[j][j])
                    maxDiagonal = maxDiagonal if a < maxDiagonal else a      # std::max(fabs(..), maxDiagonal)
                lam, ni, lm_nBad = 1e-5 * maxDiagonal, 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                trials += 1
                backup = vSE3                                       # push
                M = [[H[j][k] + (lam if j == k else 0.0) for k in range(6)] for j in range(6)]
                ok2, sol = solve(M, b)
                if ok2:
                    x = sol
                else:
                    flags |= R.FLAG_SOLVE_FAILED
                vSE3 = SE3Quat.exp(x, sincos) * vSE3                # oplusImpl
                if not all(math.isfinite(v) for v in vSE3.r + vSE3.t):
                    flags |= R.FLAG_NONFINITE
                computeActiveErrors()
                tempChi = activeRobustChi2()
                if not ok2:
                    tempChi = float(R.DBL_MAX)
                rho = currentChi - tempChi
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                rho /= scale
                if rho > 0 and math.isfinite(tempChi):
                    v = 2 * rho - 1
                    alpha = 1. - v * v * v
                    alpha = min(alpha, 2. / 3.)
                    scaleFactor = max(1. / 3., alpha)
                    lam *= scaleFactor
                    ni = 2.0
                    currentChi = tempChi
                    rejected_last = False                           # discardTop
                else:
                    lam *= ni
                    ni *= 2
                    vSE3 = backup                                   # pop
                    stats[6] += 1
                    rejected_last = True
                qmax += 1
                if not (rho < 0 and qmax < maxTrials):
                    break
            if qmax == maxTrials or rho == 0:
                break
            if (iniChi - currentChi) * 1e3 < iniChi:
                lm_nBad += 1
            else:
                lm_nBad = 0
            if lm_nBad >= 3:
                break
        if rejected_last:
            flags |= R.FLAG_ENDED_REJECTED
        nBad = 0
        for e in edges:                                             # Optimizer.cc:294-384
            if outlier[e.idx]:
                e.computeError(vSE3)
            with np.errstate(over="ignore"):                         # `const float chi2 = e->chi2()`: past FLT_MAX it is inf
                chi2 = F32(e.chi2())
            chi2_d[e.idx], chi2_out[e.idx] = e.chi2(), chi2
            if chi2 > (F32(7.815) if e.stereo else F32(5.991)):
                outlier[e.idx] = 1
                e.level = 1
                nBad += 1
            else:
                outlier[e.idx] = 0
                e.level = 0
            if it == 2:
                e.robust = False
        stats[3] += 1
        stats[4] += iters
        stats[5] += trials
        trace[it, :5] = [iters, trials, lam, currentChi, nInitialCorrespondences - nBad]
        if len(edges) < 10:
            break
    pose = np.array(vSE3.r + vSE3.t, F64)
    stats[0], stats[2], stats[7] = nInitialCorrespondences - nBad, nBad, flags
    res.update(pose=pose, pose_f32=pose.astype(F32), ret=int(stats[0]))
    return res


def same(got, ref, what=("pose", "pose_f32", "outlier", "chi2", "trace", "stats")):
    for k in what:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k]), equal_nan=True), (k, got[k], ref[k])
    assert np.asarray(got["pose"]).tobytes() == np.asarray(ref["pose"]).tobytes() or not np.all(np.isfinite(ref["pose"]))


# ---------------------------------------------------------------- 1: the restatement is the transcription
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [3, 9, 10, 257, 1100])
def test_restatement_equals_transcription(N, kind):
    c = R.scene(100 + N, N, kind, has=1.0 if N < 20 else 0.9)
    ref = R.solve(c)
    assert ref["stats"][1] == int(c["has_mp"].sum()) and (N < 3 or ref["stats"][3] >= 1)
    same(transcription(c), ref)


# ---------------------------------------------------------------- 2: what the three departures cost
# measured over these cases (profiles/pose_opt.md): at most 3.5e-16 rad and 9.3e-15 in translation, both at N = 3, where the system is the
# worst conditioned -- not at the largest N; no flag differs and no edge lies near a threshold.  The bounds are 16 times those
DEPARTURE_ROT, DEPARTURE_TRANS = 16 * 3.5e-16, 16 * 9.3e-15


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [3, 9, 10, 257, 1100])
def test_departures_from_g2o_choices(N, kind):
    c = R.scene(100 + N, N, kind, has=1.0 if N < 20 else 0.9)
    ref = R.solve(c)
    g2o = transcription(c, summer=sequential_sum, sincos=libm_sincos, solve=general_solve)
    drot, dtrans = R.pose_distance(ref["pose"], g2o["pose"])
    edge = c["has_mp"] != 0
    thr = np.where(c["uright"] < 0, 5.991, 7.815)
    near = edge & (np.abs(g2o["chi2_f64"] - thr) <= 1e-6 * thr)
    differ = int((ref["outlier"] != g2o["outlier"])[edge & ~near].sum())
    print(f"departures N={N} {kind}: rotation {drot:.3e} rad, translation {dtrans:.3e}, flags differing {differ}, near a threshold {int(near.sum())}")
    assert near.sum() <= 0.01 * edge.sum()
    assert differ == 0
    assert drot <= DEPARTURE_ROT and dtrans <= DEPARTURE_TRANS


# ---------------------------------------------------------------- 3: sincos
SINCOS_ULP = 8.0                                    # measured 2.0 ulp, at theta = 547.42 (profiles/pose_opt.md); four times that


def test_sincos():
    # k = floor(theta 2/pi + 0.5) steps at the odd multiples of pi/4: every multiple of pi/4 up to 1e3 (the 1273rd), either side of it
    k = np.arange(1, 1275, dtype=F64)
    edges = (k[:, None] * (math.pi / 4) * (1 + np.array([-1e-9, -1e-15, 0, 1e-15, 1e-9]))).ravel()
    edges = edges[edges <= 1e3]
    assert edges.max() > 1273 * (math.pi / 4) and len(edges) >= 5 * 1273
    worst, at = 0.0, 0.0
    for th in np.concatenate([np.logspace(-5, 3, 4001), edges, [1e-5, 1e3]]):
        s, co = R.sincos(th)
        for got, want in ((float(s), math.sin(th)), (float(co), math.cos(th))):
            err = abs(got - want) / float(np.spacing(abs(want)))
            if err > worst:
                worst, at = err, float(th)
    print(f"sincos: largest error {worst} ulp at theta = {at!r}")
    assert worst <= SINCOS_ULP
    for th in (1e300, 1e-320, 0.0, 1.7976931348623157e308):
        s, co = R.sincos(th)
        assert np.isfinite(s) and np.isfinite(co) and -1 <= s <= 1 and -1 <= co <= 1


@pytest.mark.parametrize("name,reached", [("quadrants", {0, 1, 2, 3}), ("huge_step", {-1})])
def test_steps_of_many_radians(name, reached):
    """the forced cases that take sincos through every quadrant and through its r = 0 fallback inside the optimisation"""
    c = R.forced(name)
    R.SINCOS_LOG = []
    try:
        r = R.solve(c)
        seen = set(R.SINCOS_LOG)
    finally:
        R.SINCOS_LOG = None
    print(f"{name}: sincos quadrants reached {sorted(seen)} (-1: the fallback), stats {r['stats'].tolist()}")
    assert reached <= seen
    same(transcription(c), r)


def test_ldlt_solves():
    rng = np.random.default_rng(5)
    for _ in range(20):
        A = rng.standard_normal((6, 9))
        M = A @ A.T + np.diag(rng.uniform(0, 1e-3, 6))
        b = rng.standard_normal(6)
        ok, x = R.ldlt_solve(M.tolist(), b.tolist())
        assert ok and np.allclose(np.array(x, F64), np.linalg.solve(M, b), rtol=1e-9, atol=1e-12)
    assert R.ldlt_solve((-np.eye(6)).tolist(), [1.0] * 6)[0] is False


# ---------------------------------------------------------------- 4: it optimises
# measured (profiles/pose_opt.md): the start is at least 227 times further from the truth than the result in rotation and 31 times in
# translation over these cases; the bounds are a sixteenth of that
GAIN_ROT, GAIN_TRANS = 14.0, 1.9


@pytest.mark.parametrize("kind", KINDS)
def test_it_optimises(kind):
    c = R.scene(7, 400, kind)
    r = R.solve(c)
    r0, t0 = R.pose_distance(c["pose0"], c["truth"])
    r1, t1 = R.pose_distance(r["pose"], c["truth"])
    print(f"optimises {kind}: rotation {r0:.4f} -> {r1:.5f} rad, translation {t0:.4f} -> {t1:.5f}")
    assert abs(r0 - 0.05) < 1e-4 and abs(t0 - 0.1) < 1e-4
    assert r1 * GAIN_ROT <= r0 and t1 * GAIN_TRANS <= t0
    edge = c["has_mp"] != 0
    assert (edge & c["planted"]).sum() > 40 and r["outlier"][edge & c["planted"]].all()
    assert r["ret"] == r["stats"][0] == edge.sum() - r["outlier"][edge].sum()


# ---------------------------------------------------------------- 5: paths that need forcing
def solve_rounds(c, rounds):
    """the call cut after its first `rounds` rounds"""
    saved = R.ROUNDS
    try:
        R.ROUNDS = rounds
        return R.solve(c)
    finally:
        R.ROUNDS = saved


def test_round_ends_on_a_rejected_trial():
    c = R.forced("rejected")
    r = R.solve(c)
    assert r["stats"][7] & R.FLAG_ENDED_REJECTED and r["stats"][6] > 0
    same(transcription(c), r)


def test_classification_uses_the_errors_of_the_rejected_estimate():
    """a round that ends on a rejected trial with its inliers active: cut after that round, the chi2 its classification compared is the
    chi2 at the rejected estimate, not at the restored one the call returns"""
    c = R.forced("stale")
    same(transcription(c), R.solve(c))
    k = next(k for k in range(1, 5) if solve_rounds(c, k)["stats"][7] & R.FLAG_ENDED_REJECTED)
    rk = solve_rounds(c, k)
    with np.errstate(all="ignore"):
        f = R.features(c["P"], c["kpts"], c["octave"], c["uright"], c["xw"], c["has_mp"], len(c["kpts"]))
        fresh = R.edge_terms(c["P"], [F64(v) for v in rk["pose"][:4]], [F64(v) for v in rk["pose"][4:]], f, False)[0].astype(F32)
    edge = c["has_mp"] != 0
    print(f"round {k - 1} ends on a rejected trial: {int((fresh != rk['chi2'])[edge].sum())} of {int(edge.sum())} edges carry a stale chi2")
    assert rk["stats"][0] > 150 and (fresh != rk["chi2"])[edge].mean() > 0.5


def test_one_iteration_per_round():
    c = R.forced("one_iteration")
    r = R.solve(c)
    assert r["stats"][3] == 4 and r["stats"][4] == 4 and (r["trace"][:, 0] == 1).all()
    same(transcription(c), r)


def test_exact_data_terminates_on_rho_zero():
    c = R.forced("exact")
    r = R.solve(c)
    assert (r["trace"][:, 0] == 1).all() and r["stats"][2] == 0
    same(transcription(c), r)


def test_below_three_edges():
    c = R.forced("two")
    r = R.solve(c, outlier=np.full(2, 7, np.uint8), chi2=np.full(2, 3, F32))
    assert r["ret"] == 0 and r["stats"].tolist() == [0, 2, 0, 0, 0, 0, 0, 0] and (r["outlier"] == 0).all() and (r["chi2"] == 3).all()
    assert np.array_equal(r["pose_f32"], c["pose0"]) and np.array_equal(r["pose"], c["pose0"].astype(F64)) and not r["trace"].any()


def test_nine_edges_run_one_round():
    c = R.forced("nine")
    r = R.solve(c)
    assert r["stats"][1] == 9 and r["stats"][3] == 1 and not r["trace"][1:].any()
    same(transcription(c), r)


def test_outlier_comes_back():
    c = R.forced("comes_back")
    first, second = solve_rounds(c, 1)["outlier"], solve_rounds(c, 2)["outlier"]
    back = (first == 1) & (second == 0) & (c["has_mp"] != 0)
    print("outliers after round 0 that are inliers after round 1:", int(back.sum()))
    assert back.any()
    same(transcription(c), R.solve(c))


def test_point_behind_the_camera():
    c = R.forced("behind")
    r = R.solve(c)
    assert r["outlier"][c["special"]] == 1 and np.all(np.isfinite(r["pose"]))
    same(transcription(c), r)


def test_nan_world_position():
    c = R.forced("nan")
    r = R.solve(c)
    assert r["stats"][7] & R.FLAG_NONFINITE
    assert np.array_equal(r["pose"][4:], c["pose0"][4:].astype(F64))          # every trial is rejected: the translation is the input's
    same(transcription(c), r)


# ---------------------------------------------------------------- 6: exports
def test_exports():
    from rover_slam_amd import capi
    assert {"rfe_pose_optimization", "rfe_pose_optimization_dev"} <= set(capi.EXPORTS)
    assert C_SIZEOF_POSE_PARAMS == __import__("ctypes").sizeof(capi.PoseParams)


C_SIZEOF_POSE_PARAMS = 4 * (5 + 1 + 16 + 4 + 1)     # rfe_pose_params: five floats, nlevels, the table, iterations[4], max_trials
