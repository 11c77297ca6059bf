"""CPU: the contract of DESIGN.md 6k.  tests/optimize_sim3_ref.py (what the kernel is compared with bit for bit) against a sequential,
per-edge transcription of the reference's lines (Optimizer.cc:4195-4494, OptimizableTypes.h:162-235, sim3.h, base_binary_edge.hpp,
optimization_algorithm_levenberg.cpp, robust_kernel_impl.cpp): one object per vertex and per edge with push / pop / oplus, the numeric
linearizeOplus per edge as written, the LM loop and both rounds statement by statement.  With the departures (a)-(d) switched in, the
two agree in every output bit; with g2o's own choices (sequential sums, libm, a dense solve) the cost of the departures is measured."""
import math
import subprocess

import numpy as np
import pytest

import dropin_driver as DD
import optimize_sim3_ref as R

F32, F64 = np.float32, np.float64


# ================================================================ the sequential transcription (Python floats are IEEE doubles)
class Choices:
    """what the contract departs in: the sum over edges, sin / cos, exp and the solve"""

    def __init__(self, ours):
        self.ours = ours

    def exp(self, x):
        return float(R.exp_(x)) if self.ours else math.exp(x)

    def sincos(self, t):
        if self.ours:
            s, c = R.sincos(t)
            return float(s), float(c)
        return math.sin(t), math.cos(t)

    def solve(self, H, b):
        if self.ours:
            ok, x = R.ldlt_solve(H, b)
            return ok, ([float(v) for v in x] if ok else None)
        A = np.array(H, F64)
        try:
            np.linalg.cholesky(A)                  # LinearSolverDense: an LDLT whose isPositive() decides
        except np.linalg.LinAlgError:
            return False, None
        return True, [float(v) for v in np.linalg.solve(A, np.array(b, F64))]

    def total(self, contributions):
        """contributions: a list of (row i, e12's terms, e21's terms) in edge order; the totals of every term"""
        C = len(contributions[0][1]) if contributions else 36
        if not self.ours:                          # g2o: e12_0, e21_0, e12_1, ... one after the other
            tot = [0.0] * C
            for _, t12, t21 in contributions:
                for c in range(C):
                    tot[c] = (tot[c] + t12[c]) + t21[c]
            return tot
        part = [[0.0] * C for _ in range(R.LANES)]
        for i, t12, t21 in contributions:          # ascending i
            p = part[i % R.LANES]
            for c in range(C):
                p[c] = (p[c] + t12[c]) + t21[c]
        s = R.LANES // 2
        while s >= 1:
            for l in range(s):
                for c in range(C):
                    part[l][c] = part[l][c] + part[l + s][c]
            s //= 2
        return part[0]


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]], F64)


def q_rotate(q, X):                                # Eigen's quaternion * vector
    u = [q[1] * X[2] - q[2] * X[1], q[2] * X[0] - q[0] * X[2], q[0] * X[1] - q[1] * X[0]]
    u = [v + v for v in u]
    c = [q[1] * u[2] - q[2] * u[1], q[2] * u[0] - q[0] * u[2], q[0] * u[1] - q[1] * u[0]]
    return [(X[i] + q[3] * u[i]) + c[i] for i in range(3)]


def q_from_matrix(m):                              # Eigen's Quaterniond(Matrix3d)
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t, w]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
    q = [None] * 4
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[k][j] - m[j][k]) * t
    q[j] = (m[j][i] + m[i][j]) * t
    q[k] = (m[k][i] + m[i][k]) * t
    return q


class Sim3:
    """g2o::Sim3 (sim3.h)"""

    def __init__(self, r, t, s):
        self.r, self.t, self.s = list(r), list(t), s

    @staticmethod
    def from_update(update, M):                    # :70-142
        omega, upsilon, sigma = update[0:3], update[3:6], update[6]
        theta = math.sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
        Om = [[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]]
        s = M.exp(sigma)
        Om2 = [[(Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c] for c in range(3)] for r in range(3)]
        I = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
        eps = 0.00001

        def rodrigues():
            sn, cs = M.sincos(theta)
            return [[(I[r][c] + sn / theta * Om[r][c]) + (1 - cs) / (theta * theta) * Om2[r][c] for c in range(3)] for r in range(3)], sn, cs
        if abs(sigma) < eps:
            C = 1.0
            if theta < eps:
                A, B = 1. / 2., 1. / 6.
                Rm = [[(I[r][c] + Om[r][c]) + Om2[r][c] for c in range(3)] for r in range(3)]
            else:
                theta2 = theta * theta
                Rm, sn, cs = rodrigues()
                A = (1 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
        else:
            C = (s - 1) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                Rm = [[(I[r][c] + Om[r][c]) + Om2[r][c] for c in range(3)] for r in range(3)]
            else:
                Rm, sn, cs = rodrigues()
                a, b = s * sn, s * cs
                theta2, sigma2 = theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        W = [[(A * Om[r][c] + B * Om2[r][c]) + C * I[r][c] for c in range(3)] for r in range(3)]
        t = [(W[r][0] * upsilon[0] + W[r][1] * upsilon[1]) + W[r][2] * upsilon[2] for r in range(3)]
        return Sim3(q_from_matrix(Rm), t, s)

    def map(self, xyz):                            # :144-146
        r = q_rotate(self.r, xyz)
        return [self.s * r[i] + self.t[i] for i in range(3)]

    def inverse(self):                             # :233-236
        rc = [-self.r[0], -self.r[1], -self.r[2], self.r[3]]
        c = -1. / self.s
        return Sim3(rc, q_rotate(rc, [c * v for v in self.t]), 1. / self.s)

    def __mul__(self, other):                      # :266-272
        ax, ay, az, aw = self.r
        bx, by, bz, bw = other.r
        r = [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz,
             ((aw * bz + az * bw) + ax * by) - ay * bx, ((aw * bw - ax * bx) - ay * by) - az * bz]
        rt = q_rotate(self.r, other.t)
        return Sim3(r, [self.s * rt[i] + self.t[i] for i in range(3)], self.s * other.s)

    def key(self):
        return tuple(self.r) + tuple(self.t) + (self.s,)


class VertexSim3Expmap:                            # OptimizableTypes.h:162-191 over BaseVertex
    def __init__(self, estimate, fix_scale, M):
        self._estimate, self._fix_scale, self.M, self._stack = estimate, fix_scale, M, []
        self._memo = {}                            # Sim3(update) * estimate and estimate.inverse() are pure: every edge asks for the same 14

    def estimate(self):
        return self._estimate

    def push(self):
        self._stack.append(self._estimate)

    def pop(self):
        self._estimate = self._stack.pop()

    def discardTop(self):
        self._stack.pop()

    def oplus(self, update):                       # oplusImpl: update is the caller's array
        if self._fix_scale:
            update[6] = 0
        k = ("o", self._estimate.key(), tuple(update))
        if k not in self._memo:
            self._memo[k] = Sim3.from_update(update, self.M) * self._estimate
        self._estimate = self._memo[k]

    def inverse(self):
        k = ("i", self._estimate.key())
        if k not in self._memo:
            self._memo[k] = self._estimate.inverse()
        return self._memo[k]


class Edge:
    """EdgeSim3ProjectXYZ (inverse = False) / EdgeInverseSim3ProjectXYZ (True) over BaseBinaryEdge with the point vertex fixed"""

    def __init__(self, inverse, point, vertex, cam, measurement, inv_sigma2, delta):
        self.inverse, self.point, self.v, self.cam = inverse, point, vertex, cam
        self.measurement, self.information, self.delta = measurement, inv_sigma2, delta    # Identity * invSigmaSquare
        self.error, self.J, self.analytic = [0.0, 0.0], [[0.0] * 7, [0.0] * 7], False

    def computeError(self):                        # OptimizableTypes.h:202-209 / :224-231, Pinhole.cpp:47-54
        y = (self.v.inverse() if self.inverse else self.v.estimate()).map(self.point)
        fx, fy, cx, cy = self.cam
        z = F64(y[2])                              # a numpy double: x / 0 is inf or NaN as in C++, where Python's float raises
        self.error = [float(self.measurement[0] - (fx * y[0] / z + cx)), float(self.measurement[1] - (fy * y[1] / z + cy))]

    def chi2(self):
        e, w = self.error, self.information
        return e[0] * (w * e[0]) + e[1] * (w * e[1])

    def linearizeAnalytic(self):
        """what the reference leaves commented out: the Jacobian of the error in the update of exp(update) * S, in closed form.  For
        information only (test_departure_cost); not the contract."""
        S = self.v.estimate()
        fx, fy = self.cam[0], self.cam[1]
        if not self.inverse:                       # Y = S.map(P2); exp(d) moves it by [-[Y]x | I | Y] d
            Y = np.array(S.map(self.point), F64)
            dY = np.hstack([-skew(Y), np.eye(3), Y.reshape(3, 1)])
        else:                                      # Y = S^-1.map(P1) = R^T (P1 - t) / s; (exp(d) S)^-1 = S^-1 exp(-d)
            X = np.array(self.point, F64)
            Y = np.array(self.v.inverse().map(self.point), F64)
            Rt = np.array([q_rotate([-S.r[0], -S.r[1], -S.r[2], S.r[3]], list(e)) for e in np.eye(3)], F64).T
            dY = (Rt / S.s) @ -np.hstack([-skew(X), np.eye(3), X.reshape(3, 1)])
        dproj = np.array([[fx / Y[2], 0.0, -fx * Y[0] / (Y[2] * Y[2])], [0.0, fy / Y[2], -fy * Y[1] / (Y[2] * Y[2])]], F64)
        J = -dproj @ dY
        if self.v._fix_scale:
            J[:, 6] = 0.0
        self.J = [[float(v) for v in J[0]], [float(v) for v in J[1]]]

    def linearizeOplus(self):                      # base_binary_edge.hpp:131-205, vertex 0 fixed
        if self.analytic:
            return self.linearizeAnalytic()
        delta = 1e-9
        scalar = 1.0 / (2 * delta)
        errorBeforeNumeric = list(self.error)
        add_vj = [0.0] * 7
        for d in range(7):
            self.v.push()
            add_vj[d] = delta
            self.v.oplus(add_vj)
            self.computeError()
            errorBak = list(self.error)
            self.v.pop()
            self.v.push()
            add_vj[d] = -delta
            self.v.oplus(add_vj)
            self.computeError()
            errorBak = [errorBak[0] - self.error[0], errorBak[1] - self.error[1]]
            self.v.pop()
            add_vj[d] = 0.0
            self.J[0][d], self.J[1][d] = scalar * errorBak[0], scalar * errorBak[1]
        self.error = errorBeforeNumeric

    def robustify(self, e):                        # RobustKernelHuber, dsqr a float member
        dsqr = float(F32(self.delta * self.delta))
        if e <= dsqr:
            return e, 1.0
        sqrte = math.sqrt(e)
        return 2 * sqrte * self.delta - dsqr, self.delta / sqrte

    def rho0(self):
        return self.chi2() if self.delta is None else self.robustify(self.chi2())[0]

    def constructQuadraticForm(self):              # base_binary_edge.hpp:55-120 -> this edge's 28 + 7 + 1 terms
        B, omega = self.J, self.information
        omega_r = [-(omega * self.error[0]), -(omega * self.error[1])]
        rho = (self.chi2(), 1.0) if self.delta is None else self.robustify(self.chi2())
        omega_r = [omega_r[0] * rho[1], omega_r[1] * rho[1]]
        w = rho[1] * omega
        out = []
        for j in range(7):
            for k in range(j, 7):
                out.append((B[0][j] * w) * B[0][k] + (B[1][j] * w) * B[1][k])
        for j in range(7):
            out.append(B[0][j] * omega_r[0] + B[1][j] * omega_r[1])
        out.append(rho[0])
        return out


class Levenberg:
    """optimization_algorithm_levenberg.cpp:61-194 over one vertex and a list of (row, e12, e21)"""

    def __init__(self, vertex, pairs, M, max_trials, counters):
        self.v, self.pairs, self.M, self.max_trials, self.n = vertex, pairs, M, max_trials, counters
        self.x = counters["x"]

    def computeActiveErrors(self):
        for _, a, b in self.pairs:
            a.computeError()
            b.computeError()

    def activeRobustChi2(self):
        return self.M.total([(i, [a.rho0()], [b.rho0()]) for i, a, b in self.pairs])[0]

    def buildSystem(self):
        con = []
        for i, a, b in self.pairs:
            a.linearizeOplus()
            b.linearizeOplus()
            con.append((i, a.constructQuadraticForm(), b.constructQuadraticForm()))
        tot = self.M.total(con) if con else [0.0] * 36
        self.H = [[0.0] * 7 for _ in range(7)]
        col = 0
        for j in range(7):
            for k in range(j, 7):
                self.H[j][k] = self.H[k][j] = tot[col]
                col += 1
        self.b = tot[28:35]

    def solve(self, iteration):
        n = self.n
        n["iters"] += 1
        self.computeActiveErrors()
        currentChi = self.activeRobustChi2()
        iniChi = currentChi
        self.buildSystem()
        if iteration == 0:
            maxDiagonal = 0.
            for j in range(7):
                maxDiagonal = max(abs(self.H[j][j]), maxDiagonal)
            self.lam, self.ni, self.nBad = 1e-5 * maxDiagonal, 2., 0
        rho, qmax = 0., 0
        while True:
            self.v.push()
            n["trials"] += 1
            ok2, sol = self.M.solve([[self.H[j][k] + self.lam if j == k else self.H[j][k] for k in range(7)] for j in range(7)], self.b)
            if ok2:
                self.x[:] = sol
            else:
                n["flags"] |= R.FLAG_SOLVE_FAILED
            self.v.oplus(self.x)
            if not all(math.isfinite(v) for v in self.v.estimate().key()):
                n["flags"] |= R.FLAG_NONFINITE
            self.computeActiveErrors()
            tempChi = self.activeRobustChi2()
            if not ok2:
                tempChi = float(R.DBL_MAX)
            rho = currentChi - tempChi
            scale = 0.
            for j in range(7):
                scale += self.x[j] * (self.lam * self.x[j] + self.b[j])
            scale += 1e-3
            rho /= scale
            if rho > 0 and math.isfinite(tempChi):
                v = 2 * rho - 1
                alpha = 1. - (v * v) * v
                alpha = min(alpha, 2. / 3.)
                self.lam *= max(1. / 3., alpha)
                self.ni = 2.
                currentChi = tempChi
                self.v.discardTop()
                n["ended_rejected"] = False
            else:
                self.lam *= self.ni
                self.ni *= 2
                self.v.pop()
                n["rejected"] += 1
                n["ended_rejected"] = True
            qmax += 1
            if not (rho < 0 and qmax < self.max_trials):
                break
        n["current"] = currentChi
        if qmax == self.max_trials or rho == 0:
            return False
        if (iniChi - currentChi) * 1e3 < iniChi:
            self.nBad += 1
        else:
            self.nBad = 0
        return self.nBad < 3

    def optimize(self, iterations):
        for i in range(iterations):
            if not self.solve(i):
                break


def transcription(c, ours=True, keep=None, chi2=None, analytic=False):
    """Optimizer::OptimizeSim3 on a case of optimize_sim3_ref.scene(), statement by statement; the outputs of the restatement.
    analytic: closed-form Jacobians in place of g2o's numeric ones (for information)"""
    with np.errstate(all="ignore"):
        return _transcription(c, ours, keep, chi2, analytic)


def _transcription(c, ours, keep, chi2, analytic):
    P, M = c["P"], Choices(ours)
    N = len(c["valid"])
    n, n2 = P["n"], P["n2"]
    R1w, t1w, R2w, t2w = P["rcw1"], P["tcw1"], P["rcw2"], P["tcw2"]
    out_keep = np.ones(N, np.uint8) if keep is None else np.array(keep, np.uint8)
    out_chi2 = np.zeros((N, 2), F64) if chi2 is None else np.array(chi2, F64)
    th2 = float(P["th2"])                          # `e12->chi2() > th2`: the float parameter widened, a double comparison
    vSim3 = VertexSim3Expmap(Sim3([float(v) for v in c["s12_0"][:4]], [float(v) for v in c["s12_0"][4:7]], float(c["s12_0"][7])), P["fix_scale"], M)
    deltaHuber = float(F32(np.sqrt(F64(th2))))
    cam1, cam2 = [float(v) for v in P["cam1"]], [float(v) for v in P["cam2"]]
    flags = 0
    pairs = []
    nCorrespondences = 0
    for i in range(n):
        if not c["valid"][i]:                      # vpMatches1[i], pMP1, pMP2 and their isBad()
            continue
        i2 = int(c["idx2"][i])
        if i2 >= n2:
            flags |= R.FLAG_IDX2
            i2 = -1
        X1, X2 = c["xw1"][i], c["xw2"][i]
        P3D1c = [F32(F32(F32(F32(R1w[r, 0] * X1[0]) + F32(R1w[r, 1] * X1[1])) + F32(R1w[r, 2] * X1[2])) + t1w[r]) for r in range(3)]
        P3D2c = [F32(F32(F32(F32(R2w[r, 0] * X2[0]) + F32(R2w[r, 1] * X2[1])) + F32(R2w[r, 2] * X2[2])) + t2w[r]) for r in range(3)]
        if i2 < 0 and not P["all_points"]:
            continue
        if P3D2c[2] < 0:
            continue
        nCorrespondences += 1
        obs1 = [float(c["kpts1"][i, 0]), float(c["kpts1"][i, 1])]
        o1 = int(c["octave1"][i])
        invSigmaSquare1 = float(P["inv1"][o1 if 0 <= o1 < len(P["inv1"]) else 0])
        e12 = Edge(False, [float(v) for v in P3D2c], vSim3, cam1, obs1, invSigmaSquare1, deltaHuber)
        if i2 >= 0:
            obs2 = [float(c["kpts2"][i2, 0]), float(c["kpts2"][i2, 1])]
            o2 = int(c["octave2"][i2])
        else:
            invz = F32(1) / P3D2c[2]
            obs2 = [float(F32(P3D2c[0] * invz)), float(F32(P3D2c[1] * invz))]
            o2 = 0                                 # cv::KeyPoint(Point2f, size): the octave stays 0
        invSigmaSquare2 = float(P["inv2"][o2 if 0 <= o2 < len(P["inv2"]) else 0])
        e21 = Edge(True, [float(v) for v in P3D1c], vSim3, cam2, obs2, invSigmaSquare2, deltaHuber)
        e12.analytic = e21.analytic = analytic
        pairs.append((i, e12, e21))
    trace, stats = np.zeros((2, 8), F64), np.zeros(8, np.int32)
    counters = {"x": [0.0] * 7, "iters": 0, "trials": 0, "rejected": 0, "flags": flags, "ended_rejected": False, "current": 0.0}
    its = [P["iterations"][0] or 5, P["iterations"][1] or 5, P["iterations"][2] or 10]
    max_trials = P["max_trials"] or 10
    s12_0 = np.asarray(c["s12_0"], F64)

    def result(s12, ret, nBad, rounds):
        f = counters["flags"] | (0 if bool(np.all(np.isfinite(s12))) else R.FLAG_NONFINITE)
        stats[:] = [ret, nCorrespondences, nBad, rounds, counters["iters"], counters["trials"], counters["rejected"], f]
        return {"s12": s12, "s12_f32": s12.astype(F32), "keep": out_keep, "chi2": out_chi2, "trace": trace, "stats": stats, "ret": ret}

    def close_round(rnd, lm, left):
        if counters["ended_rejected"]:
            counters["flags"] |= R.FLAG_ENDED_REJECTED
        trace[rnd, :5] = [counters["iters"] - sum(trace[:rnd, 0]), counters["trials"] - sum(trace[:rnd, 1]), lm.lam, counters["current"], left]

    if nCorrespondences == 0:                      # g2o has nothing to optimise; :4456 returns 0
        counters["flags"] |= R.FLAG_EARLY
        return result(s12_0.copy(), 0, 0, 0)
    lm = Levenberg(vSim3, pairs, M, max_trials, counters)
    lm.optimize(its[0])
    nBad = 0
    alive = []
    for i, e12, e21 in pairs:
        out_chi2[i] = [e12.chi2(), e21.chi2()]
        if e12.chi2() > th2 or e21.chi2() > th2:
            out_keep[i] = 0
            nBad += 1
            continue
        e12.delta = e21.delta = None               # setRobustKernel(0)
        alive.append((i, e12, e21))
    close_round(0, lm, nCorrespondences - nBad)
    nMoreIterations = its[2] if nBad > 0 else its[1]
    if nCorrespondences - nBad < 10:
        counters["flags"] |= R.FLAG_EARLY
        return result(s12_0.copy(), 0, nBad, 1)
    counters["ended_rejected"] = False
    lm = Levenberg(vSim3, alive, M, max_trials, counters)
    lm.optimize(nMoreIterations)
    nIn = 0
    for i, e12, e21 in alive:
        e12.computeError()
        e21.computeError()
        out_chi2[i] = [e12.chi2(), e21.chi2()]
        if e12.chi2() > th2 or e21.chi2() > th2:
            out_keep[i] = 0
        else:
            nIn += 1
    close_round(1, lm, nIn)
    return result(np.array(vSim3.estimate().key(), F64), nIn, nBad, 2)


def same(a, b):
    for k in ("s12", "s12_f32", "keep", "chi2", "trace", "stats"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (k, a[k], b[k])
    assert a["ret"] == b["ret"]


# ================================================================ 1. the restatement against the transcription
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n", [0, 1, 9, 10, 11, 257, 1100])
def test_restatement_equals_the_transcription(n, fix_scale, mixed):
    c = R.scene(100 + n, n, fix_scale=fix_scale, mixed=mixed, pixel=False)
    N = c["P"]["n"]
    keep, chi2 = np.full(N, 7, np.uint8), np.full((N, 2), -3.0)
    r = R.solve(c, keep=keep, chi2=chi2)
    same(r, transcription(c, True, keep, chi2))
    if n >= 257:
        assert r["stats"][3] == 2 and r["ret"] > n // 2 and r["stats"][2] > 0


@pytest.mark.parametrize("name", R.FORCED)
def test_forced_cases_equal_the_transcription(name):
    c = R.forced(name)
    same(R.solve(c), transcription(c, True))


# ================================================================ 2. what the departures cost
DEPARTURE_CASES = [(200 + k, n, fs, mx) for k, (n, fs, mx) in enumerate([(60, False, False), (150, True, False), (300, False, True), (700, True, True)])]


def test_departure_cost():
    worst, margin = 0.0, np.inf
    for seed, n, fs, mx in DEPARTURE_CASES:
        c = R.scene(seed, n, fix_scale=fs, mixed=mx, pixel=False)
        ours, g2o = R.solve(c), transcription(c, False)
        th2 = float(c["P"]["th2"])
        pair = ours["chi2"].any(1)
        # first: no chi2 the classifications compared is near th2, so a different rounding cannot flip a bit of keep
        m = np.min(np.abs(ours["chi2"][pair] - th2) / th2)
        margin = min(margin, m)
        assert m > 1e-6, (seed, m)
        assert np.array_equal(ours["keep"], g2o["keep"]) and ours["ret"] == g2o["ret"] and np.array_equal(ours["stats"][:3], g2o["stats"][:3])
        d = float(np.max(np.abs(ours["s12"] - g2o["s12"])))
        worst = max(worst, d)
        print(f"seed {seed} n {n} fix_scale {fs} mixed {mx}: max |s12 - s12_g2o| = {d:.3e}, chi2 margin {m:.3e}")
        ana = transcription(c, True, analytic=True)                    # for information: what the numeric Jacobian itself costs
        print(f"    analytic Jacobian: max |s12 - s12_analytic| = {float(np.max(np.abs(ours['s12'] - ana['s12']))):.3e}, keep bits that differ "
              f"{int((ours['keep'] != ana['keep']).sum())}, return {ours['ret']} / {ana['ret']}, LM iterations {ours['stats'][4]} / {ana['stats'][4]}, "
              f"trials {ours['stats'][5]} / {ana['stats'][5]}")
    print(f"departures: worst Sim3 difference {worst:.3e} (recorded {R.DEPARTURE_SIM3_MAX:.3e}), smallest relative chi2 margin {margin:.3e}")
    assert worst <= 8 * R.DEPARTURE_SIM3_MAX


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def test_exp_against_libm():
    xs = list(np.linspace(-5.0, 5.0, 20001)) + [0.0, 1e-9, -1e-9, 1e-5, -1e-5, np.nextafter(1e-5, 0), -np.nextafter(1e-5, 0)]
    ln2 = math.log(2.0)
    for k in range(-7, 8):                         # the edges of the argument reduction: (k + 1/2) ln 2
        e = (k + 0.5) * ln2
        xs += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
    worst = max(_ulps(R.exp_(x), math.exp(x)) for x in xs)
    print(f"exp_: max {worst} ulp from libm over [-5, 5]")
    assert worst <= R.EXP_MAX_ULP
    assert R.exp_(0.0) == 1.0 and R.exp_(-0.0) == 1.0 and np.isnan(R.exp_(np.nan))
    assert R.exp_(710.0) == np.inf and R.exp_(np.inf) == np.inf and R.exp_(-746.0) == 0.0 and R.exp_(-np.inf) == 0.0
    assert R.exp_(-745.0) == math.exp(-745.0) and _ulps(R.exp_(709.0), math.exp(709.0)) <= 1


# ================================================================ 3. that it optimises
@pytest.mark.parametrize("fix_scale", [False, True])
def test_it_optimises(fix_scale):
    c = R.scene(300 + fix_scale, 400, fix_scale=fix_scale, rot=0.05, trans=0.1, dscale=0.03, gross=0.2)
    r = R.solve(c)
    n = c["P"]["n"]
    planted, kept = c["planted"][:n], r["keep"][:n] == 1
    assert not (planted & kept).any() and kept[~planted].all() and r["ret"] == int((~planted).sum())
    before, after = R.sim3_distance(c["s12_0"], c["truth"]), R.sim3_distance(r["s12"], c["truth"])
    gains = [b / a for b, a in zip(before, after) if b > 0]
    print(f"fix_scale {fix_scale}: before {before}, after {after}, gains {gains}")
    assert min(gains) >= R.OPTIMISES_GAIN / 16
    if fix_scale:
        assert r["s12"][7] == c["s12_0"][7] == 1.0


# ================================================================ 4. forced paths
def test_round_two_iterations_follow_nbad():
    a, b = R.solve(R.forced("no_bad")), R.solve(R.forced("some_bad"))
    assert a["stats"][2] == 0 and a["trace"][1, 0] <= 5 and b["stats"][2] > 0
    long = R.forced("some_bad")
    long["P"] = dict(long["P"], iterations=(5, 1, 2))
    assert R.solve(long)["trace"][1, 0] == 2       # nBad > 0 takes the third count
    short = R.forced("no_bad")
    short["P"] = dict(short["P"], iterations=(5, 1, 2))
    assert R.solve(short)["trace"][1, 0] == 1


def test_early_exit_around_ten_survivors():
    c9, c10 = R.forced("survivors9"), R.forced("survivors10")
    r9, r10 = R.solve(c9), R.solve(c10)
    assert r9["stats"].tolist()[:4] == [0, 12, 3, 1] and r9["stats"][7] & R.FLAG_EARLY and r9["ret"] == 0
    assert np.array_equal(r9["s12"], c9["s12_0"]) and (r9["keep"][:3] == 0).all() and (r9["keep"][3:] == 1).all()
    assert not np.array_equal(r9["round1"], c9["s12_0"])           # round 1 moved the vertex; it is not written back
    assert r10["stats"].tolist()[1:4] == [12, 2, 2] and r10["ret"] == 10 and not r10["stats"][7] & R.FLAG_EARLY
    assert not np.array_equal(r10["s12"], c10["s12_0"])


def test_stale_chi2_decides_pairs():
    c = R.forced("stale")
    r = R.solve(c)
    assert r["stats"][7] & R.FLAG_ENDED_REJECTED
    P, n = c["P"], c["P"]["n"]
    f, _ = R.pairs(P, c["xw1"], c["xw2"], c["valid"], c["kpts1"], c["octave1"], c["idx2"], c["kpts2"], c["octave2"], n, P["n2"])
    S = [F64(v) for v in r["round1"]]
    a, b = R.pair_errors(P, f, S, R.sim3_inverse(S))
    fresh = (a[0] * (f["isg1"] * a[0]) + a[1] * (f["isg1"] * a[1]) > float(P["th2"])) | (b[0] * (f["isg2"] * b[0]) + b[1] * (f["isg2"] * b[1]) > float(P["th2"]))
    assert int((f["pair"] & fresh).sum()) < r["stats"][2]          # pairs the vertex's own estimate would have kept were removed


def test_max_trials_one():
    r = R.solve(R.forced("max_trials1"))
    assert r["trace"][:, :2].tolist() == [[1, 1], [1, 1]] and r["stats"][4] == 2


def test_normalised_observation_of_rows_outside_kf2():
    px, unit = R.forced("normalised_pixel"), R.forced("normalised_unit")
    rp, ru = R.solve(px), R.solve(unit)
    out_p, out_u = px["idx2"][:px["P"]["n"]] < 0, unit["idx2"][:unit["P"]["n"]] < 0
    # with a pixel-unit camera every such row's e21 is hundreds of pixels off and the row goes; with fx = fy = 1, cx = cy = 0 it survives
    assert out_p.sum() > 20 and (rp["keep"][:len(out_p)][out_p] == 0).all()
    assert (ru["keep"][:len(out_u)][out_u & ~unit["planted"][:len(out_u)]] == 1).mean() > 0.9
    lvl = R.forced("octave_level0")                # KF2's octaves are all 3: rows outside KF2 still weigh with level 0
    f, _ = R.pairs(lvl["P"], lvl["xw1"], lvl["xw2"], lvl["valid"], lvl["kpts1"], lvl["octave1"], lvl["idx2"], lvl["kpts2"], lvl["octave2"],
                   lvl["P"]["n"], lvl["P"]["n2"])
    o = lvl["idx2"][:lvl["P"]["n"]] < 0
    assert (f["isg2"][o] == F64(lvl["P"]["inv2"][0])).all() and (f["isg2"][~o] == F64(lvl["P"]["inv2"][3])).all()


def test_skipped_and_degenerate_rows():
    c = R.forced("behind")
    r = R.solve(c)
    assert r["stats"][1] == c["P"]["n"] - 1 and r["keep"][c["special"]] == 1 and not r["chi2"][c["special"]].any()
    for name in ("z_zero", "nan"):
        c = R.forced(name)
        r = R.solve(c)
        assert r["stats"][1] == c["P"]["n"] and r["stats"][7] & R.FLAG_NONFINITE and np.array_equal(r["s12"], c["s12_0"])
    c = R.forced("not_all_points")
    r = R.solve(c)
    n = c["P"]["n"]
    assert r["stats"][1] == int((c["idx2"][:n] >= 0).sum()) and (r["keep"][:n][c["idx2"][:n] < 0] == 1).all()
    c = R.forced("idx2_range")
    assert R.solve(c)["stats"][7] & R.FLAG_IDX2
    c = R.forced("invalid")
    r = R.solve(c)
    assert r["stats"][1] == int(c["valid"].sum()) and (r["keep"][c["valid"] == 0] == 1).all()


@pytest.mark.parametrize("name,ulps,kept", [("th2_below", -1, 1), ("th2_equal", 0, 1), ("th2_above", 1, 0)])
def test_one_ulp_either_side_of_th2_in_the_final_classification(name, ulps, kept):
    c = R.forced(name)
    row, th2 = c["th2_row"], F64(c["P"]["th2"])
    want = th2 if ulps == 0 else np.nextafter(th2, F64(ulps) * np.inf)
    for r in (R.solve(c), transcription(c, True)):
        # the estimate never moved, both rounds ran, and the row's e12 met the final check with exactly the planted double
        assert np.array_equal(r["s12"], c["s12_0"]) and r["stats"][3] == 2 and r["stats"][2] == 0 and not r["stats"][7] & R.FLAG_EARLY
        assert r["chi2"][row, 0] == want and r["chi2"][row, 1] < 1.0
        assert r["keep"][row] == kept              # `>` against (double) th2: th2 itself and the double below stay, the double above goes
    # a float comparison would not tell the three apart
    assert F32(want) == F32(th2)


def test_fix_scale_leaves_the_scale_bit_unchanged():
    c = R.forced("fix_scale")
    r = R.solve(c)
    assert r["ret"] > 0 and r["s12"][7] == 1.0625 and not np.array_equal(r["s12"][:7], c["s12_0"][:7])


# ================================================================ 5. the exports and the driver
def test_exports():
    from rover_slam_amd import capi
    assert {"rfe_optimize_sim3", "rfe_optimize_sim3_dev"} <= set(capi.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"rfe_optimize_sim3", "rfe_optimize_sim3_dev"} <= syms


def test_driver_builds_links_and_runs_without_a_device(tmp_path):
    exe = DD.build(tmp_path, "optimize_sim3_driver")
    assert "no device touched" in DD.run(exe).stdout
