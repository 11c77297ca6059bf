"""Sequential transcription of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:4509-4840) over g2o: one object per vertex
and per edge, the reference's statements in the reference's order (sim3.h, types_seven_dof_expmap.h, base_binary_edge.hpp,
block_solver.hpp, optimization_algorithm_levenberg.cpp), scalar float64.  With Choices() it makes the contract's choices
and must equal tests/essential_graph_ref.py exactly; with Choices.g2o() it makes g2o's own -- sequential sums, numpy.linalg.solve for the
system and for W, libm's log / acos / sin / cos / exp -- which is what test_departure_cost measures the departures against."""
import math

import numpy as np

import essential_graph_ref as R
import optimize_sim3_ref as OS
import pose_opt_ref as R6

F32, F64 = np.float32, np.float64


class Choices:
    def __init__(self, tree_sums=True, ldlt=True, own_math=True, own_lu=True):
        self.tree_sums, self.ldlt, self.own_math, self.own_lu = tree_sums, ldlt, own_math, own_lu

    @staticmethod
    def g2o():
        return Choices(False, False, False, False)

    def log(self, x):
        return F64(R.log_(np.array([x], F64))[0]) if self.own_math else F64(math.log(x)) if x > 0 else F64(np.log(F64(x)))

    def acos(self, x):
        return F64(R.acos_(np.array([x], F64))[0]) if self.own_math else F64(math.acos(x))

    def sincos(self, x):
        return R6.sincos(x) if self.own_math else (F64(math.sin(x)), F64(math.cos(x)))

    def exp(self, x):
        return OS.exp_(x) if self.own_math else F64(math.exp(x))

    def total(self, values):
        if self.tree_sums:
            return R.tree_sum(values)
        s = F64(0.0)
        for v in values:
            s = s + v
        return s


def skew(o):
    z = F64(0.0)
    return [[z, -o[2], o[1]], [o[2], z, -o[0]], [-o[1], o[0], z]]


def matmul3(A, B):
    return [[(A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


EYE = [[F64(1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]


class Sim3:
    def __init__(self, r, t, s):
        self.r, self.t, self.s = [F64(v) for v in r], [F64(v) for v in t], F64(s)

    @staticmethod
    def from_row(a):
        return Sim3(a[:4], a[4:7], a[7])

    def row(self):
        return self.r + self.t + [self.s]

    @staticmethod
    def exp(update, ch):
        """sim3.h:70-142"""
        omega, upsilon, sigma = [F64(v) for v in update[:3]], [F64(v) for v in update[3:6]], F64(update[6])
        theta = np.sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
        Omega = skew(omega)
        Omega2 = matmul3(Omega, Omega)
        eps = F64(0.00001)
        s = ch.exp(sigma)
        if theta < eps:
            Rm = [[(EYE[r][c] + Omega[r][c]) + Omega2[r][c] for c in range(3)] for r in range(3)]
        else:
            sn, cs = ch.sincos(theta)
            a, b = sn / theta, (1.0 - cs) / (theta * theta)
            Rm = [[(EYE[r][c] + a * Omega[r][c]) + b * Omega2[r][c] for c in range(3)] for r in range(3)]
        if np.abs(sigma) < eps:
            C = F64(1.0)
            if theta < eps:
                A, B = F64(1.0) / 2.0, F64(1.0) / 6.0
            else:
                theta2 = theta * theta
                A = (1.0 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
        else:
            C = (s - 1.0) / sigma
            if theta < eps:
                sigma2 = sigma * sigma
                A = ((sigma - 1.0) * s + 1.0) / sigma2
                B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma)
            else:
                a, b, theta2, sigma2 = s * sn, s * cs, theta * theta, sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1.0 - b) * theta) / (theta * c)
                B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2
        W = [[(A * Omega[r][c] + B * Omega2[r][c]) + C * EYE[r][c] for c in range(3)] for r in range(3)]
        t = [(W[r][0] * upsilon[0] + W[r][1] * upsilon[1]) + W[r][2] * upsilon[2] for r in range(3)]
        return Sim3(R6.mat_to_quat(Rm), t, s)

    def __mul__(self, o):
        """sim3.h:266-272"""
        rt = R6.rotate(self.r, o.t)
        return Sim3(R6.quat_mul(self.r, o.r), [self.s * rt[i] + self.t[i] for i in range(3)], self.s * o.s)

    def inverse(self):
        qi = [-self.r[0], -self.r[1], -self.r[2], self.r[3]]
        c = F64(-1.0) / self.s
        return Sim3(qi, R6.rotate(qi, [c * self.t[0], c * self.t[1], c * self.t[2]]), F64(1.0) / self.s)

    def map(self, X):
        rx = R6.rotate(self.r, X)
        return [self.s * rx[i] + self.t[i] for i in range(3)]

    def log(self, ch):
        """sim3.h:148-230"""
        sigma = ch.log(self.s)
        Rm = [[F64(v) for v in row] for row in R.quat_to_rot(self.r)]
        d = 0.5 * (((Rm[0][0] + Rm[1][1]) + Rm[2][2]) - 1)
        dR = [Rm[2][1] - Rm[1][2], Rm[0][2] - Rm[2][0], Rm[1][0] - Rm[0][1]]
        eps = F64(0.00001)
        s = self.s
        if np.abs(sigma) < eps:
            C = F64(1.0)
            if d > 1 - eps:
                omega = [0.5 * v for v in dR]
                A, B = F64(1.0) / 2.0, F64(1.0) / 6.0
            else:
                theta = ch.acos(d)
                theta2 = theta * theta
                k = theta / (2 * np.sqrt(1 - d * d))
                omega = [k * v for v in dR]
                sn, cs = ch.sincos(theta)
                A = (1 - cs) / theta2
                B = (theta - sn) / (theta2 * theta)
        else:
            C = (s - 1) / sigma
            if d > 1 - eps:
                sigma2 = sigma * sigma
                omega = [0.5 * v for v in dR]
                A = ((sigma - 1) * s + 1) / sigma2
                B = (((0.5 * sigma2 - sigma) + 1) * s) / (sigma2 * sigma)
            else:
                theta = ch.acos(d)
                k = theta / (2 * np.sqrt(1 - d * d))
                omega = [k * v for v in dR]
                theta2 = theta * theta
                sn, cs = ch.sincos(theta)
                a, b = s * sn, s * cs
                c = theta2 + sigma * sigma
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = ((C - ((b - 1) * sigma + a * theta) / c) * 1.) / theta2
        Omega = skew(omega)
        Omega2 = matmul3(Omega, Omega)
        W = [[(A * Omega[r][c_] + B * Omega2[r][c_]) + C * EYE[r][c_] for c_ in range(3)] for r in range(3)]
        if ch.own_lu:
            upsilon = lu_solve(W, list(self.t))
        else:
            upsilon = [F64(v) for v in np.linalg.solve(np.array(W, F64), np.array(self.t, F64))]
        return omega + upsilon + [sigma]


def lu_solve(W, t):
    """departure (f) on scalars, with real row exchanges"""
    W = [list(r) for r in W]
    p = 0
    for r in (1, 2):
        if np.abs(W[r][0]) > np.abs(W[p][0]):
            p = r
    W[0], W[p] = W[p], W[0]
    t[0], t[p] = t[p], t[0]
    for r in (1, 2):
        l = W[r][0] / W[0][0]
        W[r][1] = W[r][1] - l * W[0][1]
        W[r][2] = W[r][2] - l * W[0][2]
        t[r] = t[r] - l * t[0]
    if np.abs(W[2][1]) > np.abs(W[1][1]):
        W[1], W[2] = W[2], W[1]
        t[1], t[2] = t[2], t[1]
    l = W[2][1] / W[1][1]
    W[2][2] = W[2][2] - l * W[1][2]
    t[2] = t[2] - l * t[1]
    x2 = t[2] / W[2][2]
    x1 = (t[1] - W[1][2] * x2) / W[1][1]
    x0 = ((t[0] - W[0][1] * x1) - W[0][2] * x2) / W[0][0]
    return [x0, x1, x2]


class Vertex:
    """VertexSim3Expmap"""

    def __init__(self, estimate, fixed, fix_scale, ch):
        self.estimate, self.fixed, self.fix_scale, self.ch = estimate, fixed, fix_scale, ch
        self.hidx = -1
        self.stack = []

    def push(self):
        self.stack.append(self.estimate)

    def pop(self):
        self.estimate = self.stack.pop()

    def discard_top(self):
        self.stack.pop()

    def oplus(self, update):
        """types_seven_dof_expmap.h:60-69: update is the caller's array and is written"""
        if self.fix_scale:
            update[6] = F64(0.0)
        self.estimate = Sim3.exp(update, self.ch) * self.estimate


class Edge:
    """EdgeSim3, information = identity"""

    def __init__(self, v0, v1, meas, ch):
        self.v = (v0, v1)
        self.meas, self.ch = meas, ch
        self.error = [F64(0.0)] * 7
        self.J = [None, None]

    def compute_error(self):
        e = self.meas * self.v[0].estimate * self.v[1].estimate.inverse()
        self.error = e.log(self.ch)

    def chi2(self):
        c = self.error[0] * self.error[0]
        for k in range(1, 7):
            c = c + self.error[k] * self.error[k]
        return c

    def linearize_oplus(self):
        """base_binary_edge.hpp:131-205"""
        delta = F64(1e-9)
        scalar = F64(1.0) / (2 * delta)
        backup = self.error
        for side in range(2):
            v = self.v[side]
            if v.fixed:
                continue
            J = [[None] * 7 for _ in range(7)]
            for d in range(7):
                add = [F64(0.0)] * 7
                v.push()
                add[d] = delta
                v.oplus(add)
                self.compute_error()
                e1 = self.error
                v.pop()
                add = [F64(0.0)] * 7
                v.push()
                add[d] = -delta
                v.oplus(add)
                self.compute_error()
                e2 = self.error
                v.pop()
                for k in range(7):
                    J[k][d] = scalar * (e1[k] - e2[k])
            self.J[side] = J
        self.error = backup


def dot(X, a, Y, b):
    v = X[0][a] * Y[0][b]
    for k in range(1, 7):
        v = v + X[k][a] * Y[k][b]
    return v


def ldlt_entrywise(S, b):
    """departure (g) as written: entry (i, j) subtracts L_ik (L_jk d_k) for k ascending, then divides by d_j"""
    n = len(b)
    L = np.zeros((n, n), F64)
    d = np.zeros(n, F64)
    ok = True
    for j in range(n):
        col = np.array([S[j, i] for i in range(j, n)], F64)             # the upper triangle is what is stored
        for k in range(j):
            col = col - L[j:, k] * (L[j, k] * d[k])
        d[j] = col[0]
        if not np.isfinite(d[j]) or d[j] == 0.0:
            ok = False
        L[j + 1:, j] = col[1:] / d[j]
        if not np.all(np.isfinite(L[j + 1:, j])):
            ok = False
    if not ok:
        return False, None
    y = np.array(b, F64)
    for i in range(n):
        for k in range(i):
            y[i] = y[i] - L[i, k] * y[k]
    for i in range(n):
        y[i] = y[i] / d[i]
    for i in range(n - 1, -1, -1):
        for k in range(n - 1, i, -1):
            y[i] = y[i] - L[k, i] * y[k]
    y = y + 0.0
    if not np.all(np.isfinite(y)):
        return False, None
    return True, y


def essential_graph(c, P=None, ch=None):
    P = R.params() if P is None else P
    ch = Choices() if ch is None else ch
    with np.errstate(all="ignore"):
        return _essential_graph(c, P, ch)


def _essential_graph(c, P, ch):
    R.check(c, P)
    N, E = len(c["s_est"]), len(c["edge_i"])
    vScw = [Sim3.from_row(list(r)) for r in np.asarray(c["s_est"], F64)]
    vMeas = [Sim3.from_row(list(r)) for r in np.asarray(c["s_meas"], F64)]
    vertices = [Vertex(vScw[i], bool(c["fixed"][i]), P["fix_scale"], ch) for i in range(N)]
    n = 0
    for v in vertices:                                        # buildStructure: the non-fixed vertices in ascending id
        if not v.fixed:
            v.hidx = n
            n += 1
    edges = []
    for e in range(E):
        i, j = int(c["edge_i"][e]), int(c["edge_j"][e])
        src = vScw if c["edge_from_est"][e] else vMeas
        edges.append(Edge(vertices[i], vertices[j], src[j] * src[i].inverse(), ch))
    free = [v for v in vertices if not v.fixed]
    n7 = 7 * n

    def compute_active_errors():
        for ed in edges:
            ed.compute_error()

    def active_chi2():
        return ch.total([ed.chi2() for ed in edges])

    def build_system():
        for ed in edges:
            ed.linearize_oplus()
        H = np.zeros((n7, n7), F64)
        b = np.zeros(n7, F64)
        for ed in edges:                                      # constructQuadraticForm, base_binary_edge.hpp:55-120
            v0, v1 = ed.v
            A, B = ed.J
            omega_r = [-ed.error[k] for k in range(7)]
            if not v0.fixed:
                o = 7 * v0.hidx
                for a in range(7):
                    g = A[0][a] * omega_r[0]
                    for k in range(1, 7):
                        g = g + A[k][a] * omega_r[k]
                    b[o + a] = b[o + a] + g
                    for bb in range(a, 7):
                        H[o + a, o + bb] = H[o + a, o + bb] + dot(A, a, A, bb)
                if not v1.fixed:
                    o1 = 7 * v1.hidx
                    for a in range(7):
                        for bb in range(7):
                            if v0.hidx < v1.hidx:
                                H[o + a, o1 + bb] = H[o + a, o1 + bb] + dot(A, a, B, bb)      # _hessian += AtO B
                            else:
                                H[o1 + bb, o + a] = H[o1 + bb, o + a] + dot(A, a, B, bb)      # _hessianTransposed += B^T AtO^T
            if not v1.fixed:
                o = 7 * v1.hidx
                for a in range(7):
                    g = B[0][a] * omega_r[0]
                    for k in range(1, 7):
                        g = g + B[k][a] * omega_r[k]
                    b[o + a] = b[o + a] + g
                    for bb in range(a, 7):
                        H[o + a, o + bb] = H[o + a, o + bb] + dot(B, a, B, bb)
        return H, b

    max_trials = P["max_trials"] if P["max_trials"] > 0 else 10
    trace, stats = np.zeros((P["iterations"], 4), F64), np.zeros(8, np.int32)
    flags = iters = trials = rejected = failed = 0
    ended_rejected = False
    x = np.zeros(n7, F64)
    lam, ni, nbad = F64(0.0), F64(2.0), 0
    for it in range(P["iterations"]):
        iters += 1
        compute_active_errors()
        current = active_chi2()
        ini = current
        H, b = build_system()
        if it == 0:
            if P["user_lambda_init"] > 0:
                lam = F64(P["user_lambda_init"])
            else:
                m = F64(0.0)
                for k in range(n7):
                    if np.abs(H[k, k]) > m:
                        m = np.abs(H[k, k])
                lam = 1e-5 * m
            ni, nbad = F64(2.0), 0
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            for v in free:
                v.push()
            S = H.copy()
            for k in range(n7):
                S[k, k] = S[k, k] + lam
            if ch.ldlt:
                ok, sol = ldlt_entrywise(S, b) if n7 else (True, np.zeros(0, F64))
            else:
                full = np.triu(S) + np.triu(S, 1).T
                sol = np.linalg.solve(full, b) if n7 else np.zeros(0, F64)
                ok = bool(np.all(np.isfinite(sol)))
            if ok:
                x = sol
            else:
                failed += 1
                flags |= R.FLAG_SOLVE_FAILED
            for v in free:
                u = [F64(t) for t in x[7 * v.hidx:7 * v.hidx + 7]]
                v.oplus(u)
                x[7 * v.hidx:7 * v.hidx + 7] = u              # oplusImpl writes update[6] = 0 into the solver's x
            if not all(np.all(np.isfinite(v.estimate.row())) for v in vertices):
                flags |= R.FLAG_NONFINITE
            compute_active_errors()
            temp = active_chi2()
            if not ok:
                temp = F64(R.DBL_MAX)
            scale = ch.total(list(x * (lam * x + b))) + 1e-3
            rho = (current - temp) / scale
            if rho > 0 and np.isfinite(temp):
                v_ = 2 * rho - 1
                alpha = 1.0 - (v_ * v_) * v_
                alpha = F64(2.0 / 3.0) if F64(2.0 / 3.0) < alpha else alpha
                lam = lam * (alpha if F64(1.0 / 3.0) < alpha else F64(1.0 / 3.0))
                ni = F64(2.0)
                current = temp
                for v in free:
                    v.discard_top()
                ended_rejected = False
            else:
                lam = lam * ni
                ni = ni * 2
                for v in free:
                    v.pop()
                rejected += 1
                ended_rejected = True
            qmax += 1
            if not (rho < 0 and qmax < max_trials):
                break
        trace[it] = [qmax, lam, current, 0.0]
        if qmax == max_trials or rho == 0:
            break
        if (ini - current) * 1e3 < ini:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            break
    if iters == 0:
        flags |= R.FLAG_NO_ITERATION
    if ended_rejected:
        flags |= R.FLAG_ENDED_REJECTED
    compute_active_errors()
    chi2 = np.array([ed.chi2() for ed in edges], F64)
    # write-back, Optimizer.cc:4787-4836
    siw = np.array([v.estimate.row() for v in vertices], F64)
    if not np.all(np.isfinite(siw)):
        flags |= R.FLAG_NONFINITE
    vCorrectedSwc = [v.estimate.inverse() for v in vertices]
    swi = np.array([s.row() for s in vCorrectedSwc], F64)
    tiw = np.zeros((N, 7), F32)
    for i, v in enumerate(vertices):
        s = F32(v.estimate.s)
        tiw[i, :4] = [F32(q) for q in v.estimate.r]
        tiw[i, 4:] = [F32(t) / s for t in v.estimate.t]
    xw = np.asarray(c["xw"], F32).reshape(-1, 3)
    out = xw.copy()
    for l in range(len(xw)):
        r = int(c["point_ref"][l])
        if r < 0:
            continue
        out[l] = [F32(v) for v in vCorrectedSwc[r].map(vScw[r].map([F64(v) for v in xw[l]]))]
    stats[:6] = [iters, trials, rejected, failed, flags, n]
    return {"siw": siw, "tiw_f32": tiw, "swi": swi, "xw_out": out, "chi2": chi2, "trace": trace, "stats": stats, "ret": iters}
