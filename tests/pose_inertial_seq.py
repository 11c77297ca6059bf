"""A sequential transcription of Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (reference src/Optimizer.cc:416-968,
:983-1623, Marginalize :1644-1725; G2oTypes.cc / G2oTypes.h for ImuCamPose, the vertices and the edges; ImuTypes.cc:377-427; g2o's
sparse_optimizer.cpp, optimization_algorithm_gauss_newton.cpp:50-93, base_unary_edge.hpp / base_multi_edge.hpp and
linear_solver_dense.h): one object per vertex and per edge with computeError / linearizeOplus / constructQuadraticForm, the optimizer's
initializeOptimization / optimize loop and the two functions statement by statement.  Written from the reference's lines, not from
tests/pose_inertial_ref.py; it shares with it only what the contract calls a departure, through Choices: with ours=True the sums over
the visual edges, sin / cos / acos, the eigen-solver, the nearest rotation, the inverses, the dense solve and the order of small
products are the contract's (taken from pose_inertial_ref), with ours=False they are the reference's own (edge after edge, libm,
numpy.linalg.eigh / svd / inv / solve, BLAS).  test_pose_inertial_ref.py holds the two against each other."""
import math

import numpy as np

import pose_inertial_ref as R

F32, F64 = np.float32, np.float64


class Choices:
    def __init__(self, ours):
        self.ours = ours

    def sincos(self, t):
        if self.ours:
            s, c = R.sincos(t)
            return F64(s), F64(c)
        return F64(math.sin(t)), F64(math.cos(t))

    def acos(self, x):
        return R.acos(x) if self.ours else F64(np.arccos(x))

    def mm(self, A, B):
        return R.mm(A, B) if self.ours else np.asarray(A) @ np.asarray(B)

    def mv(self, A, x):
        return self.mm(A, np.asarray(x).reshape(-1, 1))[:, 0]

    def eig(self, M, n):
        """SelfAdjointEigenSolver: (eigenvalues, eigenvectors as columns); reads the lower triangle"""
        return R.jacobi_eig(M, n) if self.ours else np.linalg.eigh(np.asarray(M, F64), UPLO="L")

    def normalize_rotation(self, M):
        """NormalizeRotation: U V^T of the SVD"""
        if self.ours:
            return R.nearest_rotation(M)
        U, _, Vt = np.linalg.svd(np.asarray(M, F64))
        return U @ Vt

    def normalize_rotation_f(self, Mf):
        """the float NormalizeRotation of ImuTypes.cc:39-47"""
        if self.ours:
            return R.nearest_rotation(Mf.astype(F64)).astype(F32)
        U, _, Vt = np.linalg.svd(Mf.astype(F32))
        return (U @ Vt).astype(F32)

    def inverse3(self, M):
        return R.inv3(M) if self.ours else np.linalg.inv(np.asarray(M, F64))

    def inverse9(self, M):
        return R.ldlt_inverse(M, 9) if self.ours else np.linalg.inv(np.asarray(M, F64))

    def solve(self, H, b):
        """LinearSolverDense: an LDLT whose isPositive() decides"""
        D = len(b)
        if self.ours:
            return R.ldlt_solve(H, b, D)
        try:
            np.linalg.cholesky(np.asarray(H, F64))
        except np.linalg.LinAlgError:
            return False, None
        return True, np.linalg.solve(np.asarray(H, F64), np.asarray(b, F64))

    def pinv_block(self, M):
        """Marginalize's JacobiSVD pseudo-inverse with the > 1e-6 cut: (inverse, whether a value was cut)"""
        if self.ours:
            lam, Q = R.jacobi_eig(M, 15)
            keep = np.abs(lam) > 1e-6
            return R.recompose(Q, np.where(keep, 1.0 / lam, 0.0)), not keep.all()
        U, sv, Vt = np.linalg.svd(np.asarray(M, F64))
        keep = sv > 1e-6
        return (Vt.T * np.where(keep, 1.0 / np.where(keep, sv, 1.0), 0.0)[None, :]) @ U.T, not keep.all()

    def recompose(self, V, d):
        return R.recompose(V, d) if self.ours else (V * d[None, :]) @ V.T

    def total(self, contributions):
        """contributions: (feature index, 28 terms) of the active visual edges in edge order -> their totals"""
        tot = np.zeros(28, F64)
        if not self.ours:                                    # g2o: one edge after the other
            for _, t in contributions:
                tot = tot + t
            return tot
        part = np.zeros((R.LANES, 28), F64)
        for i, t in contributions:                           # ascending feature index into partial i mod 256
            part[i % R.LANES] = part[i % R.LANES] + t
        s = R.LANES // 2
        while s >= 1:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
        return part[0].copy()


EYE3 = np.eye(3, dtype=F64)


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], F64)


# ---------------------------------------------------------------- G2oTypes.cc:908-985
def ExpSO3(ch, w):
    d2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    d = np.sqrt(d2)
    W = skew(w)
    if d < 1e-5:
        res = (EYE3 + W) + ch.mm(0.5 * W, W)
    else:
        s, c = ch.sincos(d)
        res = (EYE3 + (W * s) / d) + (ch.mm(W, W) * (1.0 - c)) / d2
    return ch.normalize_rotation(res)


def LogSO3(ch, Rm):
    tr = (Rm[0, 0] + Rm[1, 1]) + Rm[2, 2]
    w = np.array([(Rm[2, 1] - Rm[1, 2]) / 2, (Rm[0, 2] - Rm[2, 0]) / 2, (Rm[1, 0] - Rm[0, 1]) / 2], F64)
    costheta = (tr - 1.0) * 0.5
    if costheta > 1 or costheta < -1:
        return w
    theta = ch.acos(costheta)
    s, _ = ch.sincos(theta)
    if abs(s) < 1e-5:
        return w
    return (theta * w) / s


def InverseRightJacobianSO3(ch, v):
    d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    d = np.sqrt(d2)
    W = skew(v)
    if d < 1e-5:
        return EYE3.copy()
    s, c = ch.sincos(d)
    return (EYE3 + W / 2) + ch.mm(W, W) * (1.0 / d2 - (1.0 + c) / ((2.0 * d) * s))


def RightJacobianSO3(ch, v):
    d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    d = np.sqrt(d2)
    W = skew(v)
    if d < 1e-5:
        return EYE3.copy()
    s, c = ch.sincos(d)
    return (EYE3 - (W * (1.0 - c)) / d2) + (ch.mm(W, W) * (d - s)) / (d2 * d)


# ---------------------------------------------------------------- ImuTypes.cc:377-427 (float)
class Preintegrated:
    def __init__(self, ch, p):
        self.ch = ch
        p = np.asarray(p, F32)
        self.dT, self.dR, self.dV, self.dP = p[0], p[1:10].reshape(3, 3), p[10:13], p[13:16]
        self.JRg, self.JVg, self.JVa = p[16:25].reshape(3, 3), p[25:34].reshape(3, 3), p[34:43].reshape(3, 3)
        self.JPg, self.JPa = p[43:52].reshape(3, 3), p[52:61].reshape(3, 3)
        self.ba, self.bg = p[61:64], p[64:67]                # IMU::Bias b: bax bay baz, bwx bwy bwz
        self.C9 = p[67:148].reshape(9, 9)

    def so3f_exp(self, om):
        """Sophus::SO3f::exp(om).matrix() (so3.hpp:583-619, Eigen's toRotationMatrix)"""
        ch = self.ch
        theta_sq = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
        if theta_sq < F32(1e-5) * F32(1e-5):
            po4 = theta_sq * theta_sq
            imag = (F32(0.5) - F32(1.0 / 48.0) * theta_sq) + F32(1.0 / 3840.0) * po4
            real = (F32(1) - F32(1.0 / 8.0) * theta_sq) + F32(1.0 / 384.0) * po4
        else:
            theta = np.sqrt(theta_sq)
            half = F32(0.5) * theta
            if ch.ours:
                s, c = ch.sincos(F64(half))
                s, c = F32(s), F32(c)
            else:
                s, c = np.sin(half), np.cos(half)
            imag, real = s / theta, c
        w, x, y, z = real, imag * om[0], imag * om[1], imag * om[2]
        tx, ty, tz = F32(2) * x, F32(2) * y, F32(2) * z
        twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
        one = F32(1)
        return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                         [txz - twy, tyz + twx, one - (txx + tyy)]], F32)

    def delta_bias(self, bg, ba):
        """GetDeltaBias of IMU::Bias(b_) whose members are the float casts of the double estimates"""
        return np.asarray(bg, F64).astype(F32) - self.bg, np.asarray(ba, F64).astype(F32) - self.ba

    def GetDeltaRotation(self, bg, ba):
        dbg, _ = self.delta_bias(bg, ba)
        return self.ch.normalize_rotation_f(self.ch.mm(self.dR, self.so3f_exp(self.ch.mv(self.JRg, dbg))))

    def GetDeltaVelocity(self, bg, ba):
        dbg, dba = self.delta_bias(bg, ba)
        return (self.dV + self.ch.mv(self.JVg, dbg)) + self.ch.mv(self.JVa, dba)

    def GetDeltaPosition(self, bg, ba):
        dbg, dba = self.delta_bias(bg, ba)
        return (self.dP + self.ch.mv(self.JPg, dbg)) + self.ch.mv(self.JPa, dba)


# ---------------------------------------------------------------- vertices
class ImuCamPose:
    """G2oTypes.cc:81-127 and :188-250, one camera"""

    def __init__(self, ch, P, cam, state):
        self.ch, self.P = ch, P
        cam, s = np.asarray(cam, F32).astype(F64), np.asarray(state, F32).astype(F64)
        self.twb, self.Rwb = s[9:12].copy(), s[0:9].reshape(3, 3).copy()
        if cam is not None and len(cam):
            self.tcw, self.Rcw = cam[9:12].copy(), cam[0:9].reshape(3, 3).copy()
            self.tcb, self.Rcb = cam[21:24].copy(), cam[12:21].reshape(3, 3).copy()
            self.Rbc, self.tbc = self.Rcb.T.copy(), cam[33:36].copy()
        self.its = 0

    def Xc(self, Xw):
        return [((self.Rcw[r, 0] * Xw[0] + self.Rcw[r, 1] * Xw[1]) + self.Rcw[r, 2] * Xw[2]) + self.tcw[r] for r in range(3)]

    def Project(self, Xw):
        x, y, z = self.Xc(Xw)
        fx, fy, cx, cy = (F64(self.P[k]) for k in ("fx", "fy", "cx", "cy"))
        return fx * x / z + cx, fy * y / z + cy

    def ProjectStereo(self, Xw):
        x, y, z = self.Xc(Xw)
        invZ = 1.0 / z
        u, v = self.Project(Xw)
        return u, v, u - F64(self.P["bf"]) * invZ

    def isDepthPositive(self, Xw):
        return (((self.Rcw[2, 0] * Xw[0] + self.Rcw[2, 1] * Xw[1]) + self.Rcw[2, 2] * Xw[2]) + self.tcw[2]) > 0.0

    def Update(self, pu, camera=True):
        ch = self.ch
        ur, ut = np.asarray(pu[0:3], F64), np.asarray(pu[3:6], F64)
        self.twb = self.twb + ch.mv(self.Rwb, ut)
        self.Rwb = ch.mm(self.Rwb, ExpSO3(ch, ur))
        self.its += 1
        if self.its >= 3:
            ch.normalize_rotation(self.Rwb)                  # NormalizeRotation(Rwb): the result is discarded (:236)
            self.its = 0
        if camera:
            Rbw = self.Rwb.T
            tbw = ch.mv(-Rbw, self.twb)
            self.Rcw = ch.mm(self.Rcb, Rbw)
            self.tcw = ch.mv(self.Rcb, tbw) + self.tcb


class Vertex:
    def __init__(self, vid, dim, estimate, fixed, pose=False):
        self.id, self.dim, self.estimate, self.fixed, self.pose, self.hidx = vid, dim, estimate, fixed, pose, -1

    def oplus(self, u):
        if self.pose:
            self.estimate.Update(u, camera=hasattr(self.estimate, "Rcb"))
        else:
            self.estimate = self.estimate + np.asarray(u, F64)


# ---------------------------------------------------------------- edges
DELTA = {False: R.DELTA_MONO, True: R.DELTA_STEREO}
DSQR = {False: R.DSQR_MONO, True: R.DSQR_STEREO}


class EdgeVisual:
    """EdgeMonoOnlyPose / EdgeStereoOnlyPose (G2oTypes.h:457-571, G2oTypes.cc:434-454, :497-522)"""

    def __init__(self, idx, VP, Xw, obs, inv_sigma2, stereo):
        self.idx, self.VP, self.Xw, self.obs, self.info, self.stereo = idx, VP, [F64(v) for v in Xw], [F64(v) for v in obs], F64(inv_sigma2), stereo
        self.level, self.robust, self.error = 0, True, None

    def computeError(self):
        est = self.VP.estimate
        proj = est.ProjectStereo(self.Xw) if self.stereo else est.Project(self.Xw)
        self.error = [self.obs[k] - proj[k] for k in range(len(proj))]

    def chi2(self):
        e, w = self.error, self.info
        c = e[0] * (w * e[0]) + e[1] * (w * e[1])
        return c + e[2] * (w * e[2]) if self.stereo else c

    def isDepthPositive(self):
        return self.VP.estimate.isDepthPositive(self.Xw)

    def linearizeOplus(self):
        est = self.VP.estimate
        x, y, z = est.Xc(self.Xw)
        Rbc, tbc, Rcb = est.Rbc, est.tbc, est.Rcb
        xb, yb, zb = [((Rbc[r, 0] * x + Rbc[r, 1] * y) + Rbc[r, 2] * z) + tbc[r] for r in range(3)]
        fx, fy, bf = F64(est.P["fx"]), F64(est.P["fy"]), F64(est.P["bf"])
        zz = z * z
        pj = [[fx / z, F64(0.0), -fx * x / zz], [F64(0.0), fy / z, -fy * y / zz]]
        if self.stereo:
            pj.append([pj[0][0], pj[0][1], pj[0][2] + bf * (1.0 / zz)])
        PR = [[(pj[r][0] * Rcb[0, c] + pj[r][1] * Rcb[1, c]) + pj[r][2] * Rcb[2, c] for c in range(3)] for r in range(len(pj))]
        S = [[0.0, zb, -yb, 1.0, 0.0, 0.0], [-zb, 0.0, xb, 0.0, 1.0, 0.0], [yb, -xb, 0.0, 0.0, 0.0, 1.0]]
        self.J = [[(PR[r][0] * S[0][c] + PR[r][1] * S[1][c]) + PR[r][2] * S[2][c] for c in range(6)] for r in range(len(pj))]

    def quadratic_form(self):
        """base_unary_edge.hpp:44-72 with RobustKernelHuber: the 21 entries of A^T (rho1 Omega) A, the 6 of rho1 A^T Omega e, rho0"""
        e, A, w0 = self.error, self.J, self.info
        chi2 = self.chi2()
        rho0, rho1 = chi2, F64(1.0)
        if self.robust:
            delta, dsqr = DELTA[self.stereo], DSQR[self.stereo]
            if not (chi2 <= dsqr):
                sq = np.sqrt(chi2)
                rho0, rho1 = 2 * sq * delta - dsqr, delta / sq
        w = rho1 * w0
        t = np.zeros(28, F64)
        col = 0
        for j in range(6):
            for k in range(j, 6):
                h = (A[0][j] * w) * A[0][k] + (A[1][j] * w) * A[1][k]
                t[col] = h + (A[2][j] * w) * A[2][k] if self.stereo else h
                col += 1
        for j in range(6):
            g = ((rho1 * A[0][j]) * w0) * e[0] + ((rho1 * A[1][j]) * w0) * e[1]
            t[col] = g + ((rho1 * A[2][j]) * w0) * e[2] if self.stereo else g
            col += 1
        t[27] = rho0
        return t

    def GetHessian(self):
        self.linearizeOplus()
        keep = self.robust
        self.robust = False
        if self.error is None:
            self.computeError()
        t = self.quadratic_form()
        self.robust = keep
        return t


class EdgeMulti:
    """what base_multi_edge.hpp:constructQuadraticForm does for the edges below: J [R, C] over `verts` in order, information Om"""
    delta = None

    def chi2(self):
        Oe = self.ch.mv(self.Om, self.error)
        acc = self.error[0] * Oe[0]
        for r in range(1, len(self.error)):
            acc = acc + self.error[r] * Oe[r]
        return acc

    def quadratic_form(self):
        ch = self.ch
        Oe = ch.mv(self.Om, self.error)
        chi2 = self.chi2()
        rho0, rho1 = chi2, F64(1.0)
        if self.delta is not None:
            dsqr = self.delta * self.delta
            if not (chi2 <= dsqr):
                sq = np.sqrt(chi2)
                rho0, rho1 = 2 * sq * self.delta - dsqr, self.delta / sq
        JtO = ch.mm(self.J.T, rho1 * self.Om)
        return ch.mm(JtO, self.J), ch.mv(self.J.T, rho1 * Oe), rho0, rho1

    def GetHessian(self):
        self.linearizeOplus()
        return self.ch.mm(self.ch.mm(self.J.T, self.Om), self.J)


class EdgeInertial(EdgeMulti):
    """G2oTypes.cc:563-686"""

    def __init__(self, ch, pInt, verts):
        self.ch, self.pInt, self.verts, self.dt = ch, pInt, verts, F64(pInt.dT)
        self.g = np.array([0.0, 0.0, -F64(F32(9.81))], F64)
        Info = ch.inverse9(pInt.C9.astype(F64))
        Info = (Info + Info.T) / 2
        lam, V = ch.eig(Info, 9)
        self.clipped = bool((lam < 1e-12).any())
        self.Om = ch.recompose(V, np.where(lam < 1e-12, 0.0, lam))

    def _parts(self):
        VP1, VV1, VG1, VA1, VP2, VV2 = (v.estimate for v in self.verts)
        return VP1, VV1, VG1, VA1, VP2, VV2

    def computeError(self):
        ch = self.ch
        VP1, VV1, VG1, VA1, VP2, VV2 = self._parts()
        dR = self.pInt.GetDeltaRotation(VG1, VA1).astype(F64)
        dV = self.pInt.GetDeltaVelocity(VG1, VA1).astype(F64)
        dP = self.pInt.GetDeltaPosition(VG1, VA1).astype(F64)
        dt, g = self.dt, self.g
        er = LogSO3(ch, ch.mm(ch.mm(dR.T, VP1.Rwb.T), VP2.Rwb))
        ev = ch.mv(VP1.Rwb.T, (VV2 - VV1) - g * dt) - dV
        ep = ch.mv(VP1.Rwb.T, ((VP2.twb - VP1.twb) - VV1 * dt) - ((g * dt) * dt) / 2) - dP
        self.error = np.concatenate([er, ev, ep])

    def linearizeOplus(self):
        ch = self.ch
        VP1, VV1, VG1, VA1, VP2, VV2 = self._parts()
        dbg = self.pInt.delta_bias(VG1, VA1)[0].astype(F64)
        Rwb1, Rbw1, Rwb2 = VP1.Rwb, VP1.Rwb.T, VP2.Rwb
        dt, g = self.dt, self.g
        dR = self.pInt.GetDeltaRotation(VG1, VA1).astype(F64)
        eR = ch.mm(ch.mm(dR.T, Rbw1), Rwb2)
        er = LogSO3(ch, eR)
        invJr = InverseRightJacobianSO3(ch, er)
        J = np.zeros((9, 24), F64)
        J[0:3, 0:3] = ch.mm(ch.mm(-invJr, Rwb2.T), Rwb1)
        J[3:6, 0:3] = skew(ch.mv(Rbw1, (VV2 - VV1) - g * dt))
        J[6:9, 0:3] = skew(ch.mv(Rbw1, ((VP2.twb - VP1.twb) - VV1 * dt) - ((0.5 * g) * dt) * dt))
        J[6:9, 3:6] = -EYE3
        J[3:6, 6:9] = -Rbw1
        J[6:9, 6:9] = -Rbw1 * dt
        JRg = self.pInt.JRg.astype(F64)
        J[0:3, 9:12] = ch.mm(ch.mm(ch.mm(-invJr, eR.T), RightJacobianSO3(ch, ch.mv(JRg, dbg))), JRg)
        J[3:6, 9:12] = -self.pInt.JVg.astype(F64)
        J[6:9, 9:12] = -self.pInt.JPg.astype(F64)
        J[3:6, 12:15] = -self.pInt.JVa.astype(F64)
        J[6:9, 12:15] = -self.pInt.JPa.astype(F64)
        J[0:3, 15:18] = invJr
        J[6:9, 18:21] = ch.mm(Rbw1, Rwb2)
        J[3:6, 21:24] = Rbw1
        self.J = J


class EdgeRW(EdgeMulti):
    """EdgeGyroRW / EdgeAccRW (G2oTypes.h:736-815): error = second - first, Jacobians -I and I"""

    def __init__(self, ch, verts, Om):
        self.ch, self.verts, self.Om = ch, verts, Om
        self.J = np.concatenate([-EYE3, EYE3], 1)

    def computeError(self):
        self.error = self.verts[1].estimate - self.verts[0].estimate

    def linearizeOplus(self):
        pass


class EdgePriorPoseImu(EdgeMulti):
    """G2oTypes.cc:841-891"""
    delta = F64(5.0)

    def __init__(self, ch, prior, verts):
        self.ch, self.verts = ch, verts
        p = np.asarray(prior, F64)
        self.Rwb, self.twb, self.vwb, self.bg, self.ba = p[0:9].reshape(3, 3).copy(), p[9:12].copy(), p[12:15].copy(), p[15:18].copy(), p[18:21].copy()
        self.Om = p[21:246].reshape(15, 15).copy()

    def computeError(self):
        ch = self.ch
        VP, VV, VG, VA = (v.estimate for v in self.verts)
        er = LogSO3(ch, ch.mm(self.Rwb.T, VP.Rwb))
        et = ch.mv(self.Rwb.T, VP.twb - self.twb)
        self.error = np.concatenate([er, et, VV - self.vwb, VG - self.bg, VA - self.ba])

    def linearizeOplus(self):
        ch = self.ch
        VP = self.verts[0].estimate
        RtR = ch.mm(self.Rwb.T, VP.Rwb)
        er = LogSO3(ch, RtR)
        J = np.zeros((15, 15), F64)
        J[0:3, 0:3] = InverseRightJacobianSO3(ch, er)
        J[3:6, 3:6] = RtR
        J[6:15, 6:15] = np.eye(9)
        self.J = J


# ---------------------------------------------------------------- the optimizer (sparse_optimizer.cpp, gauss_newton.cpp, linear_solver_dense.h)
class SparseOptimizer:
    def __init__(self, ch):
        self.ch, self.vertices, self.visual, self.others = ch, [], [], []
        self.x = None
        self.log = []                                        # per optimize(): (iterations run, first chi2, last chi2, every solve ok)
        self.huber = False

    def addVertex(self, v):
        self.vertices.append(v)

    def edges(self):
        return len(self.visual) + len(self.others)

    def initializeOptimization(self, level=0):
        self.active = [e for e in self.visual if e.level == level]
        n = 0
        for v in sorted(self.vertices, key=lambda v: v.id):
            v.hidx = -1
            if not v.fixed:
                v.hidx = n
                n += v.dim
        self.dim = n
        if self.x is None:
            self.x = np.zeros(30, F64)

    def optimize(self, iterations):
        ch = self.ch
        first = last = F64(0.0)
        ok, done = True, 0
        for it in range(iterations):
            if not ok:
                break
            # computeActiveErrors
            for e in self.active:
                e.computeError()
            for e in self.others:
                e.computeError()
            # buildSystem
            H, b = np.zeros((self.dim, self.dim), F64), np.zeros(self.dim, F64)
            contrib = []
            for e in self.active:
                e.linearizeOplus()
                contrib.append((e.idx, e.quadratic_form()))
            S = ch.total(contrib)
            col = 0
            for j in range(6):
                for k in range(j, 6):
                    H[j, k] = H[k, j] = S[col]
                    col += 1
            for j in range(6):
                b[j] = -S[21 + j]
            total = S[27]
            for e in self.others:
                e.linearizeOplus()
                He, ge, rho0, rho1 = e.quadratic_form()
                if e.delta is not None and rho1 != 1.0:
                    self.huber = True
                total = total + rho0
                cols = []
                for v in e.verts:
                    cols += [(-1 if v.fixed else v.hidx + k) for k in range(v.dim)]
                for a, ia in enumerate(cols):
                    if ia < 0:
                        continue
                    b[ia] = b[ia] - ge[a]
                    for c, ic in enumerate(cols):
                        if ic >= 0:
                            H[ia, ic] = H[ia, ic] + He[a, c]
            if it == 0:
                first = total
            last, done = total, it + 1
            good, sol = ch.solve(H, b)
            if good:
                self.x[:self.dim] = sol
            ok = good
            # update: oplus on every active vertex, whether the solve succeeded or not
            for v in self.vertices:
                if not v.fixed:
                    v.oplus(self.x[v.hidx:v.hidx + v.dim])
        self.log.append((done, first, last, ok))
        return done


def Marginalize(ch, H, start, end):
    """Optimizer.cc:1644-1725 with its reordering, for start = 0"""
    a, b = start, end - start + 1
    c = H.shape[1] - (end + 1)
    Hn = np.zeros_like(H)
    Hn[a:a + c, a:a + c] = H[a + b:, a + b:]
    Hn[a:a + c, a + c:] = H[a + b:, a:a + b]
    Hn[a + c:, a:a + c] = H[a:a + b, a + b:]
    Hn[a + c:, a + c:] = H[a:a + b, a:a + b]
    inv, cut = ch.pinv_block(Hn[a + c:, a + c:])
    Hn[:a + c, :a + c] = Hn[:a + c, :a + c] - ch.mm(ch.mm(Hn[:a + c, a + c:], inv), Hn[a + c:, :a + c])
    Hn[a + c:, a + c:] = 0.0
    Hn[:a + c, a + c:] = 0.0
    Hn[a + c:, :a + c] = 0.0
    res = np.zeros_like(H)
    res[a + b:, a + b:] = Hn[a:a + c, a:a + c]
    return res, cut


def ConstraintPoseImu(ch, H):
    H = (H + H) / 2
    lam, V = ch.eig(H, 15)
    return ch.recompose(V, np.where(lam < 1e-12, 0.0, lam)), bool((lam < 1e-12).any())


# ---------------------------------------------------------------- the two functions
def pose_inertial_optimization(ch, P, mode, rec_init, cam, state, prev_state, preint, cov_rw, prior_in, kpts, octave, uright, xw, has_mp, track_depth,
                               n=None, outlier=None, chi2=None):
    with np.errstate(all="ignore"):
        return _run(ch, P, int(mode), bool(rec_init), cam, state, prev_state, preint, cov_rw, prior_in, kpts, octave, uright, xw, has_mp, track_depth,
                    n, outlier, chi2)


def _run(ch, P, mode, bRecInit, cam, state, prev_state, preint, cov_rw, prior_in, kpts, octave, uright, xw, has_mp, track_depth, n, outlier, chi2):
    last_frame = mode == R.MODE_LAST_FRAME
    N = len(np.asarray(has_mp).reshape(-1))
    n = N if n is None else min(max(int(n), 0), N)
    mvbOutlier = np.zeros(N, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    out_chi2 = np.zeros(N, F32) if chi2 is None else np.array(chi2, F32)
    kpts, xw = np.asarray(kpts, F32).reshape(-1, 2), np.asarray(xw, F32).reshape(-1, 3)
    optimizer = SparseOptimizer(ch)
    s, ps = np.asarray(state, F32).astype(F64), np.asarray(prev_state, F32).astype(F64)
    VP = Vertex(0, 6, ImuCamPose(ch, P, cam, state), False, pose=True)
    VV = Vertex(1, 3, s[12:15].copy(), False)
    VG = Vertex(2, 3, s[15:18].copy(), False)
    VA = Vertex(3, 3, s[18:21].copy(), False)
    for v in (VP, VV, VG, VA):
        optimizer.addVertex(v)
    nInitialMono = nInitialStereo = 0
    for i in range(n):
        if not has_mp[i]:
            continue
        ur = F32(-1.0) if uright is None else F32(uright[i])
        o = 0 if octave is None else int(octave[i])
        if o < 0 or o >= P["nlevels"]:
            o = 0
        inv_sigma2 = F32(P["inv_level_sigma2"][o])
        mvbOutlier[i] = 0
        if ur < 0:
            nInitialMono += 1
            e = EdgeVisual(i, VP, xw[i], kpts[i], inv_sigma2, False)
        else:
            nInitialStereo += 1
            e = EdgeVisual(i, VP, xw[i], [kpts[i][0], kpts[i][1], ur], inv_sigma2, True)
        optimizer.visual.append(e)
    nInitialCorrespondences = nInitialMono + nInitialStereo
    prev_pose = ImuCamPose(ch, P, [], prev_state)
    VPk = Vertex(4, 6, prev_pose, not last_frame, pose=True)
    VVk = Vertex(5, 3, ps[12:15].copy(), not last_frame)
    VGk = Vertex(6, 3, ps[15:18].copy(), not last_frame)
    VAk = Vertex(7, 3, ps[18:21].copy(), not last_frame)
    for v in (VPk, VVk, VGk, VAk):
        optimizer.addVertex(v)
    ei = EdgeInertial(ch, Preintegrated(ch, preint), [VPk, VVk, VGk, VAk, VP, VV])
    cov = np.asarray(cov_rw, F32).astype(F64)
    egr = EdgeRW(ch, [VGk, VG], ch.inverse3(cov[0:9].reshape(3, 3)))
    ear = EdgeRW(ch, [VAk, VA], ch.inverse3(cov[9:18].reshape(3, 3)))
    optimizer.others += [ei, egr, ear]
    ep = None
    if last_frame:
        ep = EdgePriorPoseImu(ch, prior_in, [VPk, VVk, VGk, VAk])
        optimizer.others.append(ep)
    chi2Mono = [F32(5.991)] * 4 if last_frame else [F32(12), F32(7.5), F32(5.991), F32(5.991)]
    chi2Stereo = [F32(15.6), F32(9.8), F32(7.815), F32(7.815)]
    nBad = nInliers = 0
    rounds = 0
    few = False
    chi2_rounds = np.full((5, N), np.nan, F32)
    inl_rounds = []
    for it in range(4):
        optimizer.initializeOptimization(0)
        optimizer.optimize(10)
        nBad = nInliers = 0
        chi2close = F32(1.5 * float(chi2Mono[it]))
        for e in optimizer.visual:
            idx = e.idx
            if mvbOutlier[idx]:
                e.computeError()
            c2 = F32(e.chi2())
            if e.stereo:
                bad = c2 > chi2Stereo[it]
            else:
                bClose = F32(track_depth[idx]) < F32(10.0)
                bad = (c2 > chi2Mono[it] and not bClose) or (bClose and c2 > chi2close) or not e.isDepthPositive()
            mvbOutlier[idx] = 1 if bad else 0
            e.level = 1 if bad else 0
            nBad += 1 if bad else 0
            nInliers += 0 if bad else 1
            out_chi2[idx] = c2
            chi2_rounds[it, idx] = c2
            if it == 2:
                e.robust = False
        rounds += 1
        inl_rounds.append(nInliers)
        if optimizer.edges() < 10:
            few = True
            break
    recovery = nInliers < 30 and not bRecInit
    if recovery:
        nBad = 0
        for e in optimizer.visual:
            e.computeError()
            c2 = F32(e.chi2())
            out_chi2[e.idx] = c2
            chi2_rounds[4, e.idx] = c2
            if c2 < (F32(24.0) if e.stereo else F32(18.0)):
                mvbOutlier[e.idx] = 0
            else:
                nBad += 1
    # the final Hessian
    inl = [(e.idx, e.GetHessian()) for e in optimizer.visual if not mvbOutlier[e.idx] and _recompute(e)]
    Sv = ch.total(inl)
    Hv = np.zeros((6, 6), F64)
    col = 0
    for j in range(6):
        for k in range(j, 6):
            Hv[j, k] = Hv[k, j] = Sv[col]
            col += 1
    Hi = ei.GetHessian()
    cut = False
    if last_frame:
        H = np.zeros((30, 30), F64)
        H[0:24, 0:24] = H[0:24, 0:24] + Hi
        for edge, o1, o2 in ((egr, 9, 24), (ear, 12, 27)):
            Hrw = np.block([[edge.Om, -edge.Om], [-edge.Om, edge.Om]])        # J^T Omega J with J = [-I, I]
            H[o1:o1 + 3, o1:o1 + 3] = H[o1:o1 + 3, o1:o1 + 3] + Hrw[0:3, 0:3]
            H[o1:o1 + 3, o2:o2 + 3] = H[o1:o1 + 3, o2:o2 + 3] + Hrw[0:3, 3:6]
            H[o2:o2 + 3, o1:o1 + 3] = H[o2:o2 + 3, o1:o1 + 3] + Hrw[3:6, 0:3]
            H[o2:o2 + 3, o2:o2 + 3] = H[o2:o2 + 3, o2:o2 + 3] + Hrw[3:6, 3:6]
        H[0:15, 0:15] = H[0:15, 0:15] + ep.GetHessian()
        H[15:21, 15:21] = H[15:21, 15:21] + Hv
        H, cut = Marginalize(ch, H, 0, 14)
        Hf = H[15:30, 15:30]
    else:
        Hf = np.zeros((15, 15), F64)
        Hf[0:9, 0:9] = Hf[0:9, 0:9] + Hi[15:24, 15:24]
        Hf[9:12, 9:12] = Hf[9:12, 9:12] + egr.Om
        Hf[12:15, 12:15] = Hf[12:15, 12:15] + ear.Om
        Hf[0:6, 0:6] = Hf[0:6, 0:6] + Hv
    Hc, clipped = ConstraintPoseImu(ch, Hf)
    est = VP.estimate
    so = np.concatenate([est.Rwb.reshape(-1), est.twb, VV.estimate, VG.estimate, VA.estimate]).astype(F64)
    flags = 0
    fails = sum(0 if lg[3] else 1 for lg in optimizer.log)
    flags |= R.FLAG_SOLVE_FAILED if fails else 0
    flags |= R.FLAG_FEW_EDGES if few else 0
    flags |= R.FLAG_RECOVERY if recovery else 0
    flags |= R.FLAG_INFO_CLIPPED if ei.clipped else 0
    flags |= R.FLAG_MARG_CUT if cut else 0
    flags |= R.FLAG_PRIOR_CLIPPED if clipped else 0
    flags |= R.FLAG_PRIOR_HUBER if optimizer.huber else 0
    if not (R.finite(so) and R.finite(Hc)):
        flags |= R.FLAG_NONFINITE
    trace, stats = np.zeros((4, 8), F64), np.zeros(16, np.int32)
    for r, lg in enumerate(optimizer.log):
        trace[r, 0:5] = [lg[0], lg[1], lg[2], 1.0 if lg[3] else 0.0, inl_rounds[r]]
    stats[:10] = [nInitialCorrespondences - nBad, nInitialCorrespondences, nBad, nInitialMono, nInitialStereo, rounds,
                  sum(lg[0] for lg in optimizer.log), fails, flags, nInliers]
    return {"state": so, "state_f32": so.astype(F32), "outlier": mvbOutlier, "chi2": out_chi2, "prior_out": np.concatenate([so, Hc.reshape(-1)]),
            "trace": trace, "stats": stats, "ret": int(stats[0]), "chi2_rounds": chi2_rounds}


def _recompute(e):
    """GetHessian linearises at the final estimate; its information-weighted product needs no error, but quadratic_form reads one"""
    e.computeError()
    return True


def solve(ch, c, **kw):
    return pose_inertial_optimization(ch, c["P"], **dict(c["args"], **kw))
