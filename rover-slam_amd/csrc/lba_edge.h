// lba_edge.h -- the per-edge mathematics local_ba.hip and global_ba.hip (6n) share: one observation's inputs, computeError
// with chi2() and the kernel's rho, and linearizeOplus with constructQuadraticForm (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ, vertex 0
// the point, vertex 1 the pose).  Dev is LbaDev or GbaDev: both name the inputs, the estimates and lin / chi2 / rho0 alike.  ROBUST true is
// base_binary_edge.hpp:91-113 under RobustKernelHuber, false :75-90 with no kernel.  Everything is double, one rounding per operation.
#pragma once
#include "rfe_internal.h"
#include "lm_device.h"

namespace rfe {

struct LbaEdge {
    double X[3], q[7], fx, fy, cx, cy, bf, u, v, ur, isg;
    bool stereo;
    int p, k;
};

template <class Dev>
__device__ inline LbaEdge lba_load(const Dev& d, int e, int cur) {
    LbaEdge E;
    E.p = d.edge_point[e]; E.k = d.edge_kf[e];
    const int f = d.kf_feat_off[E.k] + d.edge_feat[e];
    const double* X = d.pt[cur] + 3 * (size_t)E.p;
    E.X[0] = X[0]; E.X[1] = X[1]; E.X[2] = X[2];
    const double* q = d.pose[cur] + 7 * (size_t)E.k;
    for (int i = 0; i < 7; ++i) E.q[i] = q[i];
    const float* c = d.kf_cam + 5 * (size_t)E.k;
    E.fx = (double)c[0]; E.fy = (double)c[1]; E.cx = (double)c[2]; E.cy = (double)c[3]; E.bf = (double)c[4];
    E.u = (double)d.kpts[2 * (size_t)f]; E.v = (double)d.kpts[2 * (size_t)f + 1];
    const float ur = d.uright ? d.uright[f] : -1.f;
    E.stereo = !(ur < 0);
    E.ur = (double)ur;
    int o = d.octave ? d.octave[f] : 0;
    if (o < 0 || o >= d.kf_nlevels[E.k]) o = 0;
    E.isg = (double)d.kf_sigma2[RFE_MAX_LEVELS * (size_t)E.k + o];
    return E;
}

// computeError, chi2() and the kernel's rho at the edge's estimates; x y z: the point in the camera frame.  Without a kernel
// activeRobustChi2 is chi2 itself and rho' is 1
template <bool ROBUST, class Dev>
__device__ inline double lba_error(const Dev& d, const LbaEdge& E, double& x, double& y, double& z, double (&e)[3], double& rho0, double& rho1) {
    po_rotate(E.q, E.X[0], E.X[1], E.X[2], x, y, z);
    x = x + E.q[4]; y = y + E.q[5]; z = z + E.q[6];
    double chi2;
    if (E.stereo) {
        const double invz = (double)(float)(1.0 / z);
        const double pu = x * invz * E.fx + E.cx;
        const double pv = y * invz * E.fy + E.cy;
        const double pr = pu - E.bf * invz;
        e[0] = E.u - pu; e[1] = E.v - pv; e[2] = E.ur - pr;
        chi2 = e[0] * (E.isg * e[0]) + e[1] * (E.isg * e[1]);
        chi2 = chi2 + e[2] * (E.isg * e[2]);
    } else {
        e[0] = E.u - (E.fx * x / z + E.cx);
        e[1] = E.v - (E.fy * y / z + E.cy);
        e[2] = 0.0;
        chi2 = e[0] * (E.isg * e[0]) + e[1] * (E.isg * e[1]);
    }
    rho0 = chi2; rho1 = 1.0;
    if (ROBUST) {
        const double delta = E.stereo ? d.delta_stereo : d.delta_mono, dsqr = E.stereo ? d.dsqr_stereo : d.dsqr_mono;
        if (!(chi2 <= dsqr)) {
            const double sq = sqrt(chi2);
            rho0 = 2 * sq * delta - dsqr;
            rho1 = delta / sq;
        }
    }
    return chi2;
}

// computeActiveErrors, linearizeOplus and constructQuadraticForm of edge e at estimate `cur`: its finished contributions go to
// lin [LBA_LIN][E]: 0-5 Hll's upper triangle, 6-8 bl, 9-29 Hpp's upper triangle, 30-35 bp, 36-53 the stored 6 x 3 Hpl block.  free_pose
// false: the keyframe is fixed, the point's terms only.  ROBUST: (U^T wOmega) V with wOmega = rho' invSigma2.  Otherwise AtO = A^T Omega
// is rounded first: the point gets AtO A, the pose (B^T Omega) B, and the stored block (_hessianRowMajor) is B^T AtO^T
template <bool ROBUST, class Dev>
__device__ __forceinline__ void lba_linearise_edge(const Dev& d, int e, int cur, const LbaEdge& E, bool free_pose) {
    double x, y, z, er[3], rho0, rho1;
    d.chi2[e] = lba_error<ROBUST>(d, E, x, y, z, er, rho0, rho1);
    d.rho0[e] = rho0;
    // Eigen's toRotationMatrix
    const double qx = E.q[0], qy = E.q[1], qz = E.q[2], qw = E.q[3];
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const double R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}};
    double Xi[3][3], Xj[3][6];
    const double fx = E.fx, fy = E.fy, bf = E.bf;
    if (E.stereo) {
        const double z_2 = z * z;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Xi[0][c] = -fx * R[0][c] / z + fx * x * R[2][c] / z_2;
            Xi[1][c] = -fy * R[1][c] / z + fy * y * R[2][c] / z_2;
            Xi[2][c] = Xi[0][c] - bf * R[2][c] / z_2;
        }
        Xj[0][0] = x * y / z_2 * fx;
        Xj[0][1] = -(1 + (x * x / z_2)) * fx;
        Xj[0][2] = y / z * fx;
        Xj[0][3] = -1. / z * fx;
        Xj[0][4] = 0;
        Xj[0][5] = x / z_2 * fx;
        Xj[1][0] = (1 + y * y / z_2) * fy;
        Xj[1][1] = -x * y / z_2 * fy;
        Xj[1][2] = -x / z * fy;
        Xj[1][3] = 0;
        Xj[1][4] = -1. / z * fy;
        Xj[1][5] = y / z_2 * fy;
        Xj[2][0] = Xj[0][0] - bf * y / z_2;
        Xj[2][1] = Xj[0][1] + bf * x / z_2;
        Xj[2][2] = Xj[0][2];
        Xj[2][3] = Xj[0][3];
        Xj[2][4] = 0;
        Xj[2][5] = Xj[0][5] - bf / z_2;
    } else {
        const double nJ[2][3] = {{-(fx / z), -0.0, -(-fx * x / (z * z))}, {-0.0, -(fy / z), -(-fy * y / (z * z))}};
        const double Sd[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Xi[r][c] = (nJ[r][0] * R[0][c] + nJ[r][1] * R[1][c]) + nJ[r][2] * R[2][c];
#pragma unroll
            for (int c = 0; c < 6; ++c) Xj[r][c] = (nJ[r][0] * Sd[0][c] + nJ[r][1] * Sd[1][c]) + nJ[r][2] * Sd[2][c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) Xi[2][c] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) Xj[2][c] = 0.0;
    }
    const double w = ROBUST ? rho1 * E.isg : E.isg;
    double omr[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) omr[r] = ROBUST ? (-(E.isg * er[r])) * rho1 : -(E.isg * er[r]);
    double* out = d.lin + e;
    const size_t S = (size_t)d.E;
    int col = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double h = (Xi[0][a] * w) * Xi[0][b] + (Xi[1][a] * w) * Xi[1][b];
            if (E.stereo) h = h + (Xi[2][a] * w) * Xi[2][b];
            out[S * col] = h; ++col;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double g = Xi[0][a] * omr[0] + Xi[1][a] * omr[1];
        if (E.stereo) g = g + Xi[2][a] * omr[2];
        out[S * col] = g; ++col;
    }
    if (!free_pose) return;                          // a fixed keyframe: the point's terms only
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            double h = (Xj[0][a] * w) * Xj[0][b] + (Xj[1][a] * w) * Xj[1][b];
            if (E.stereo) h = h + (Xj[2][a] * w) * Xj[2][b];
            out[S * col] = h; ++col;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double g = Xj[0][a] * omr[0] + Xj[1][a] * omr[1];
        if (E.stereo) g = g + Xj[2][a] * omr[2];
        out[S * col] = g; ++col;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            double h;
            if (ROBUST) {
                h = (Xj[0][a] * w) * Xi[0][b] + (Xj[1][a] * w) * Xi[1][b];
                if (E.stereo) h = h + (Xj[2][a] * w) * Xi[2][b];
            } else {
                h = Xj[0][a] * (Xi[0][b] * w) + Xj[1][a] * (Xi[1][b] * w);
                if (E.stereo) h = h + Xj[2][a] * (Xi[2][b] * w);
            }
            out[S * col] = 0.0 + h; ++col;               // the block is cleared and this edge is its only += (a -0.0 becomes +0.0)
        }
}

}  // namespace rfe
