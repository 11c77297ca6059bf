// pose_inertial.hip -- Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (reference src/Optimizer.cc:416-968, :983-1623 with
// Marginalize :1644-1725, over g2o's Gauss-Newton and LinearSolverDense), DESIGN.md 6p.  One workgroup of 256 lanes per problem, as in
// pose_opt.hip: lane l owns the features i = l (mod 256), a pass leaves the visual edges' 21 + 6 + 1 sums at the estimate in LDS, each
// lane adding its edges in ascending i, the 256 partials combined by stride halving.  The serial section follows: lane 0 evaluates the
// errors and Jacobians of EdgeInertial, the two random-walk edges and the prior edge; the products J^T Omega J, the assembly in vertex-id
// order (VP VV VG VA VPk VVk VGk VAk), the pivoted LDLT of 6i's departure (c) at lambda 0 (lm_ldlt_solve's operations in their order, on
// a matrix in LDS), and at the end the final Hessian, the marginalisation, the Jacobi sweeps and ConstraintPoseImu's clipping are spread
// over the workgroup's lanes: every output entry is computed by one lane in the serial form's own order, so no bit depends on the
// spreading.  Everything is double (the preintegration's bias correction float, as the reference has it), one rounding per operation
// (-ffp-contract=off); small products add left to right from their first term.  tests/pose_inertial_ref.py restates it operation by
// operation.
#include <float.h>
#include "rfe_internal.h"
#include "lm_device.h"

namespace rfe {
namespace {

constexpr int PIO_LANES = 256;
constexpr int PIO_MAX_N = 4096;
constexpr int PIO_TERMS = 28;
enum : uint8_t { PIO_EDGE = 1, PIO_OUTLIER = 2, PIO_STEREO = 4, PIO_CLOSE = 8 };
enum { PIO_FLAG_SOLVE_FAILED = 1, PIO_FLAG_NONFINITE = 2, PIO_FLAG_FEW_EDGES = 4, PIO_FLAG_RECOVERY = 8, PIO_FLAG_INFO_CLIPPED = 16,
       PIO_FLAG_MARG_CUT = 32, PIO_FLAG_PRIOR_CLIPPED = 64, PIO_FLAG_PRIOR_HUBER = 128, PIO_FLAG_MODE = 256 };

struct PioState { double Rwb[9], twb[3], v[3], bg[3], ba[3]; };

// the serial section's state, in LDS: lane 0 alone writes it between barriers
struct PioSerial {
    double sums[PIO_TERMS];
    PioState cur, prev, pri;
    double Rcw[9], tcw[3];                      // the current frame's camera pose, what the passes read
    double Rcb[9], tcb[3], Rbc[9], tbc[3];
    double info9[81], infoG[9], infoA[9], priH[225];
    double H[900], W[900], b[30], x[30];
    double J[216], e[15];
    double M1[225], M2[225];
    // the preintegration, float
    float dT, dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], pba[3], pbg[3];
    // what the cooperative steps hand from lane to lane
    double ep[15], Oe[15], g[24], ld[30], ly[30], cs[2], total, rho1;
    int lperm[30], piv;
    int lf, D, ok, flags, fails, iters, n_inl, n_bad;
};

// ---------------------------------------------------------------- small dense algebra, strides in elements: C = A B, sums left to right
__device__ void pio_mm(const double* A, int ars, int acs, const double* B, int brs, int bcs, double* C, int ldc, int m, int k, int n) {
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) {
            double acc = A[i * ars] * B[j * bcs];
            for (int t = 1; t < k; ++t) acc = acc + A[i * ars + t * acs] * B[t * brs + j * bcs];
            C[i * ldc + j] = acc;
        }
}
__device__ void pio_mm3(const double* A, const double* B, double* C) { pio_mm(A, 3, 1, B, 3, 1, C, 3, 3, 3, 3); }
__device__ void pio_mtm3(const double* A, const double* B, double* C) { pio_mm(A, 1, 3, B, 3, 1, C, 3, 3, 3, 3); }   // A^T B
__device__ void pio_mv3(const double* A, const double* x, double* y) { pio_mm(A, 3, 1, x, 1, 1, y, 1, 3, 3, 1); }
__device__ void pio_mtv3(const double* A, const double* x, double* y) { pio_mm(A, 1, 3, x, 1, 1, y, 1, 3, 3, 1); }    // A^T x
__device__ void pio_hat(const double* w, double* W) {
    W[0] = 0.0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0.0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0.0;
}

// cyclic Jacobi on the symmetric matrix whose lower triangle is A's (n x n, row-major): `sweeps` sweeps over (p, q), p < q, row by row; a
// pair whose entry is exactly 0 is skipped.  The eigenvalues are the final diagonal, the eigenvectors V's columns
__device__ void pio_jacobi(double* A, double* V, int n, int sweeps) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            if (j > i) A[i * n + j] = A[j * n + i];
            V[i * n + j] = (i == j) ? 1.0 : 0.0;
        }
    for (int sw = 0; sw < sweeps; ++sw)
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double a = A[k * n + p], bq = A[k * n + q];
                    A[k * n + p] = c * a - s * bq;
                    A[k * n + q] = s * a + c * bq;
                }
                for (int k = 0; k < n; ++k) {
                    const double a = A[p * n + k], bq = A[q * n + k];
                    A[p * n + k] = c * a - s * bq;
                    A[q * n + k] = s * a + c * bq;
                }
                for (int k = 0; k < n; ++k) {
                    const double a = V[k * n + p], bq = V[k * n + q];
                    V[k * n + p] = c * a - s * bq;
                    V[k * n + q] = s * a + c * bq;
                }
            }
}
// out = (V diag(d)) V^T; tmp: n * n
__device__ void pio_recompose(const double* V, const double* d, int n, double* tmp, double* out) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) tmp[i * n + j] = V[i * n + j] * d[j];
    pio_mm(tmp, n, 1, V, 1, n, out, n, n, n, n);
}

// the stated step in place of NormalizeRotation's SVD: R (R^T R)^(-1/2), the inverse root through pio_jacobi
__device__ void pio_nearest_rotation(const double* R, double* out) {
    double M[9], Q[9], d[3], tmp[9], S[9];
    pio_mtm3(R, R, M);
    pio_jacobi(M, Q, 3, 6);
    for (int i = 0; i < 3; ++i) d[i] = 1.0 / sqrt(M[i * 3 + i]);
    pio_recompose(Q, d, 3, tmp, S);
    pio_mm3(R, S, out);
}

// cofactor inverse of a 3 x 3
__device__ void pio_inv3(const double* a, double* out) {
    double c[9];
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[i * 3 + j] = a[i1 * 3 + j1] * a[i2 * 3 + j2] - a[i1 * 3 + j2] * a[i2 * 3 + j1];
        }
    }
    const double det = (a[0] * c[0] + a[1] * c[1]) + a[2] * c[2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = c[j * 3 + i] / det;
}

// inverse through an unpivoted LDLT of the symmetric matrix whose lower triangle is A's, column by column.  L: n * n, work: 3 n
__device__ void pio_ldlt_inverse(const double* A, int n, double* L, double* work, double* X) {
    double *d = work, *v = work + n, *y = work + 2 * n;
    for (int i = 0; i < n * n; ++i) L[i] = 0.0;
    for (int j = 0; j < n; ++j) {
        double acc = A[j * n + j];
        for (int k = 0; k < j; ++k) {
            v[k] = L[j * n + k] * d[k];
            acc = acc - L[j * n + k] * v[k];
        }
        d[j] = acc;
        for (int i = j + 1; i < n; ++i) {
            acc = A[i * n + j];
            for (int k = 0; k < j; ++k) acc = acc - L[i * n + k] * v[k];
            L[i * n + j] = acc / d[j];
        }
    }
    for (int c = 0; c < n; ++c) {
        for (int i = 0; i < n; ++i) {
            double acc = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) acc = acc - L[i * n + k] * y[k];
            y[i] = acc;
        }
        for (int i = 0; i < n; ++i) y[i] = y[i] / d[i];
        for (int i = n - 1; i >= 0; --i) {
            double acc = y[i];
            for (int k = i + 1; k < n; ++k) acc = acc - L[k * n + i] * y[k];
            y[i] = acc;
        }
        for (int i = 0; i < n; ++i) X[i * n + c] = y[i];
    }
}

// ---------------------------------------------------------------- SO3 (G2oTypes.cc:908-985)
__device__ void pio_exp_so3(const double* w, double* out) {
    const double d2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double d = sqrt(d2);
    double W[9], WW[9], res[9];
    pio_hat(w, W);
    if (d < 1e-5) {
        double hW[9];
        for (int i = 0; i < 9; ++i) hW[i] = 0.5 * W[i];
        pio_mm3(hW, W, WW);
        for (int i = 0; i < 9; ++i) res[i] = (((i % 4 == 0) ? 1.0 : 0.0) + W[i]) + WW[i];
    } else {
        double s, c;
        po_sincos(d, s, c);
        pio_mm3(W, W, WW);
        for (int i = 0; i < 9; ++i) res[i] = (((i % 4 == 0) ? 1.0 : 0.0) + (W[i] * s) / d) + (WW[i] * (1.0 - c)) / d2;
    }
    pio_nearest_rotation(res, out);
}
__device__ void pio_log_so3(const double* R, double* w) {
    const double tr = (R[0] + R[4]) + R[8];
    w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5;
    if (costheta > 1 || costheta < -1) return;
    const double theta = lm_acos(costheta);
    double s, c;
    po_sincos(theta, s, c);
    if (fabs(s) < 1e-5) return;
    for (int i = 0; i < 3; ++i) w[i] = (theta * w[i]) / s;
}
__device__ void pio_inv_right_jacobian(const double* v, double* out) {
    const double d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double d = sqrt(d2);
    if (d < 1e-5) {
        for (int i = 0; i < 9; ++i) out[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double W[9], WW[9], s, c;
    pio_hat(v, W);
    po_sincos(d, s, c);
    pio_mm3(W, W, WW);
    const double k = 1.0 / d2 - (1.0 + c) / ((2.0 * d) * s);
    for (int i = 0; i < 9; ++i) out[i] = (((i % 4 == 0) ? 1.0 : 0.0) + W[i] / 2) + WW[i] * k;
}
__device__ void pio_right_jacobian(const double* v, double* out) {
    const double d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double d = sqrt(d2);
    if (d < 1e-5) {
        for (int i = 0; i < 9; ++i) out[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double W[9], WW[9], s, c;
    pio_hat(v, W);
    po_sincos(d, s, c);
    pio_mm3(W, W, WW);
    for (int i = 0; i < 9; ++i) out[i] = (((i % 4 == 0) ? 1.0 : 0.0) - (W[i] * (1.0 - c)) / d2) + (WW[i] * (d - s)) / (d2 * d);
}

// ---------------------------------------------------------------- the preintegration (ImuTypes.cc:377-427), float
__device__ void pio_mv3f(const float* A, const float* x, float* y) {
    for (int r = 0; r < 3; ++r) y[r] = (A[r * 3] * x[0] + A[r * 3 + 1] * x[1]) + A[r * 3 + 2] * x[2];
}
// Sophus::SO3f::exp(om).matrix(): so3.hpp's expAndTheta with its small-angle branch, Eigen's toRotationMatrix.  sin and cos of the half
// angle are the float casts of po_sincos of its double cast
__device__ void pio_so3f_exp_matrix(const float* om, float* R) {
    const float theta_sq = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
    float imag, real;
    if (theta_sq < 1e-5f * 1e-5f) {
        const float po4 = theta_sq * theta_sq;
        imag = (0.5f - (float)(1.0 / 48.0) * theta_sq) + (float)(1.0 / 3840.0) * po4;
        real = (1.f - (float)(1.0 / 8.0) * theta_sq) + (float)(1.0 / 384.0) * po4;
    } else {
        const float theta = sqrtf(theta_sq);
        const float half = 0.5f * theta;
        double s, c;
        po_sincos((double)half, s, c);
        imag = (float)s / theta;
        real = (float)c;
    }
    const float qw = real, qx = imag * om[0], qy = imag * om[1], qz = imag * om[2];
    const float tx = 2.f * qx, ty = 2.f * qy, tz = 2.f * qz;
    const float twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0] = 1.f - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.f - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.f - (txx + tyy);
}

// EdgeInertial::computeError and linearizeOplus: S.e [9] and S.J [9, 24] over VPk 6, VVk 3, VGk 3, VAk 3, VP 6, VV 3
__device__ void pio_inertial_edge(PioSerial& S, bool linearise) {
    const double dt = (double)S.dT;
    const double g[3] = {0.0, 0.0, -(double)9.81f};
    float dbg[3], dba[3];
    for (int i = 0; i < 3; ++i) { dbg[i] = (float)S.prev.bg[i] - S.pbg[i]; dba[i] = (float)S.prev.ba[i] - S.pba[i]; }
    float om[3], Ef[9], Rf[9], t1[3], t2[3];
    pio_mv3f(S.JRg, dbg, om);
    pio_so3f_exp_matrix(om, Ef);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rf[r * 3 + c] = (S.dR[r * 3] * Ef[c] + S.dR[r * 3 + 1] * Ef[3 + c]) + S.dR[r * 3 + 2] * Ef[6 + c];
    double Rd[9], dR[9], dV[3], dP[3];
    for (int i = 0; i < 9; ++i) Rd[i] = (double)Rf[i];
    pio_nearest_rotation(Rd, dR);
    for (int i = 0; i < 9; ++i) dR[i] = (double)(float)dR[i];
    pio_mv3f(S.JVg, dbg, t1); pio_mv3f(S.JVa, dba, t2);
    for (int i = 0; i < 3; ++i) dV[i] = (double)((S.dV[i] + t1[i]) + t2[i]);
    pio_mv3f(S.JPg, dbg, t1); pio_mv3f(S.JPa, dba, t2);
    for (int i = 0; i < 3; ++i) dP[i] = (double)((S.dP[i] + t1[i]) + t2[i]);
    const double *Rwb1 = S.prev.Rwb, *Rwb2 = S.cur.Rwb;
    double A[9], eR[9], er[3], dv[3], dp[3], t[3];
    pio_mm(dR, 1, 3, Rwb1, 1, 3, A, 3, 3, 3, 3);          // dR^T Rwb1^T
    pio_mm3(A, Rwb2, eR);
    pio_log_so3(eR, er);
    for (int i = 0; i < 3; ++i) {
        dv[i] = (S.cur.v[i] - S.prev.v[i]) - g[i] * dt;
        dp[i] = ((S.cur.twb[i] - S.prev.twb[i]) - S.prev.v[i] * dt) - ((g[i] * dt) * dt) / 2;
    }
    pio_mtv3(Rwb1, dv, t);
    for (int i = 0; i < 3; ++i) { S.e[i] = er[i]; S.e[3 + i] = t[i] - dV[i]; }
    pio_mtv3(Rwb1, dp, t);
    for (int i = 0; i < 3; ++i) S.e[6 + i] = t[i] - dP[i];
    if (!linearise) return;
    double* J = S.J;
    for (int i = 0; i < 216; ++i) J[i] = 0.0;
    double invJr[9], nJr[9], B3[9], C3[9], hv[9];
    pio_inv_right_jacobian(er, invJr);
    for (int i = 0; i < 9; ++i) nJr[i] = -invJr[i];
    pio_mm(nJr, 3, 1, Rwb2, 1, 3, B3, 3, 3, 3, 3);        // -invJr Rwb2^T
    pio_mm3(B3, Rwb1, C3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) J[r * 24 + c] = C3[r * 3 + c];
    pio_mtv3(Rwb1, dv, t); pio_hat(t, hv);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) J[(3 + r) * 24 + c] = hv[r * 3 + c];
    for (int i = 0; i < 3; ++i) dp[i] = ((S.cur.twb[i] - S.prev.twb[i]) - S.prev.v[i] * dt) - ((0.5 * g[i]) * dt) * dt;
    pio_mtv3(Rwb1, dp, t); pio_hat(t, hv);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            J[(6 + r) * 24 + c] = hv[r * 3 + c];
            J[(6 + r) * 24 + 3 + c] = -((r == c) ? 1.0 : 0.0);
            J[(3 + r) * 24 + 6 + c] = -Rwb1[c * 3 + r];
            J[(6 + r) * 24 + 6 + c] = -Rwb1[c * 3 + r] * dt;
            J[(3 + r) * 24 + 9 + c] = -(double)S.JVg[r * 3 + c];
            J[(6 + r) * 24 + 9 + c] = -(double)S.JPg[r * 3 + c];
            J[(3 + r) * 24 + 12 + c] = -(double)S.JVa[r * 3 + c];
            J[(6 + r) * 24 + 12 + c] = -(double)S.JPa[r * 3 + c];
            J[r * 24 + 15 + c] = invJr[r * 3 + c];
            J[(3 + r) * 24 + 21 + c] = Rwb1[c * 3 + r];
        }
    double JRg[9], dbgd[3], jr[9];
    for (int i = 0; i < 9; ++i) JRg[i] = (double)S.JRg[i];
    for (int i = 0; i < 3; ++i) dbgd[i] = (double)dbg[i];
    pio_mv3(JRg, dbgd, t);
    pio_right_jacobian(t, jr);
    pio_mm(nJr, 3, 1, eR, 1, 3, B3, 3, 3, 3, 3);          // -invJr eR^T
    pio_mm3(B3, jr, C3);
    pio_mm3(C3, JRg, B3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) J[r * 24 + 9 + c] = B3[r * 3 + c];
    pio_mtm3(Rwb1, Rwb2, B3);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) J[(6 + r) * 24 + 18 + c] = B3[r * 3 + c];
}

// EdgePriorPoseImu: S.e [15], J [15, 15] (in Jp) over VPk 6, VVk 3, VGk 3, VAk 3
__device__ void pio_prior_edge(PioSerial& S, double* Jp, double* e, bool linearise) {
    double RtR[9], er[3], d[3], t[3];
    pio_mtm3(S.pri.Rwb, S.prev.Rwb, RtR);
    pio_log_so3(RtR, er);
    for (int i = 0; i < 3; ++i) d[i] = S.prev.twb[i] - S.pri.twb[i];
    pio_mtv3(S.pri.Rwb, d, t);
    for (int i = 0; i < 3; ++i) {
        e[i] = er[i]; e[3 + i] = t[i]; e[6 + i] = S.prev.v[i] - S.pri.v[i]; e[9 + i] = S.prev.bg[i] - S.pri.bg[i];
        e[12 + i] = S.prev.ba[i] - S.pri.ba[i];
    }
    if (!linearise) return;
    double ij[9];
    pio_inv_right_jacobian(er, ij);
    for (int i = 0; i < 225; ++i) Jp[i] = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { Jp[r * 15 + c] = ij[r * 3 + c]; Jp[(3 + r) * 15 + 3 + c] = RtR[r * 3 + c]; }
    for (int i = 6; i < 15; ++i) Jp[i * 15 + i] = 1.0;
}

// e . (Om e), R rows; Oe receives Om e
__device__ double pio_chi2(const double* Om, const double* e, int R, double* Oe) {
    pio_mm(Om, R, 1, e, 1, 1, Oe, 1, R, R, 1);
    double acc = e[0] * Oe[0];
    for (int r = 1; r < R; ++r) acc = acc + e[r] * Oe[r];
    return acc;
}
// ImuCamPose::Update: the NormalizeRotation(Rwb) of G2oTypes.cc:236 discards its result, so nothing is re-normalised
__device__ void pio_pose_update(PioState& st, const double* u) {
    double t[3], E[9], R[9];
    pio_mv3(st.Rwb, u + 3, t);
    for (int i = 0; i < 3; ++i) st.twb[i] = st.twb[i] + t[i];
    pio_exp_so3(u, E);
    pio_mm3(st.Rwb, E, R);
    for (int i = 0; i < 9; ++i) st.Rwb[i] = R[i];
}
__device__ void pio_camera_update(PioSerial& S) {
    double nRbw[9], tbw[3], t[3];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) nRbw[r * 3 + c] = -S.cur.Rwb[c * 3 + r];
    pio_mv3(nRbw, S.cur.twb, tbw);
    pio_mm(S.Rcb, 3, 1, S.cur.Rwb, 1, 3, S.Rcw, 3, 3, 3, 3);      // Rcb Rwb^T
    pio_mv3(S.Rcb, tbw, t);
    for (int i = 0; i < 3; ++i) S.tcw[i] = t[i] + S.tcb[i];
}

__device__ int pio_imap(int c) { return c < 15 ? c + 15 : c - 15; }   // inertial column -> solver index

__device__ void pio_sums_to_block(const double* sums, double* Hv) {
    int col = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k) { Hv[j * 6 + k] = sums[col]; Hv[k * 6 + j] = sums[col]; ++col; }
}

// ---------------------------------------------------------------- the cooperative forms: every lane of the workgroup calls them
// Each output entry is computed by ONE lane with the operations and the order of the serial form (pio_mm, pio_jacobi, pio_ldlt_solve), so
// which lane computes it changes no bit; __syncthreads separates the steps.  Operands and results live in LDS.
__device__ void pio_mm_par(const double* A, int ars, int acs, const double* B, int brs, int bcs, double* C, int ldc, int m, int k, int n, int lane) {
    for (int idx = lane; idx < m * n; idx += PIO_LANES) {
        const int i = idx / n, j = idx - i * n;
        double acc = A[i * ars] * B[j * bcs];
        for (int t = 1; t < k; ++t) acc = acc + A[i * ars + t * acs] * B[t * brs + j * bcs];
        C[i * ldc + j] = acc;
    }
}
// pio_jacobi: lane 0 computes the rotation of a pair, lanes 0 .. n-1 apply it to the columns of A, lanes 64 .. 64+n-1 to V, then lanes
// 0 .. n-1 to the rows of A.  cs: two doubles in LDS
__device__ void pio_jacobi_par(double* A, double* V, int n, int sweeps, double* cs, int lane) {
    for (int idx = lane; idx < n * n; idx += PIO_LANES) {
        const int i = idx / n, j = idx - i * n;
        if (j > i) A[i * n + j] = A[j * n + i];
        V[i * n + j] = (i == j) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sw = 0; sw < sweeps; ++sw)
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;                    // every lane reads the same entry
                if (lane == 0) {
                    const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0) t = -t;
                    const double c = 1.0 / sqrt(t * t + 1.0);
                    cs[0] = c; cs[1] = t * c;
                }
                __syncthreads();
                const double c = cs[0], s = cs[1];
                if (lane < n) {
                    const int k = lane;
                    const double a = A[k * n + p], bq = A[k * n + q];
                    A[k * n + p] = c * a - s * bq;
                    A[k * n + q] = s * a + c * bq;
                } else if (lane >= 64 && lane < 64 + n) {
                    const int k = lane - 64;
                    const double a = V[k * n + p], bq = V[k * n + q];
                    V[k * n + p] = c * a - s * bq;
                    V[k * n + q] = s * a + c * bq;
                }
                __syncthreads();
                if (lane < n) {
                    const int k = lane;
                    const double a = A[p * n + k], bq = A[q * n + k];
                    A[p * n + k] = c * a - s * bq;
                    A[q * n + k] = s * a + c * bq;
                }
                __syncthreads();
            }
}
// out = (V diag(d)) V^T; d: n doubles in LDS
__device__ void pio_recompose_par(const double* V, const double* d, int n, double* tmp, double* out, int lane) {
    for (int idx = lane; idx < n * n; idx += PIO_LANES) tmp[idx] = V[idx] * d[idx % n];
    __syncthreads();
    pio_mm_par(tmp, n, 1, V, 1, n, out, n, n, n, n, lane);
    __syncthreads();
}
// pio_ldlt_solve on S.b -> S.x: lane 0 finds the pivot, the swaps, the scaling of the column and the update of the trailing block are
// spread over the lanes, lane 0 runs the two triangular solves.  Every lane returns the same answer
__device__ bool pio_ldlt_solve_par(PioSerial& S, double* A, int D, int lane) {
    if (lane < D) { S.lperm[lane] = lane; S.ly[lane] = S.b[lane]; }
    __syncthreads();
    for (int k = 0; k < D; ++k) {
        if (lane == 0) {
            int p = k; double best = fabs(A[k * D + k]);
            for (int j = k + 1; j < D; ++j) {
                const double a = fabs(A[j * D + j]);
                if (a > best) { p = j; best = a; }
            }
            S.piv = p;
        }
        __syncthreads();
        const int p = S.piv;
        if (p != k) {
            if (lane < D) { const double t = A[k * D + lane]; A[k * D + lane] = A[p * D + lane]; A[p * D + lane] = t; }
            __syncthreads();
            if (lane < D) { const double t = A[lane * D + k]; A[lane * D + k] = A[lane * D + p]; A[lane * D + p] = t; }
            if (lane == 64) {
                const int t = S.lperm[k]; S.lperm[k] = S.lperm[p]; S.lperm[p] = t;
                const double u = S.ly[k]; S.ly[k] = S.ly[p]; S.ly[p] = u;
            }
            __syncthreads();
        }
        const double dk = A[k * D + k];
        if (lane == 0) S.ld[k] = dk;
        if (dk < 0.0) return false;                          // every lane reads the same pivot
        for (int i = k + 1 + lane; i < D; i += PIO_LANES) A[i * D + k] = (dk != 0.0) ? A[i * D + k] / dk : 0.0;
        __syncthreads();
        const int m = D - k - 1;
        for (int idx = lane; idx < m * m; idx += PIO_LANES) {
            const int ii = idx / m, jj = idx - ii * m;
            if (jj > ii) continue;
            const int i = k + 1 + ii, j = k + 1 + jj;
            const double v = A[i * D + j] - A[i * D + k] * A[k * D + j];
            A[i * D + j] = v; A[j * D + i] = v;
        }
        __syncthreads();
    }
    if (lane == 0) {
        double* y = S.ly;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < i; ++j) y[i] = y[i] - A[i * D + j] * y[j];
        for (int i = 0; i < D; ++i) y[i] = (S.ld[i] != 0.0) ? y[i] / S.ld[i] : 0.0;
        for (int i = D - 1; i >= 0; --i)
            for (int j = i + 1; j < D; ++j) y[i] = y[i] - A[j * D + i] * y[j];
        for (int i = 0; i < D; ++i) S.x[S.lperm[i]] = y[i];
    }
    __syncthreads();
    return true;
}

// one Gauss-Newton iteration behind a pass (optimization_algorithm_gauss_newton.cpp:50-93): S.sums were taken at the estimate.  Every lane
// calls it.  Lane 0 evaluates the errors and Jacobians of the four other edges, the lanes share the products J^T Omega J, the assembly and
// the factorisation, lane 0 applies the update
__device__ void pio_iteration(PioSerial& S, double* trace, int it, int lane) {
    double* H = S.H;
    double* W = S.W;
    __syncthreads();                                           // S.sums are lane 0's
    for (int i = lane; i < 900; i += PIO_LANES) H[i] = 0.0;
    if (lane >= 64 && lane < 94) S.b[lane - 64] = 0.0;
    if (lane == 0) {
        double total = S.sums[27];
        pio_inertial_edge(S, true);
        total = total + pio_chi2(S.info9, S.e, 9, S.Oe);
        S.total = total;
    }
    __syncthreads();
    // EdgeInertial: W = [wOm 81 | JtO 216 | Hi 576]
    for (int i = lane; i < 81; i += PIO_LANES) W[i] = 1.0 * S.info9[i];
    if (lane >= 128 && lane < 149) {                           // the visual block: entry col of the upper triangle, row by row
        const int col = lane - 128;
        int j = 0, rem = col;
        while (rem >= 6 - j) { rem -= 6 - j; ++j; }
        const int k = j + rem;
        H[j * 30 + k] = S.sums[col]; H[k * 30 + j] = S.sums[col];
    }
    if (lane >= 192 && lane < 198) S.b[lane - 192] = -S.sums[21 + lane - 192];
    if (lane >= 200 && lane < 209) S.ep[lane - 200] = 1.0 * S.Oe[lane - 200];      // w (Om e), w = 1
    __syncthreads();
    pio_mm_par(S.J, 1, 24, W, 9, 1, W + 81, 9, 24, 9, 9, lane);
    if (lane >= 232) pio_mm_par(S.J, 1, 24, S.ep, 1, 1, S.g, 1, 24, 9, 1, lane - 232);
    __syncthreads();
    pio_mm_par(W + 81, 9, 1, S.J, 24, 1, W + 297, 24, 24, 9, 24, lane);
    __syncthreads();
    for (int idx = lane; idx < 576; idx += PIO_LANES) {
        const int a = idx / 24, c = idx - a * 24;
        const int ia = pio_imap(a), ic = pio_imap(c);
        H[ia * 30 + ic] = H[ia * 30 + ic] + W[297 + idx];
    }
    if (lane < 24) { const int ia = pio_imap(lane); S.b[ia] = S.b[ia] - S.g[lane]; }
    __syncthreads();
    if (lane == 0) {
        double total = S.total;
        double Oe[3];
        // EdgeGyroRW, EdgeAccRW
        for (int which = 0; which < 2; ++which) {
            const double* Om = which ? S.infoA : S.infoG;
            const double *xc = which ? S.cur.ba : S.cur.bg, *xp = which ? S.prev.ba : S.prev.bg;
            const int off = which ? 12 : 9, offk = which ? 27 : 24;
            double erw[3];
            for (int i = 0; i < 3; ++i) erw[i] = xc[i] - xp[i];
            total = total + pio_chi2(Om, erw, 3, Oe);
            for (int a = 0; a < 3; ++a) {
                S.b[off + a] = S.b[off + a] - Oe[a];
                S.b[offk + a] = S.b[offk + a] + Oe[a];
                for (int c = 0; c < 3; ++c) {
                    const double o = Om[a * 3 + c];
                    H[(off + a) * 30 + off + c] = H[(off + a) * 30 + off + c] + o;
                    H[(offk + a) * 30 + offk + c] = H[(offk + a) * 30 + offk + c] + o;
                    H[(off + a) * 30 + offk + c] = H[(off + a) * 30 + offk + c] - o;
                    H[(offk + a) * 30 + off + c] = H[(offk + a) * 30 + off + c] - o;
                }
            }
        }
        if (S.lf) {                                            // EdgePriorPoseImu under Huber 5: its error and Jacobian (Jp in M1)
            pio_prior_edge(S, S.M1, S.ep, true);
            const double chi2 = pio_chi2(S.priH, S.ep, 15, S.Oe);
            double rho0 = chi2, rho1 = 1.0;
            const double delta = 5.0, dsqr = delta * delta;
            if (!(chi2 <= dsqr)) {
                const double sq = sqrt(chi2);
                rho0 = 2 * sq * delta - dsqr;
                rho1 = delta / sq;
            }
            if (rho1 != 1.0) S.flags |= PIO_FLAG_PRIOR_HUBER;
            S.rho1 = rho1;
            total = total + rho0;
        }
        if (trace) {
            if (it == 0) trace[1] = total;
            trace[0] = (double)(it + 1); trace[2] = total;
        }
    }
    __syncthreads();
    if (S.lf) {                                                // W = [wOm 225 | JtO 225 | Hp 225]
        const double rho1 = S.rho1;
        for (int i = lane; i < 225; i += PIO_LANES) W[i] = rho1 * S.priH[i];
        if (lane >= 232 && lane < 247) S.ld[lane - 232] = rho1 * S.Oe[lane - 232];
        __syncthreads();
        pio_mm_par(S.M1, 1, 15, W, 15, 1, W + 225, 15, 15, 15, 15, lane);
        if (lane >= 232) pio_mm_par(S.M1, 1, 15, S.ld, 1, 1, S.g, 1, 15, 15, 1, lane - 232);
        __syncthreads();
        pio_mm_par(W + 225, 15, 1, S.M1, 15, 1, W + 450, 15, 15, 15, 15, lane);
        __syncthreads();
        for (int idx = lane; idx < 225; idx += PIO_LANES) {
            const int a = idx / 15, c = idx - a * 15;
            H[(15 + a) * 30 + 15 + c] = H[(15 + a) * 30 + 15 + c] + W[450 + idx];
        }
        if (lane >= 232 && lane < 247) S.b[15 + lane - 232] = S.b[15 + lane - 232] - S.g[lane - 232];
        __syncthreads();
    }
    const int D = S.D;
    for (int idx = lane; idx < D * D; idx += PIO_LANES) { const int i = idx / D, j = idx - i * D; W[idx] = H[i * 30 + j]; }
    __syncthreads();
    const bool ok = pio_ldlt_solve_par(S, W, D, lane);
    __syncthreads();
    if (lane == 0) {
        S.ok = ok ? 1 : 0;
        if (!ok) { S.flags |= PIO_FLAG_SOLVE_FAILED; ++S.fails; }
        pio_pose_update(S.cur, S.x);
        pio_camera_update(S);
        for (int i = 0; i < 3; ++i) {
            S.cur.v[i] = S.cur.v[i] + S.x[6 + i]; S.cur.bg[i] = S.cur.bg[i] + S.x[9 + i]; S.cur.ba[i] = S.cur.ba[i] + S.x[12 + i];
        }
        ++S.iters;
    } else if (lane == 64 && S.lf) {
        pio_pose_update(S.prev, S.x + 15);
        for (int i = 0; i < 3; ++i) {
            S.prev.v[i] = S.prev.v[i] + S.x[21 + i]; S.prev.bg[i] = S.prev.bg[i] + S.x[24 + i]; S.prev.ba[i] = S.prev.ba[i] + S.x[27 + i];
        }
    }
}

// what the constructors leave: the states, EdgeInertial's information (the inverse of C's 9 x 9 block, symmetrised, eigenvalues below
// 1e-12 set to 0), InfoG, InfoA, the prior
__device__ void pio_setup(PioSerial& S, const float* cam, const float* state, const float* prev_state, const float* pre, const float* cov_rw,
                          const double* prior_in) {
    for (int i = 0; i < 9; ++i) {
        S.Rcw[i] = (double)cam[i]; S.Rcb[i] = (double)cam[12 + i];
        S.cur.Rwb[i] = (double)state[i]; S.prev.Rwb[i] = (double)prev_state[i];
    }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S.Rbc[r * 3 + c] = S.Rcb[c * 3 + r];
    for (int i = 0; i < 3; ++i) {
        S.tcw[i] = (double)cam[9 + i]; S.tcb[i] = (double)cam[21 + i]; S.tbc[i] = (double)cam[33 + i];
        S.cur.twb[i] = (double)state[9 + i]; S.cur.v[i] = (double)state[12 + i]; S.cur.bg[i] = (double)state[15 + i]; S.cur.ba[i] = (double)state[18 + i];
        S.prev.twb[i] = (double)prev_state[9 + i]; S.prev.v[i] = (double)prev_state[12 + i]; S.prev.bg[i] = (double)prev_state[15 + i];
        S.prev.ba[i] = (double)prev_state[18 + i];
        S.dV[i] = pre[10 + i]; S.dP[i] = pre[13 + i]; S.pba[i] = pre[61 + i]; S.pbg[i] = pre[64 + i];
    }
    S.dT = pre[0];
    for (int i = 0; i < 9; ++i) {
        S.dR[i] = pre[1 + i]; S.JRg[i] = pre[16 + i]; S.JVg[i] = pre[25 + i]; S.JVa[i] = pre[34 + i]; S.JPg[i] = pre[43 + i]; S.JPa[i] = pre[52 + i];
    }
    // W = [C 81 | L 81 | work 27 | X 81 | V 81 | tmp 81]: the inverse of C's block, symmetrised, is left in W for pio_setup_information
    double *Cm = S.W, *L = S.W + 81, *work = S.W + 162, *X = S.W + 189;
    for (int i = 0; i < 81; ++i) Cm[i] = (double)pre[67 + i];
    pio_ldlt_inverse(Cm, 9, L, work, X);
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) Cm[i * 9 + j] = (X[i * 9 + j] + X[j * 9 + i]) / 2;
    double c3[9];
    for (int i = 0; i < 9; ++i) c3[i] = (double)cov_rw[i];
    pio_inv3(c3, S.infoG);
    for (int i = 0; i < 9; ++i) c3[i] = (double)cov_rw[9 + i];
    pio_inv3(c3, S.infoA);
    if (S.lf) {
        for (int i = 0; i < 9; ++i) S.pri.Rwb[i] = prior_in[i];
        for (int i = 0; i < 3; ++i) { S.pri.twb[i] = prior_in[9 + i]; S.pri.v[i] = prior_in[12 + i]; S.pri.bg[i] = prior_in[15 + i]; S.pri.ba[i] = prior_in[18 + i]; }
        for (int i = 0; i < 225; ++i) S.priH[i] = prior_in[21 + i];
    }
}

// EdgeInertial's information from what pio_setup left in W: eigenvalues below 1e-12 set to 0, recomposed.  Every lane calls it
__device__ void pio_setup_information(PioSerial& S, int lane) {
    double *Cm = S.W, *V = S.W + 270, *tmp = S.W + 351;
    pio_jacobi_par(Cm, V, 9, 10, S.cs, lane);
    if (lane == 0)
        for (int i = 0; i < 9; ++i) {
            const double l = Cm[i * 9 + i];
            const bool cl = l < 1e-12;
            if (cl) S.flags |= PIO_FLAG_INFO_CLIPPED;
            S.ld[i] = cl ? 0.0 : l;
        }
    __syncthreads();
    pio_recompose_par(V, S.ld, 9, tmp, S.info9, lane);
}

// the final Hessian at the final estimate (S.sums: the inliers' visual block), Marginalize(H, 0, 14) in LastFrame mode, ConstraintPoseImu's
// clipping; leaves the 15 x 15 result in S.M2
__device__ void pio_final(PioSerial& S, int lane) {
    double* W = S.W;
    double* Hf = S.M2;
    __syncthreads();                                           // S.sums are lane 0's
    if (lane == 0) pio_inertial_edge(S, true);
    if (lane == 64 && S.lf) pio_prior_edge(S, S.M1, S.ep, true);       // Jp in M1
    for (int i = lane; i < 900; i += PIO_LANES) S.H[i] = 0.0;
    for (int i = lane; i < 225; i += PIO_LANES) Hf[i] = 0.0;
    __syncthreads();
    // Hi = (J^T info9) J: W = [JtO 216 | Hi 576]
    pio_mm_par(S.J, 1, 24, S.info9, 9, 1, W, 9, 24, 9, 9, lane);
    __syncthreads();
    pio_mm_par(W, 9, 1, S.J, 24, 1, W + 216, 24, 24, 9, 24, lane);
    __syncthreads();
    if (S.lf) {
        double* H = S.H;
        for (int idx = lane; idx < 576; idx += PIO_LANES) { const int a = idx / 24, c = idx - a * 24; H[a * 30 + c] = H[a * 30 + c] + W[216 + idx]; }
        __syncthreads();
        if (lane == 0)
            for (int which = 0; which < 2; ++which) {
                const double* Om = which ? S.infoA : S.infoG;
                const int o1 = which ? 12 : 9, o2 = which ? 27 : 24;
                for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) H[(o1 + a) * 30 + o1 + c] = H[(o1 + a) * 30 + o1 + c] + Om[a * 3 + c];
                for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) H[(o1 + a) * 30 + o2 + c] = H[(o1 + a) * 30 + o2 + c] - Om[a * 3 + c];
                for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) H[(o2 + a) * 30 + o1 + c] = H[(o2 + a) * 30 + o1 + c] - Om[a * 3 + c];
                for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) H[(o2 + a) * 30 + o2 + c] = H[(o2 + a) * 30 + o2 + c] + Om[a * 3 + c];
            }
        // the prior's GetHessian: W = [JtO 225 | Hp 225]
        pio_mm_par(S.M1, 1, 15, S.priH, 15, 1, W, 15, 15, 15, 15, lane);
        __syncthreads();
        pio_mm_par(W, 15, 1, S.M1, 15, 1, W + 225, 15, 15, 15, 15, lane);
        __syncthreads();
        for (int idx = lane; idx < 225; idx += PIO_LANES) { const int a = idx / 15, c = idx - a * 15; H[a * 30 + c] = H[a * 30 + c] + W[225 + idx]; }
        __syncthreads();
        if (lane < 36) {
            const int a = lane / 6, c = lane - a * 6;
            int lo = a < c ? a : c, hi = a < c ? c : a, col = hi - lo;
            for (int jj = 0; jj < lo; ++jj) col += 6 - jj;
            H[(15 + a) * 30 + 15 + c] = H[(15 + a) * 30 + 15 + c] + S.sums[col];
        }
        __syncthreads();
        // Marginalize(H, 0, 14): W = [A 225 | Q 225 | tmp 225 | inv_b 225], T = M1
        double *A = W, *Q = W + 225, *tmp = W + 450, *invb = W + 675, *T = S.M1;
        for (int idx = lane; idx < 225; idx += PIO_LANES) { const int i = idx / 15, j = idx - i * 15; A[idx] = H[i * 30 + j]; }
        __syncthreads();
        pio_jacobi_par(A, Q, 15, 12, S.cs, lane);
        if (lane == 0)
            for (int i = 0; i < 15; ++i) {
                const double l = A[i * 15 + i];
                const bool keep = fabs(l) > 1e-6;
                if (!keep) S.flags |= PIO_FLAG_MARG_CUT;
                S.ld[i] = keep ? 1.0 / l : 0.0;
            }
        __syncthreads();
        pio_recompose_par(Q, S.ld, 15, tmp, invb, lane);
        pio_mm_par(H + 15 * 30, 30, 1, invb, 15, 1, T, 15, 15, 15, 15, lane);                 // H[15:30, 0:15] inv_b
        __syncthreads();
        pio_mm_par(T, 15, 1, H + 15, 30, 1, tmp, 15, 15, 15, 15, lane);                       // ... H[0:15, 15:30]
        __syncthreads();
        for (int idx = lane; idx < 225; idx += PIO_LANES) { const int i = idx / 15, j = idx - i * 15; Hf[idx] = H[(15 + i) * 30 + 15 + j] - tmp[idx]; }
        __syncthreads();
    } else {
        if (lane < 81) { const int a = lane / 9, c = lane - a * 9; Hf[a * 15 + c] = Hf[a * 15 + c] + W[216 + (15 + a) * 24 + 15 + c]; }
        if (lane >= 96 && lane < 105) {
            const int a = (lane - 96) / 3, c = (lane - 96) - a * 3;
            Hf[(9 + a) * 15 + 9 + c] = Hf[(9 + a) * 15 + 9 + c] + S.infoG[a * 3 + c];
            Hf[(12 + a) * 15 + 12 + c] = Hf[(12 + a) * 15 + 12 + c] + S.infoA[a * 3 + c];
        }
        __syncthreads();
        if (lane < 36) {
            const int a = lane / 6, c = lane - a * 6;
            int lo = a < c ? a : c, hi = a < c ? c : a, col = hi - lo;
            for (int jj = 0; jj < lo; ++jj) col += 6 - jj;
            Hf[a * 15 + c] = Hf[a * 15 + c] + S.sums[col];
        }
        __syncthreads();
    }
    // ConstraintPoseImu's constructor: (H + H) / 2 changes nothing; the eigen-solver reads the lower triangle.  W = [A | V | tmp]
    double *A = W, *V = W + 225, *tmp = W + 450;
    for (int i = lane; i < 225; i += PIO_LANES) A[i] = Hf[i];
    __syncthreads();
    pio_jacobi_par(A, V, 15, 12, S.cs, lane);
    if (lane == 0)
        for (int i = 0; i < 15; ++i) {
            const double l = A[i * 15 + i];
            const bool cl = l < 1e-12;
            if (cl) S.flags |= PIO_FLAG_PRIOR_CLIPPED;
            S.ld[i] = cl ? 0.0 : l;
        }
    __syncthreads();
    pio_recompose_par(V, S.ld, 15, tmp, Hf, lane);
}

// ---------------------------------------------------------------- the visual edges
struct PioCam { double fx, fy, cx, cy, bf; };
struct PioEdge { double X0, X1, X2, u, v, ur, isg; bool stereo; };
struct PioView { double Rcw[9], tcw[3], Rcb[9], Rbc[9], tbc[3]; };

__device__ PioEdge pio_load(const PioArgs& p, const rfe_pose_inertial_params& P, int i) {
    PioEdge e;
    e.X0 = (double)p.xw[3 * i]; e.X1 = (double)p.xw[3 * i + 1]; e.X2 = (double)p.xw[3 * i + 2];
    e.u = (double)p.kpts[2 * i]; e.v = (double)p.kpts[2 * i + 1];
    const float ur = p.uright ? p.uright[i] : -1.f;
    e.stereo = !(ur < 0);
    e.ur = (double)ur;
    int o = p.octave ? p.octave[i] : 0;
    if (o < 0 || o >= P.nlevels) o = 0;
    e.isg = (double)P.inv_level_sigma2[o];
    return e;
}

// computeError and chi2() at the view: the point in the camera frame in x y z, the error in e
__device__ double pio_error(const PioCam& C, const PioView& V, const PioEdge& E, double& x, double& y, double& z, double (&e)[3]) {
    x = ((V.Rcw[0] * E.X0 + V.Rcw[1] * E.X1) + V.Rcw[2] * E.X2) + V.tcw[0];
    y = ((V.Rcw[3] * E.X0 + V.Rcw[4] * E.X1) + V.Rcw[5] * E.X2) + V.tcw[1];
    z = ((V.Rcw[6] * E.X0 + V.Rcw[7] * E.X1) + V.Rcw[8] * E.X2) + V.tcw[2];
    const double pu = C.fx * x / z + C.cx;
    const double pv = C.fy * y / z + C.cy;
    e[0] = E.u - pu; e[1] = E.v - pv; e[2] = 0.0;
    double chi2 = e[0] * (E.isg * e[0]) + e[1] * (E.isg * e[1]);
    if (E.stereo) {
        const double pr = pu - C.bf * (1.0 / z);
        e[2] = E.ur - pr;
        chi2 = chi2 + e[2] * (E.isg * e[2]);
    }
    return chi2;
}

// one edge's 28 terms added to acc; returns chi2
__device__ double pio_edge_terms(const PioCam& C, const PioView& V, const PioEdge& E, bool robust, double (&acc)[PIO_TERMS]) {
    double x, y, z, e[3];
    const double chi2 = pio_error(C, V, E, x, y, z, e);
    double rho0 = chi2, rho1 = 1.0;
    if (robust) {
        const double delta = E.stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991);
        const double dsqr = (double)(float)(delta * delta);
        if (!(chi2 <= dsqr)) {
            const double sq = sqrt(chi2);
            rho0 = 2 * sq * delta - dsqr;
            rho1 = delta / sq;
        }
    }
    const double xb = ((V.Rbc[0] * x + V.Rbc[1] * y) + V.Rbc[2] * z) + V.tbc[0];
    const double yb = ((V.Rbc[3] * x + V.Rbc[4] * y) + V.Rbc[5] * z) + V.tbc[1];
    const double zb = ((V.Rbc[6] * x + V.Rbc[7] * y) + V.Rbc[8] * z) + V.tbc[2];
    const double zz = z * z;
    double pj[3][3] = {{C.fx / z, 0.0, -C.fx * x / zz}, {0.0, C.fy / z, -C.fy * y / zz}, {0.0, 0.0, 0.0}};
    const int rows = E.stereo ? 3 : 2;
    if (E.stereo) { pj[2][0] = pj[0][0]; pj[2][1] = pj[0][1]; pj[2][2] = pj[0][2] + C.bf * (1.0 / zz); }
    const double Sd[3][6] = {{0.0, zb, -yb, 1.0, 0.0, 0.0}, {-zb, 0.0, xb, 0.0, 1.0, 0.0}, {yb, -xb, 0.0, 0.0, 0.0, 1.0}};
    double A[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double PR[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) PR[c] = (pj[r][0] * V.Rcb[c] + pj[r][1] * V.Rcb[3 + c]) + pj[r][2] * V.Rcb[6 + c];
#pragma unroll
        for (int c = 0; c < 6; ++c) A[r][c] = (r < rows) ? (PR[0] * Sd[0][c] + PR[1] * Sd[1][c]) + PR[2] * Sd[2][c] : 0.0;
    }
    const double w = rho1 * E.isg;
    int col = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = j; k < 6; ++k) {
            double h = (A[0][j] * w) * A[0][k] + (A[1][j] * w) * A[1][k];
            if (E.stereo) h = h + (A[2][j] * w) * A[2][k];
            acc[col] = acc[col] + h;
            ++col;
        }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double g = ((rho1 * A[0][j]) * E.isg) * e[0] + ((rho1 * A[1][j]) * E.isg) * e[1];
        if (E.stereo) g = g + ((rho1 * A[2][j]) * E.isg) * e[2];
        acc[21 + j] = acc[21 + j] + g;
    }
    acc[27] = acc[27] + rho0;
    return chi2;
}

// the float classification of one edge behind round rnd (Optimizer.cc:729-810, :1313-1392): an edge flagged outlier recomputes its error
// at the view, any other keeps cf, the chi2 the last iteration saw.  Returns the new flag; cf leaves as the value compared
__device__ bool pio_classify(const PioCam& C, const PioView& V, const PioEdge& E, uint8_t st, bool lf, int rnd, float& cf) {
    const float tm = lf ? 5.991f : (rnd == 0 ? 12.f : (rnd == 1 ? 7.5f : 5.991f));
    const float ts = rnd == 0 ? 15.6f : (rnd == 1 ? 9.8f : 7.815f);
    const float tclose = (float)(1.5 * (double)tm);
    if (st & PIO_OUTLIER) {
        double x, y, z, e[3];
        cf = (float)pio_error(C, V, E, x, y, z, e);
    }
    if (st & PIO_STEREO) return cf > ts;
    const bool close = (st & PIO_CLOSE) != 0;
    const double zc = ((V.Rcw[6] * E.X0 + V.Rcw[7] * E.X1) + V.Rcw[8] * E.X2) + V.tcw[2];
    return (cf > tm && !close) || (close && cf > tclose) || !(zc > 0.0);
}
// the recovery pass's test of one edge (:836-857, :1417-1437): its error recomputed, below 18 / 24
__device__ bool pio_recovered(const PioCam& C, const PioView& V, const PioEdge& E, uint8_t st, float& cf) {
    double x, y, z, e[3];
    cf = (float)pio_error(C, V, E, x, y, z, e);
    return cf < ((st & PIO_STEREO) ? 24.f : 18.f);
}

__device__ void pio_read_view(const PioSerial& S, PioView& V) {
    for (int i = 0; i < 9; ++i) { V.Rcw[i] = S.Rcw[i]; V.Rcb[i] = S.Rcb[i]; V.Rbc[i] = S.Rbc[i]; }
    for (int i = 0; i < 3; ++i) { V.tcw[i] = S.tcw[i]; V.tbc[i] = S.tbc[i]; }
}

// the 28 partials of every lane -> S.sums, in two halves so that the reduction's LDS stays at 14 KiB
__device__ void pio_reduce(double (&acc)[PIO_TERMS], double* red, double* sums, int lane) {
    double a[14];
#pragma unroll
    for (int c = 0; c < 14; ++c) a[c] = acc[c];
    lm_reduce<14>(a, red, sums, lane);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 14; ++c) a[c] = acc[14 + c];
    lm_reduce<14>(a, red, sums + 14, lane);
}

__global__ __launch_bounds__(PIO_LANES) void pose_inertial_kernel(rfe_pose_inertial_params P, PioArgs pr0) {
    __shared__ double red[128 * 14];
    __shared__ float chi2f[PIO_MAX_N];              // (float) chi2 of the error the last computeActiveErrors left on the edge
    __shared__ uint8_t state[PIO_MAX_N];
    __shared__ PioSerial S;
    __shared__ int cnt, cnt_stereo;
    const int lane = threadIdx.x, prob = blockIdx.x;
    const int N = pr0.N;
    PioArgs p = pr0;
    p.kpts += (size_t)prob * N * 2; p.xw += (size_t)prob * N * 3; p.has_mp += (size_t)prob * N; p.track_depth += (size_t)prob * N;
    if (p.uright) p.uright += (size_t)prob * N;
    if (p.octave) p.octave += (size_t)prob * N;
    p.outlier += (size_t)prob * N; p.stats += (size_t)prob * 16; p.state_out += (size_t)prob * 21;
    if (p.state_f32) p.state_f32 += (size_t)prob * 21;
    if (p.chi2) p.chi2 += (size_t)prob * N;
    if (p.trace) p.trace += (size_t)prob * 32;
    if (p.prior_out) p.prior_out += (size_t)prob * 246;
    int n = p.n ? p.n[prob] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    const bool lf = p.mode[prob] == RFE_PIO_LAST_FRAME && p.prior_in != nullptr;
    const bool rec_init = p.rec_init ? p.rec_init[prob] != 0 : false;
    const PioCam C = {(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy, (double)P.bf};

    if (lane == 0) { cnt = 0; cnt_stereo = 0; }
    if (p.trace && lane < 32) p.trace[lane] = 0.0;
    __syncthreads();
    int mine = 0, mine_stereo = 0;
    for (int i = lane; i < n; i += PIO_LANES) {
        const bool has = p.has_mp[i] != 0;
        const float ur = p.uright ? p.uright[i] : -1.f;
        const bool st = !(ur < 0);
        state[i] = has ? (uint8_t)(PIO_EDGE | (st ? PIO_STEREO : 0) | (p.track_depth[i] < 10.f ? PIO_CLOSE : 0)) : 0;
        if (has) { p.outlier[i] = 0; ++mine; mine_stereo += st ? 1 : 0; }
    }
    if (mine) atomicAdd(&cnt, mine);
    if (mine_stereo) atomicAdd(&cnt_stereo, mine_stereo);
    if (lane == 0) {
        S.lf = lf ? 1 : 0; S.D = lf ? 30 : 15; S.flags = (p.mode[prob] == RFE_PIO_LAST_KEYFRAME || lf) ? 0 : PIO_FLAG_MODE; S.fails = 0; S.iters = 0; S.n_inl = 0; S.n_bad = 0; S.ok = 1;
        for (int i = 0; i < 30; ++i) S.x[i] = 0.0;
        pio_setup(S, p.cam + (size_t)prob * 36, p.state + (size_t)prob * 21, p.prev_state + (size_t)prob * 21, p.preint + (size_t)prob * 148,
                  p.cov_rw + (size_t)prob * 18, lf ? p.prior_in + (size_t)prob * 246 : nullptr);
    }
    __syncthreads();
    pio_setup_information(S, lane);
    const int n_init = cnt, n_stereo = cnt_stereo;
    const int n_edges = n_init + (lf ? 4 : 3);
    int rounds = 0;
    PioView V;
    for (int rnd = 0; rnd < 4; ++rnd) {
        const bool robust = rnd < 3;                 // setRobustKernel(0) runs behind round 2's classification
        double* tr = p.trace ? p.trace + rnd * 8 : nullptr;
        for (int it = 0; it < 10; ++it) {
            pio_read_view(S, V);
            double acc[PIO_TERMS];
#pragma unroll
            for (int c = 0; c < PIO_TERMS; ++c) acc[c] = 0.0;
            for (int i = lane; i < n; i += PIO_LANES) {
                if ((state[i] & (PIO_EDGE | PIO_OUTLIER)) != PIO_EDGE) continue;
                const PioEdge E = pio_load(p, P, i);
                chi2f[i] = (float)pio_edge_terms(C, V, E, robust, acc);
            }
            pio_reduce(acc, red, S.sums, lane);      // its barriers also order the reads of S above before lane 0's writes below
            pio_iteration(S, tr, it, lane);
            __syncthreads();
            if (!S.ok) break;                        // a failed solve: the update was applied, the round ends
        }
        // classification in float (Optimizer.cc:729-810, :1313-1392): an outlier edge recomputes its error at the new estimate, an inlier
        // keeps the one the last iteration saw
        if (lane == 0) { cnt = 0; if (tr) tr[3] = S.ok ? 1.0 : 0.0; }
        pio_read_view(S, V);
        __syncthreads();
        {
            int bad = 0;
            for (int i = lane; i < n; i += PIO_LANES) {
                const uint8_t st = state[i];
                if (!(st & PIO_EDGE)) continue;
                const PioEdge E = pio_load(p, P, i);
                float cf = chi2f[i];
                const bool out = pio_classify(C, V, E, st, lf, rnd, cf);
                chi2f[i] = cf;
                state[i] = out ? (uint8_t)(st | PIO_OUTLIER) : (uint8_t)(st & ~PIO_OUTLIER);
                p.outlier[i] = out ? 1 : 0;
                if (p.chi2) p.chi2[i] = cf;
                bad += out ? 1 : 0;
            }
            if (bad) atomicAdd(&cnt, bad);
        }
        __syncthreads();
        if (lane == 0) {
            S.n_bad = cnt; S.n_inl = n_init - cnt; S.ok = 1;
            if (tr) tr[4] = (double)S.n_inl;
        }
        ++rounds;
        __syncthreads();
        if (n_edges < 10) {
            if (lane == 0) S.flags |= PIO_FLAG_FEW_EDGES;
            break;
        }
    }
    // the recovery pass (Optimizer.cc:826-858, :1407-1438): every edge recomputes its error; below 18 / 24 the flag is cleared, otherwise it
    // stays as it is and the edge counts as bad
    const bool recover = S.n_inl < 30 && !rec_init;
    __syncthreads();
    if (recover) {
        if (lane == 0) { cnt = 0; S.flags |= PIO_FLAG_RECOVERY; }
        pio_read_view(S, V);
        __syncthreads();
        int bad = 0;
        for (int i = lane; i < n; i += PIO_LANES) {
            const uint8_t st = state[i];
            if (!(st & PIO_EDGE)) continue;
            const PioEdge E = pio_load(p, P, i);
            float cf;
            const bool good = pio_recovered(C, V, E, st, cf);
            if (good) { state[i] = (uint8_t)(st & ~PIO_OUTLIER); p.outlier[i] = 0; }
            else ++bad;
            if (p.chi2) p.chi2[i] = cf;
        }
        if (bad) atomicAdd(&cnt, bad);
        __syncthreads();
        if (lane == 0) S.n_bad = cnt;
    }
    // the final Hessian's visual block: inliers only, no robust weight
    {
        pio_read_view(S, V);
        double acc[PIO_TERMS];
#pragma unroll
        for (int c = 0; c < PIO_TERMS; ++c) acc[c] = 0.0;
        for (int i = lane; i < n; i += PIO_LANES) {
            if ((state[i] & (PIO_EDGE | PIO_OUTLIER)) != PIO_EDGE) continue;
            const PioEdge E = pio_load(p, P, i);
            pio_edge_terms(C, V, E, false, acc);
        }
        pio_reduce(acc, red, S.sums, lane);
    }
    pio_final(S, lane);
    if (lane == 0) {
        bool fin = true;
        double so[21];
        for (int i = 0; i < 9; ++i) so[i] = S.cur.Rwb[i];
        for (int i = 0; i < 3; ++i) { so[9 + i] = S.cur.twb[i]; so[12 + i] = S.cur.v[i]; so[15 + i] = S.cur.bg[i]; so[18 + i] = S.cur.ba[i]; }
        for (int i = 0; i < 21; ++i) {
            p.state_out[i] = so[i];
            if (p.state_f32) p.state_f32[i] = (float)so[i];
            if (p.prior_out) p.prior_out[i] = so[i];
            fin = fin && isfinite(so[i]);
        }
        for (int i = 0; i < 225; ++i) {
            if (p.prior_out) p.prior_out[21 + i] = S.M2[i];
            fin = fin && isfinite(S.M2[i]);
        }
        if (!fin) S.flags |= PIO_FLAG_NONFINITE;
        p.stats[0] = n_init - S.n_bad; p.stats[1] = n_init; p.stats[2] = S.n_bad; p.stats[3] = n_init - n_stereo; p.stats[4] = n_stereo;
        p.stats[5] = rounds; p.stats[6] = S.iters; p.stats[7] = S.fails; p.stats[8] = S.flags; p.stats[9] = S.n_inl;
        for (int i = 10; i < 16; ++i) p.stats[i] = 0;
    }
}

// test hook: the classification behind round rnd (0..3) or the recovery pass (rnd 4) of n edges at a given camera pose
__global__ __launch_bounds__(PIO_LANES) void pose_inertial_classify_kernel(rfe_pose_inertial_params P, PioArgs p, const double* view, int lf, int rnd,
                                                                           const uint8_t* outlier_in, const float* chi2_in, uint8_t* code) {
    const PioCam C = {(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy, (double)P.bf};
    PioView V = PioView();
    for (int i = 0; i < 9; ++i) V.Rcw[i] = view[i];
    for (int i = 0; i < 3; ++i) V.tcw[i] = view[9 + i];
    for (int i = threadIdx.x; i < p.N; i += PIO_LANES) {
        const float ur = p.uright ? p.uright[i] : -1.f;
        const uint8_t st = (uint8_t)(PIO_EDGE | (!(ur < 0) ? PIO_STEREO : 0) | (p.track_depth[i] < 10.f ? PIO_CLOSE : 0) | (outlier_in[i] ? PIO_OUTLIER : 0));
        const PioEdge E = pio_load(p, P, i);
        float cf = chi2_in[i];
        if (rnd < 4) {
            code[i] = pio_classify(C, V, E, st, lf != 0, rnd, cf) ? 1 : 0;
        } else {
            const bool good = pio_recovered(C, V, E, st, cf);
            code[i] = (uint8_t)((good ? 0 : (outlier_in[i] ? 1 : 0)) | (good ? 0 : 2));      // bit 0: the flag afterwards, bit 1: counted in nBad
        }
        p.chi2[i] = cf;
    }
}

}  // namespace

void launch_pose_inertial_classify(hipStream_t s, const rfe_pose_inertial_params& P, const PioArgs& a, const double* view, int lf, int rnd,
                                   const uint8_t* outlier_in, const float* chi2_in, uint8_t* code) {
    hipLaunchKernelGGL(pose_inertial_classify_kernel, dim3(1), dim3(PIO_LANES), 0, s, P, a, view, lf, rnd, outlier_in, chi2_in, code);
}

void launch_pose_inertial(hipStream_t s, const rfe_pose_inertial_params& P, const PioArgs& a, int B) {
    if (B <= 0) return;
    hipLaunchKernelGGL(pose_inertial_kernel, dim3(B), dim3(PIO_LANES), 0, s, P, a);
}

}  // namespace rfe
