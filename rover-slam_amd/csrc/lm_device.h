// lm_device.h -- device functions the Levenberg-Marquardt kernels share (pose_opt.hip; optimize_sim3.hip, 6k; local_ba.hip, 6l):
// the explicit sin / cos of departure (b), Eigen's quaternion arithmetic, SE3Quat's exp and product, the pivoted LDLT of departure (c) on a D x D system and the
// stride-halving reduction of departure (a).  Everything is double, one rounding per operation (-ffp-contract=off); the numpy restatements
// tests/pose_opt_ref.py and tests/optimize_sim3_ref.py state the same operations in the same order.
#pragma once
#include <hip/hip_runtime.h>

namespace rfe {

constexpr int LM_LANES = 256;

// ---------------------------------------------------------------- departure (b): sin and cos of theta >= 0
__device__ inline void po_sincos(double theta, double& s, double& c) {
    const double k = floor(theta * 0x1.45f306dc9c883p-1 + 0.5);
    double r = (((theta - k * 0x1.921fb544p+0) - k * 0x1.0b4611a6p-34) - k * 0x1.3198a2ep-69) - k * 0x1.b839a252049c1p-104;
    if (!(fabs(r) <= 0.79)) r = 0.0;
    const int q = isfinite(k) ? (int)(k - 4.0 * floor(k * 0.25)) : 0;
    const double z = r * r;
    double ps = 0x1.5d93a5acfd57cp-33;
    ps = -0x1.ae5e68a2b9cebp-26 + z * ps;
    ps = 0x1.71de357b1fe7dp-19 + z * ps;
    ps = -0x1.a01a019c161d5p-13 + z * ps;
    ps = 0x1.111111110f8a6p-7 + z * ps;
    ps = -0x1.5555555555549p-3 + z * ps;
    double sn = r + (r * z) * ps;
    double pc = -0x1.8fae9be8838d4p-37;
    pc = 0x1.1ee9ebdb4b1c4p-29 + z * pc;
    pc = -0x1.27e4f809c52adp-22 + z * pc;
    pc = 0x1.a01a019cb159p-16 + z * pc;
    pc = -0x1.6c16c16c15177p-10 + z * pc;
    pc = 0x1.555555555554cp-5 + z * pc;
    double cs = (1.0 - 0.5 * z) + (z * z) * pc;
    if (q == 1) { const double t = sn; sn = cs; cs = -t; }
    else if (q == 2) { sn = -sn; cs = -cs; }
    else if (q == 3) { const double t = sn; sn = -cs; cs = t; }
    s = fmin(fmax(sn, -1.0), 1.0);
    c = fmin(fmax(cs, -1.0), 1.0);
}

// ---------------------------------------------------------------- exp (6k's departure (d)): fdlibm's e_exp without fma
// k = floor(x / ln 2 + 0.5), r = (x - k ln2_hi) - k ln2_lo, the Remez polynomial in Horner form, an exact scaling by 2^k.  Total: NaN passes
// through, overflow gives inf, underflow 0; exp(0) == 1 exactly
__device__ inline double lm_exp(double x) {
    if (x != x) return x;
    if (x > 0x1.62e42fefa39efp+9) return HUGE_VAL;
    if (x < -0x1.74910d52d3051p+9) return 0.0;
    const double k = floor(x * 0x1.71547652b82fep+0 + 0.5);
    const double hi = x - k * 0x1.62e42feep-1, lo = k * 0x1.a39ef35793c76p-33;
    const double r = hi - lo;
    const double t = r * r;
    double p = 0x1.6376972bea4d0p-25;
    p = -0x1.bbd41c5d26bf1p-20 + t * p;
    p = 0x1.1566aaf25de2cp-14 + t * p;
    p = -0x1.6c16c16bebd93p-9 + t * p;
    p = 0x1.555555555553ep-3 + t * p;
    const double c = r - t * p;
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    return ldexp(y, (int)k);
}

// ---------------------------------------------------------------- quaternions (q = x y z w)
__device__ inline void po_normalize(double* q) {
    double x = q[0], y = q[1], z = q[2], w = q[3];
    if (w < 0) { x = -x; y = -y; z = -z; w = -w; }
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    q[0] = x / n; q[1] = y / n; q[2] = z / n; q[3] = w / n;
}
// Eigen's quaternion * vector: uv = 2 (v x X); X + w uv + v x uv
__device__ inline void po_rotate(const double* q, double X0, double X1, double X2, double& o0, double& o1, double& o2) {
    double u0 = q[1] * X2 - q[2] * X1, u1 = q[2] * X0 - q[0] * X2, u2 = q[0] * X1 - q[1] * X0;
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    const double c0 = q[1] * u2 - q[2] * u1, c1 = q[2] * u0 - q[0] * u2, c2 = q[0] * u1 - q[1] * u0;
    o0 = (X0 + q[3] * u0) + c0; o1 = (X1 + q[3] * u1) + c1; o2 = (X2 + q[3] * u2) + c2;
}
// Eigen's quaternion product a b
__device__ inline void po_quat_mul(const double* a, const double* b, double* q) {
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    q[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    q[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    q[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
    q[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
}
// Eigen's matrix -> quaternion, not normalised
__device__ inline void po_mat_to_quat(const double (&R)[3][3], double* q1) {
    double t = (R[0][0] + R[1][1]) + R[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q1[3] = 0.5 * t;
        t = 0.5 / t;
        q1[0] = (R[2][1] - R[1][2]) * t; q1[1] = (R[0][2] - R[2][0]) * t; q1[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > (i == 1 ? R[1][1] : R[0][0])) i = 2;
        // i, j = (i + 1) % 3, k = (j + 1) % 3, one branch per i so that no index is computed at run time
        if (i == 0) {
            t = sqrt(((R[0][0] - R[1][1]) - R[2][2]) + 1.0);
            q1[0] = 0.5 * t; t = 0.5 / t;
            q1[3] = (R[2][1] - R[1][2]) * t; q1[1] = (R[1][0] + R[0][1]) * t; q1[2] = (R[2][0] + R[0][2]) * t;
        } else if (i == 1) {
            t = sqrt(((R[1][1] - R[2][2]) - R[0][0]) + 1.0);
            q1[1] = 0.5 * t; t = 0.5 / t;
            q1[3] = (R[0][2] - R[2][0]) * t; q1[2] = (R[2][1] + R[1][2]) * t; q1[0] = (R[0][1] + R[1][0]) * t;
        } else {
            t = sqrt(((R[2][2] - R[0][0]) - R[1][1]) + 1.0);
            q1[2] = 0.5 * t; t = 0.5 / t;
            q1[3] = (R[1][0] - R[0][1]) * t; q1[0] = (R[0][2] + R[2][0]) * t; q1[1] = (R[1][2] + R[2][1]) * t;
        }
    }
}

// ---------------------------------------------------------------- SE3Quat::exp(x) * cur -> est (se3quat.h:223-257, :104-110)
// x: omega, upsilon; cur / est: q (x y z w), t.  false: est is not finite
__device__ inline bool lm_se3_exp_mul(const double* x, const double* cur, double* est) {
    const double o0 = x[0], o1 = x[1], o2 = x[2];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double Om2[3][3], R[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Om2[r][c] = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
    if (theta < 0.00001) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) { R[r][c] = (((r == c) ? 1.0 : 0.0) + Om[r][c]) + Om2[r][c]; V[r][c] = R[r][c]; }
    } else {
        double sn, cs;
        po_sincos(theta, sn, cs);
        const double a = sn / theta, bq = (1.0 - cs) / (theta * theta), g = (theta - sn) / ((theta * theta) * theta);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const double e = (r == c) ? 1.0 : 0.0;
                R[r][c] = (e + a * Om[r][c]) + bq * Om2[r][c];
                V[r][c] = (e + bq * Om[r][c]) + g * Om2[r][c];
            }
    }
    double t1[3];
    for (int r = 0; r < 3; ++r) t1[r] = (V[r][0] * x[3] + V[r][1] * x[4]) + V[r][2] * x[5];
    double q1[4];
    po_mat_to_quat(R, q1);
    po_normalize(q1);
    // (q1, t1) * cur: t = t1 + q1 * t_cur, q = q1 q_cur, normalised
    double r0, r1, r2;
    po_rotate(q1, cur[4], cur[5], cur[6], r0, r1, r2);
    est[4] = t1[0] + r0; est[5] = t1[1] + r1; est[6] = t1[2] + r2;
    double q[4];
    po_quat_mul(q1, cur, q);
    po_normalize(q);
    bool fin = true;
    for (int i = 0; i < 4; ++i) { est[i] = q[i]; fin = fin && isfinite(q[i]); }
    for (int i = 4; i < 7; ++i) fin = fin && isfinite(est[i]);
    return fin;
}

// ---------------------------------------------------------------- departure (c): LDLT with diagonal pivoting on A = H + lambda I
// false: a negative pivot.  The solution replaces x only on success.  Every index is a compile-time constant after unrolling (the pivot's
// row is found by comparing with each candidate), so the matrix stays in registers
template <int D>
__device__ inline bool lm_ldlt_solve(const double (&H)[D][D], double lambda, const double (&b)[D], double (&x)[D]) {
    double A[D][D], y[D], d[D];
    int perm[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) A[i][j] = (i == j) ? H[i][j] + lambda : H[i][j];
        perm[i] = i;
        y[i] = b[i];                                     // permuted along with the rows: y[i] = b[perm[i]]
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        int p = k; double best = fabs(A[k][k]);
#pragma unroll
        for (int j = k + 1; j < D; ++j) {
            const double a = fabs(A[j][j]);
            if (a > best) { p = j; best = a; }
        }
#pragma unroll
        for (int r = k + 1; r < D; ++r)
            if (r == p) {
#pragma unroll
                for (int j = 0; j < D; ++j) { const double t = A[k][j]; A[k][j] = A[r][j]; A[r][j] = t; }
#pragma unroll
                for (int i = 0; i < D; ++i) { const double t = A[i][k]; A[i][k] = A[i][r]; A[i][r] = t; }
                const int t = perm[k]; perm[k] = perm[r]; perm[r] = t;
                const double u = y[k]; y[k] = y[r]; y[r] = u;
            }
        d[k] = A[k][k];
        if (d[k] < 0.0) return false;
#pragma unroll
        for (int i = k + 1; i < D; ++i) A[i][k] = (d[k] != 0.0) ? A[i][k] / d[k] : 0.0;
#pragma unroll
        for (int i = k + 1; i < D; ++i)
#pragma unroll
            for (int j = k + 1; j <= i; ++j) {
                const double v = A[i][j] - A[i][k] * A[k][j];
                A[i][j] = v; A[j][i] = v;
            }
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) y[i] = y[i] - A[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < D; ++i) y[i] = (d[i] != 0.0) ? y[i] / d[i] : 0.0;
#pragma unroll
    for (int i = D - 1; i >= 0; --i)
#pragma unroll
        for (int j = i + 1; j < D; ++j) y[i] = y[i] - A[j][i] * y[j];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int r = 0; r < D; ++r)
            if (perm[i] == r) x[r] = y[i];
    return true;
}

// ---------------------------------------------------------------- departure (a): the 256 partials by stride halving
// 128 and 64 through LDS (red: 128 * TERMS doubles), 32 .. 1 inside wave 0; lane 0 leaves the totals in out
template <int TERMS>
__device__ inline void lm_reduce(double (&acc)[TERMS], double* red, double* out, int lane) {
    if (lane >= 128)
#pragma unroll
        for (int c = 0; c < TERMS; ++c) red[c * 128 + (lane - 128)] = acc[c];
    __syncthreads();
    if (lane < 128)
#pragma unroll
        for (int c = 0; c < TERMS; ++c) acc[c] = acc[c] + red[c * 128 + lane];
    __syncthreads();
    if (lane >= 64 && lane < 128)
#pragma unroll
        for (int c = 0; c < TERMS; ++c) red[c * 128 + (lane - 64)] = acc[c];
    __syncthreads();
    if (lane < 64) {
#pragma unroll
        for (int c = 0; c < TERMS; ++c) acc[c] = acc[c] + red[c * 128 + lane];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int c = 0; c < TERMS; ++c) acc[c] = acc[c] + __shfl_down(acc[c], s, 64);
        if (lane == 0)
#pragma unroll
            for (int c = 0; c < TERMS; ++c) out[c] = acc[c];
    }
}

}  // namespace rfe
