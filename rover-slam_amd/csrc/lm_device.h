// lm_device.h -- device functions the Levenberg-Marquardt kernels share (pose_opt.hip; optimize_sim3.hip, 6k; local_ba.hip, 6l;
// essential_graph.hip, 6m): the explicit sin / cos of departure (b), exp, log and acos after fdlibm, Eigen's quaternion arithmetic, SE3Quat's
// exp and product, Sim3's exp, product, inverse, map and log with its 3 x 3 elimination, the pivoted LDLT of departure (c) on a D x D
// system and the stride-halving reduction of departure (a).  Everything is double, one rounding per operation (-ffp-contract=off); the
// numpy restatements tests/pose_opt_ref.py, tests/optimize_sim3_ref.py and tests/essential_graph_ref.py state the same operations in the
// same order.
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

// ---------------------------------------------------------------- Sim3 (q x y z w, t, s): 6k's exp, product with an estimate and inverse
// Sim3(update) (sim3.h:70-142): u = omega, upsilon, sigma -> q (not normalised), t, s
__device__ inline void lm_sim3_exp(const double (&u)[7], double* q, double* t, double& s) {
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double Om2[3][3], R[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Om2[r][c] = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
    s = lm_exp(sigma);
    const double eps = 0.00001;
    double A, B, C;
    double sn = 0.0, cs = 1.0;
    const bool small = theta < eps;
    if (!small) po_sincos(theta, sn, cs);
    if (small) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] = (((r == c) ? 1.0 : 0.0) + Om[r][c]) + Om2[r][c];
    } else {
        const double a = sn / theta, bq = (1.0 - cs) / (theta * theta);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] = (((r == c) ? 1.0 : 0.0) + a * Om[r][c]) + bq * Om2[r][c];
    }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small) {
            A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    po_mat_to_quat(R, q);
    double W[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W[r][c] = (A * Om[r][c] + B * Om2[r][c]) + C * ((r == c) ? 1.0 : 0.0);
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = (W[r][0] * u[3] + W[r][1] * u[4]) + W[r][2] * u[5];
}

// Sim3(u) * base (sim3.h:266-272): r = r1 r2, t = s1 (r1 * t2) + t1, s = s1 s2; nothing is normalised
__device__ inline void lm_sim3_oplus(const double (&u)[7], const double* base, double* out) {
    double q1[4], t1[3], s1;
    lm_sim3_exp(u, q1, t1, s1);
    po_quat_mul(q1, base, out);
    double r0, r1, r2;
    po_rotate(q1, base[4], base[5], base[6], r0, r1, r2);
    out[4] = s1 * r0 + t1[0]; out[5] = s1 * r1 + t1[1]; out[6] = s1 * r2 + t1[2];
    out[7] = s1 * base[7];
}

// inverse (sim3.h:233-236): (conj r, conj r * ((-1 / s) t), 1 / s)
__device__ inline void lm_sim3_inverse(const double* in, double* out) {
    out[0] = -in[0]; out[1] = -in[1]; out[2] = -in[2]; out[3] = in[3];
    const double c = -1. / in[7];
    po_rotate(out, c * in[4], c * in[5], c * in[6], out[4], out[5], out[6]);
    out[7] = 1. / in[7];
}

// A * B (sim3.h:266-272): r = r1 r2, t = s1 (r1 * t2) + t1, s = s1 s2; nothing is normalised
__device__ inline void lm_sim3_mul(const double* A, const double* B, double* out) {
    po_quat_mul(A, B, out);
    double r0, r1, r2;
    po_rotate(A, B[4], B[5], B[6], r0, r1, r2);
    out[4] = A[7] * r0 + A[4]; out[5] = A[7] * r1 + A[5]; out[6] = A[7] * r2 + A[6];
    out[7] = A[7] * B[7];
}
// S.map(X) = s (r * X) + t
__device__ inline void lm_sim3_map(const double* S, double X0, double X1, double X2, double& o0, double& o1, double& o2) {
    double r0, r1, r2;
    po_rotate(S, X0, X1, X2, r0, r1, r2);
    o0 = S[7] * r0 + S[4]; o1 = S[7] * r1 + S[5]; o2 = S[7] * r2 + S[6];
}

// ---------------------------------------------------------------- log and acos (6m's departure (e)): fdlibm's e_log and e_acos without fma
// x = 2^k (1 + f) with sqrt(2)/2 < 1 + f < sqrt(2), split on the high word as fdlibm does; s = f / (2 + f), the two interleaved polynomials,
// the k == 0 and k != 0 sums, none of fdlibm's short cuts.  x < 0 and NaN give NaN, 0 gives -inf, inf gives inf
__device__ inline double lm_log(double x) {
    if (x != x || x < 0) return __longlong_as_double(0x7ff8000000000000LL);
    if (x == 0) return -HUGE_VAL;
    if (x == HUGE_VAL) return x;
    long long sub = 0;
    if (x < 2.2250738585072014e-308) { x = x * 18014398509481984.0; sub = 54; }
    const long long bits = __double_as_longlong(x);
    long long k = (bits >> 52) - 1023 - sub;
    const long long m = bits & 0xFFFFFFFFFFFFFLL;
    const long long i = ((m >> 32) + 0x95F64) & 0x100000;
    k += i >> 20;
    const double f = __longlong_as_double(m | ((0x3FF00000LL ^ i) << 32)) - 1.0;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double R = t2 + t1;
    const double hfsq = (0.5 * f) * f;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}
__device__ inline double lm_acos_r(double z) {
    const double p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 +
                     z * (-4.00555345006794114027e-02 + z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
    const double q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 +
                     z * 7.70381505559019352791e-02)));
    return p / q;
}
// |x| < 0.5 through x^2; x < -0.5 and x > 0.5 through sqrt((1 -+ x) / 2), the latter with the root's low word cleared.  |x| > 1 and NaN
// give NaN, acos(1) == 0
__device__ inline double lm_acos(double x) {
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
    if (!(fabs(x) <= 1.0)) return __longlong_as_double(0x7ff8000000000000LL);
    if (x == 1.0) return 0.0;
    if (x == -1.0) return pi + 2.0 * pio2_lo;
    if (fabs(x) < 0.5) {
        if (fabs(x) < 6.938893903907228e-18) return pio2_hi + pio2_lo;
        const double r = lm_acos_r(x * x);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (x < 0) {
        const double z = (1.0 + x) * 0.5;
        const double s = sqrt(z);
        const double w = lm_acos_r(z) * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;
    const double s = sqrt(z);
    const double df = __longlong_as_double((__double_as_longlong(s) >> 32) << 32);
    const double c = (z - df * df) / (s + df);
    const double w = lm_acos_r(z) * s + c;
    return 2.0 * (df + w);
}

// ---------------------------------------------------------------- 6m's departure (f): W x = t, 3 x 3, partial pivoting
// column 0: the row with the largest |W[r][0]| (the first maximum) comes first, rows 1 and 2 lose l = W[r][0] / W[0][0] times row 0;
// column 1 likewise over rows 1, 2; then x2, x1, x0.  The swaps compare and exchange named rows, so every index is a constant
__device__ inline void lm_lu3_swap(double (&W)[3][3], double (&t)[3], int a, int b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { const double u = W[a][c]; W[a][c] = W[b][c]; W[b][c] = u; }
    const double u = t[a]; t[a] = t[b]; t[b] = u;
}
__device__ inline void lm_lu3_solve(double (&W)[3][3], double (&t)[3], double (&x)[3]) {
    const double a0 = fabs(W[0][0]), a1 = fabs(W[1][0]), a2 = fabs(W[2][0]);
    const bool p1 = a1 > a0;
    const bool p2 = a2 > (p1 ? a1 : a0);
    if (p2) lm_lu3_swap(W, t, 0, 2);
    else if (p1) lm_lu3_swap(W, t, 0, 1);
#pragma unroll
    for (int r = 1; r < 3; ++r) {
        const double l = W[r][0] / W[0][0];
        W[r][1] = W[r][1] - l * W[0][1];
        W[r][2] = W[r][2] - l * W[0][2];
        t[r] = t[r] - l * t[0];
    }
    if (fabs(W[2][1]) > fabs(W[1][1])) lm_lu3_swap(W, t, 1, 2);
    const double l = W[2][1] / W[1][1];
    W[2][2] = W[2][2] - l * W[1][2];
    t[2] = t[2] - l * t[1];
    x[2] = t[2] / W[2][2];
    x[1] = (t[1] - W[1][2] * x[2]) / W[1][1];
    x[0] = ((t[0] - W[0][1] * x[1]) - W[0][2] * x[2]) / W[0][0];
}

// ---------------------------------------------------------------- Sim3::log (sim3.h:148-230): S -> omega, upsilon, sigma
__device__ inline void lm_sim3_log(const double* S, double* res) {
    const double s = S[7];
    const double sigma = lm_log(s);
    const double qx = S[0], qy = S[1], qz = S[2], qw = S[3];
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const double R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy, R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx,
                 R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy);
    const double d = 0.5 * (((R00 + R11) + R22) - 1);
    const double dR0 = R21 - R12, dR1 = R02 - R20, dR2 = R10 - R01;
    const double eps = 0.00001;
    const bool near = d > 1 - eps;
    double A, B, C, k;
    double theta = 0.0, theta2 = 0.0, sn = 0.0, cs = 1.0;
    if (near) {
        k = 0.5;
    } else {
        theta = lm_acos(d);
        theta2 = theta * theta;
        k = theta / (2 * sqrt(1 - d * d));
        po_sincos(theta, sn, cs);
    }
    const double o0 = k * dR0, o1 = k * dR1, o2 = k * dR2;
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (near) { A = 1. / 2.; B = 1. / 6.; }
        else { A = (1 - cs) / theta2; B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs;
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = ((C - ((b - 1) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    const double Om[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double W[3][3], t[3] = {S[4], S[5], S[6]}, x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double om2 = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
            W[r][c] = (A * Om[r][c] + B * om2) + C * ((r == c) ? 1.0 : 0.0);
        }
    lm_lu3_solve(W, t, x);
    res[0] = o0; res[1] = o1; res[2] = o2; res[3] = x[0]; res[4] = x[1]; res[5] = x[2]; res[6] = sigma;
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
