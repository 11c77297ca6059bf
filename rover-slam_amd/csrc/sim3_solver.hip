// sim3_solver.hip -- Sim3Solver (reference src/Sim3Solver.cc:61-483) with every RANSAC hypothesis of a problem evaluated at once, DESIGN.md 6j.
//   * sim3_front_kernel:      one lane per correspondence: both map points into their camera frames and images, the two truncated error
//                             bounds (:61-121); structure-of-arrays rows in the workspace.  Its first lane of a problem also leaves the
//                             problem's camera and counts there, so the later launches take no per-problem argument by value.
//   * sim3_hypothesis_kernel: one WAVE per hypothesis, four per workgroup.  EVERY lane resolves the draws and runs ComputeSim3 redundantly
//                             (the operands are wave-uniform loads; no broadcast, no LDS), then the 64 lanes stride over the
//                             correspondences and count CheckInliers with a ballot and a population count.
//   * sim3_select_kernel:     one workgroup per problem: the first count above min_inliers, otherwise the last maximum; copies the chosen
//                             transform and recomputes its flags with the device function the counting used.
// fp32 with one rounding per operation (-ffp-contract=off), sums left to right; the Jacobi of departure (a) in double.
// tests/sim3_solver_ref.py restates all of it operation by operation.
#include "rfe_internal.h"

namespace rfe {
namespace {

constexpr int S3_SWEEPS = 8;
constexpr int S3_ROWS = 12;          // front rows of a problem: X1 xyz, X2 xyz, p1 uv, p2 uv, max1, max2
enum { S3_HYP_NAN = 1, S3_HYP_CLAMPED = 8 };
enum { S3_FLAG_FEW = 1, S3_FLAG_BELOW_THREE = 2, S3_FLAG_CLAMPED = 8 };

struct Sim3Chunk { rfe_sim3_solver_params p[S3_FRONT_CHUNK]; };

// what CheckInliers projects with: T12 = [sR | t], T21 = [sRi | ti]
struct Sim3Xf { float sR[9], t[3], sRi[9], ti[3]; };

__device__ __forceinline__ float s3_dot3(float a0, float a1, float a2, float x, float y, float z) { return (a0 * x + a1 * y) + a2 * z; }

// :406-419 from R, s and t: the same function in the hypothesis and in the selection kernel
__device__ __forceinline__ void s3_transforms(const float (&R)[9], float s, const float (&t)[3], Sim3Xf& X) {
    const float inv = (float)(1.0 / (double)s);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) { X.sR[3 * r + c] = s * R[3 * r + c]; X.sRi[3 * r + c] = inv * R[3 * c + r]; }
#pragma unroll
    for (int r = 0; r < 3; ++r) X.t[r] = t[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) X.ti[r] = -s3_dot3(X.sRi[3 * r], X.sRi[3 * r + 1], X.sRi[3 * r + 2], t[0], t[1], t[2]);
}

// CheckInliers (:423-447) of correspondence i; F: the problem's front rows, N apart
__device__ __forceinline__ bool s3_inlier(const Sim3Prob& C, const Sim3Xf& X, const float* __restrict__ F, int N, int i) {
    const float a0 = F[i], a1 = F[N + i], a2 = F[2 * N + i];                 // X1
    const float b0 = F[3 * N + i], b1 = F[4 * N + i], b2 = F[5 * N + i];     // X2
    const float x = s3_dot3(X.sR[0], X.sR[1], X.sR[2], b0, b1, b2) + X.t[0];
    const float y = s3_dot3(X.sR[3], X.sR[4], X.sR[5], b0, b1, b2) + X.t[1];
    const float z = s3_dot3(X.sR[6], X.sR[7], X.sR[8], b0, b1, b2) + X.t[2];
    const float d1x = F[6 * N + i] - ((C.fx1 * x) / z + C.cx1), d1y = F[7 * N + i] - ((C.fy1 * y) / z + C.cy1);
    const float u = s3_dot3(X.sRi[0], X.sRi[1], X.sRi[2], a0, a1, a2) + X.ti[0];
    const float v = s3_dot3(X.sRi[3], X.sRi[4], X.sRi[5], a0, a1, a2) + X.ti[1];
    const float w = s3_dot3(X.sRi[6], X.sRi[7], X.sRi[8], a0, a1, a2) + X.ti[2];
    const float d2x = ((C.fx2 * u) / w + C.cx2) - F[8 * N + i], d2y = ((C.fy2 * v) / w + C.cy2) - F[9 * N + i];
    const float e1 = d1x * d1x + d1y * d1y, e2 = d2x * d2x + d2y * d2y;
    return e1 < F[10 * N + i] && e2 < F[11 * N + i];                         // a NaN is an outlier
}

__global__ __launch_bounds__(256) void sim3_front_kernel(const Sim3Chunk K, int b0, const float* __restrict__ xw1, const float* __restrict__ xw2,
                                                         const float* __restrict__ sg1, const float* __restrict__ sg2, int N,
                                                         float* __restrict__ front, Sim3Prob* __restrict__ prob) {
    const rfe_sim3_solver_params& P = K.p[blockIdx.y];
    const int b = b0 + blockIdx.y;
    const int n = P.n < 0 ? 0 : (P.n > N ? N : P.n);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        Sim3Prob q;
        q.fx1 = P.fx1; q.fy1 = P.fy1; q.cx1 = P.cx1; q.cy1 = P.cy1; q.fx2 = P.fx2; q.fy2 = P.fy2; q.cx2 = P.cx2; q.cy2 = P.cy2;
        q.fix_scale = P.fix_scale; q.min_inliers = P.min_inliers; q.its = P.its; q.n = n;
        prob[b] = q;
    }
    if (i >= n) return;
    const size_t row = (size_t)b * N + i;
    float* F = front + (size_t)b * S3_ROWS * N;
    const float x1 = xw1[3 * row], y1 = xw1[3 * row + 1], z1 = xw1[3 * row + 2];
    const float x2 = xw2[3 * row], y2 = xw2[3 * row + 1], z2 = xw2[3 * row + 2];
    const float a0 = s3_dot3(P.rcw1[0], P.rcw1[1], P.rcw1[2], x1, y1, z1) + P.tcw1[0];
    const float a1 = s3_dot3(P.rcw1[3], P.rcw1[4], P.rcw1[5], x1, y1, z1) + P.tcw1[1];
    const float a2 = s3_dot3(P.rcw1[6], P.rcw1[7], P.rcw1[8], x1, y1, z1) + P.tcw1[2];
    const float c0 = s3_dot3(P.rcw2[0], P.rcw2[1], P.rcw2[2], x2, y2, z2) + P.tcw2[0];
    const float c1 = s3_dot3(P.rcw2[3], P.rcw2[4], P.rcw2[5], x2, y2, z2) + P.tcw2[1];
    const float c2 = s3_dot3(P.rcw2[6], P.rcw2[7], P.rcw2[8], x2, y2, z2) + P.tcw2[2];
    F[i] = a0; F[N + i] = a1; F[2 * N + i] = a2;
    F[3 * N + i] = c0; F[4 * N + i] = c1; F[5 * N + i] = c2;
    F[6 * N + i] = (P.fx1 * a0) / a2 + P.cx1; F[7 * N + i] = (P.fy1 * a1) / a2 + P.cy1;          // Pinhole::project
    F[8 * N + i] = (P.fx2 * c0) / c2 + P.cx2; F[9 * N + i] = (P.fy2 * c1) / c2 + P.cy2;
    F[10 * N + i] = (float)(unsigned long long)(9.210 * (double)sg1[row]);                       // mvnMaxError1 is a vector<size_t>
    F[11 * N + i] = (float)(unsigned long long)(9.210 * (double)sg2[row]);
}

// departure (a): eigenvector of the largest eigenvalue of the symmetric Nf, widened to double; cyclic Jacobi, pairs (0,1)(0,2)(0,3)(1,2)
// (1,3)(2,3), S3_SWEEPS sweeps, a rotation skipped when its off-diagonal entry is exactly zero.  Every index is a compile-time constant
__device__ __forceinline__ void s3_quaternion(const float (&Nf)[4][4], float (&q)[4]) {
    double A[4][4], V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { A[r][c] = (double)Nf[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < S3_SWEEPS; ++sweep)
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int r = p + 1; r < 4; ++r) {
                const double apq = A[p][r];
                if (apq != 0.0) {                                            // NaN rotates (and spreads)
                    const double theta = (A[r][r] - A[p][p]) / (2.0 * apq);
                    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(tt * tt + 1.0);
                    const double s = tt * c;
                    const double app = A[p][p] - tt * apq, arr = A[r][r] + tt * apq;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k != p && k != r) {
                            const double akp = A[k][p], akr = A[k][r];
                            const double np = c * akp - s * akr, nr = s * akp + c * akr;
                            A[k][p] = np; A[p][k] = np; A[k][r] = nr; A[r][k] = nr;
                        }
                        const double vkp = V[k][p], vkr = V[k][r];
                        V[k][p] = c * vkp - s * vkr; V[k][r] = s * vkp + c * vkr;
                    }
                    A[p][p] = app; A[r][r] = arr; A[p][r] = 0.0; A[r][p] = 0.0;
                }
            }
    double best = A[0][0], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = V[k][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool more = A[c][c] > best;                                    // maxCoeff: the first maximum stays
        best = more ? A[c][c] : best;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = more ? V[k][c] : v[k];
    }
    const double nrm = sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = v[k] / nrm;
    // w >= 0; at w == 0 the first non-zero component is positive
    const bool neg = v[0] < 0.0 || (v[0] == 0.0 && (v[1] < 0.0 || (v[1] == 0.0 && (v[2] < 0.0 || (v[2] == 0.0 && v[3] < 0.0)))));
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (float)(neg ? -v[k] : v[k]);
}

// ComputeSim3 (:319-420) on the triple P1, P2 (columns k = 0..2 of [r][k]): R, t, s; true: the NaN rotation of departure (b)
__device__ __forceinline__ bool s3_compute(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, float (&R)[9], float (&t)[3], float& s) {
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
        O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) { Pr1[r][k] = P1[r][k] - O1[r]; Pr2[r][k] = P2[r][k] - O2[r]; }
    }
    float M[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = (Pr2[r][0] * Pr1[c][0] + Pr2[r][1] * Pr1[c][1]) + Pr2[r][2] * Pr1[c][2];
    const double m00 = (double)M[0][0], m01 = (double)M[0][1], m02 = (double)M[0][2], m10 = (double)M[1][0], m11 = (double)M[1][1],
                 m12 = (double)M[1][2], m20 = (double)M[2][0], m21 = (double)M[2][1], m22 = (double)M[2][2];
    const float N11 = (float)((m00 + m11) + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10);
    const float N22 = (float)((m00 - m11) - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02);
    const float N33 = (float)((-m00 + m11) - m22), N34 = (float)(m12 + m21), N44 = (float)((-m00 - m11) + m22);
    const float Nf[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    float q[4];
    s3_quaternion(Nf, q);
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const bool nan_rot = sqrtf((x * x + y * y) + z * z) == 0.f;              // :375 divides 0 by 0
    if (nan_rot) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = __builtin_nanf("");
    } else {                                                                 // departure (b): Eigen's toRotationMatrix products
        const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
        const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
        R[0] = 1.0f - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
        R[3] = txy + twz; R[4] = 1.0f - (txx + tzz); R[5] = tyz - twx;
        R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0f - (txx + tyy);
    }
    float P3[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) P3[r][k] = (R[3 * r] * Pr2[0][k] + R[3 * r + 1] * Pr2[1][k]) + R[3 * r + 2] * Pr2[2][k];
    if (fix_scale) {
        s = 1.0f;
    } else {
        float nom = 0.0f, den = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k)                                          // column-major
#pragma unroll
            for (int r = 0; r < 3; ++r) { nom = nom + Pr1[r][k] * P3[r][k]; den = den + P3[r][k] * P3[r][k]; }
        s = (float)((double)nom / (double)den);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = O1[r] - s3_dot3(s * R[3 * r], s * R[3 * r + 1], s * R[3 * r + 2], O2[0], O2[1], O2[2]);
    return nan_rot;
}

// the reference's list of available indices after k pops, read at r without being materialised (:175-189)
__device__ __forceinline__ int s3_clamp(int r, int hi, int& flags) {
    const int c = r < 0 ? 0 : (r > hi ? hi : r);
    if (c != r) flags |= S3_HYP_CLAMPED;
    return c;
}

__global__ __launch_bounds__(256) void sim3_hypothesis_kernel(const Sim3Prob* __restrict__ prob, const float* __restrict__ front,
                                                              const int32_t* __restrict__ draws, int N, int H, int32_t* __restrict__ counts,
                                                              float* __restrict__ hyps) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
    const Sim3Prob C = prob[b];
    if (h >= C.its || h >= H || C.n < 3 || C.n < C.min_inliers) return;      // wave-uniform
    const int n = C.n;
    const float* F = front + (size_t)b * S3_ROWS * N;
    const int32_t* d = draws + ((size_t)b * H + h) * 3;
    int flags = 0;
    const int r0 = s3_clamp(d[0], n - 1, flags), r1 = s3_clamp(d[1], n - 2, flags), r2 = s3_clamp(d[2], n - 3, flags);
    const int back1 = r0 == n - 2 ? n - 1 : n - 2;                          // what the second pop moved into slot r1
    const int i0 = r0, i1 = r1 == r0 ? n - 1 : r1, i2 = r2 == r1 ? back1 : (r2 == r0 ? n - 1 : r2);
    const int idx[3] = {i0, i1, i2};
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) { P1[r][k] = F[r * N + idx[k]]; P2[r][k] = F[(3 + r) * N + idx[k]]; }
    float R[9], t[3], s;
    if (s3_compute(P1, P2, C.fix_scale != 0, R, t, s)) flags |= S3_HYP_NAN;
    Sim3Xf X;
    s3_transforms(R, s, t, X);
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {                               // the wave walks the rows 64 at a time
        const int i = base + lane;
        const bool in = i < n && s3_inlier(C, X, F, N, i);
        cnt += __popcll(__ballot(in));
    }
    if (lane == 0) counts[(size_t)b * H + h] = cnt;
    float* o = hyps + ((size_t)b * H + h) * 32;
    // the record: T12 [16], R [9], t [3], s, flags, 0, 0 -- lane k stores entry k
    const float rec[32] = {X.sR[0], X.sR[1], X.sR[2], t[0], X.sR[3], X.sR[4], X.sR[5], t[1], X.sR[6], X.sR[7], X.sR[8], t[2], 0.f, 0.f, 0.f, 1.f,
                           R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], t[0], t[1], t[2], s, __int_as_float(flags), 0.f, 0.f};
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) v = lane == k ? rec[k] : v;
    if (lane < 32) o[lane] = v;
}

__global__ __launch_bounds__(256) void sim3_select_kernel(const Sim3Prob* __restrict__ prob, const float* __restrict__ front,
                                                          const int32_t* __restrict__ counts, const float* __restrict__ hyps, int N, int H,
                                                          float* __restrict__ T12, float* __restrict__ Ro, float* __restrict__ to,
                                                          float* __restrict__ so, uint8_t* __restrict__ inliers,
                                                          uint8_t* __restrict__ best_inliers, int32_t* __restrict__ stats) {
    __shared__ int first, bestkey, nnan, clamped;
    const int b = blockIdx.x, lane = threadIdx.x;
    const Sim3Prob C = prob[b];
    const int n = C.n, its = C.its < H ? C.its : H;
    const int32_t* cnt = counts + (size_t)b * H;
    const float* hy = hyps + (size_t)b * H * 32;
    T12 += (size_t)b * 16; stats += (size_t)b * 8;
    if (n < 3 || n < C.min_inliers) {                                        // :158 / :228: no hypothesis is run
        if (lane < 16) T12[lane] = (lane & 3) == (lane >> 2) ? 1.f : 0.f;
        if (Ro && lane < 9) Ro[(size_t)b * 9 + lane] = lane % 4 == 0 ? 1.f : 0.f;
        if (to && lane < 3) to[(size_t)b * 3 + lane] = 0.f;
        if (so && lane == 0) so[b] = 1.f;
        for (int i = lane; i < n; i += 256) {
            if (inliers) inliers[(size_t)b * N + i] = 0;
            if (best_inliers) best_inliers[(size_t)b * N + i] = 0;
        }
        if (lane < 8)
            stats[lane] = lane == 3 ? -1 : (lane == 5 ? 1 : (lane == 7 ? (n < C.min_inliers ? S3_FLAG_FEW : 0) | (n < 3 ? S3_FLAG_BELOW_THREE : 0) : 0));
        return;
    }
    if (lane == 0) { first = its; bestkey = -1; nnan = 0; clamped = 0; }
    __syncthreads();
    for (int h = lane; h < its; h += 256) {
        const int c = cnt[h];
        if (c > C.min_inliers) atomicMin(&first, h);
        atomicMax(&bestkey, c * 1024 + h);                                   // the largest count, and among equals the last h
    }
    __syncthreads();
    const bool conv = first < its;
    const int chosen = conv ? first : (bestkey & 1023);
    const int iters = conv ? first + 1 : its;
    for (int h = lane; h < its; h += 256) {
        const int f = __float_as_int(hy[(size_t)h * 32 + 29]);
        if ((f & S3_HYP_NAN) && h < iters) atomicAdd(&nnan, 1);
        if (f & S3_HYP_CLAMPED) atomicOr(&clamped, 1);
    }
    const float* o = hy + (size_t)chosen * 32;
    if (lane < 16) T12[lane] = o[lane];
    if (Ro && lane < 9) Ro[(size_t)b * 9 + lane] = o[16 + lane];
    if (to && lane < 3) to[(size_t)b * 3 + lane] = o[25 + lane];
    if (so && lane == 0) so[b] = o[28];
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = o[16 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = o[25 + k];
    Sim3Xf X;
    s3_transforms(R, o[28], t, X);
    const float* F = front + (size_t)b * S3_ROWS * N;
    for (int i = lane; i < n; i += 256) {
        const bool in = s3_inlier(C, X, F, N, i);
        if (best_inliers) best_inliers[(size_t)b * N + i] = in ? 1 : 0;
        if (inliers) inliers[(size_t)b * N + i] = (conv && in) ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) {
        const int c = cnt[chosen];
        stats[0] = conv ? 1 : 0; stats[1] = conv ? c : 0; stats[2] = c; stats[3] = chosen; stats[4] = iters; stats[5] = conv ? 0 : 1;
        stats[6] = nnan; stats[7] = clamped ? S3_FLAG_CLAMPED : 0;
    }
}

}  // namespace

void launch_sim3_front(hipStream_t s, const rfe_sim3_solver_params* params, const float* xw1, const float* xw2, const float* sg1, const float* sg2,
                       int B, int N, Sim3Prob* prob, float* front) {
    for (int b0 = 0; b0 < B; b0 += S3_FRONT_CHUNK) {
        const int nb = B - b0 < S3_FRONT_CHUNK ? B - b0 : S3_FRONT_CHUNK;
        Sim3Chunk K;
        for (int k = 0; k < S3_FRONT_CHUNK; ++k) K.p[k] = params[b0 + (k < nb ? k : 0)];
        hipLaunchKernelGGL(sim3_front_kernel, dim3(N > 0 ? (N + 255) / 256 : 1, nb), dim3(256), 0, s, K, b0, xw1, xw2, sg1, sg2, N, front, prob);
    }
}

void launch_sim3_hypotheses(hipStream_t s, const Sim3Prob* prob, const float* front, const int32_t* draws, int B, int N, int H, int32_t* counts,
                            float* hyps) {
    hipLaunchKernelGGL(sim3_hypothesis_kernel, dim3((H + 3) / 4, B), dim3(256), 0, s, prob, front, draws, N, H, counts, hyps);
}

void launch_sim3_select(hipStream_t s, const Sim3Prob* prob, const float* front, const int32_t* counts, const float* hyps, int B, int N, int H,
                        float* T12, float* R, float* t, float* sc, uint8_t* inliers, uint8_t* best_inliers, int32_t* stats) {
    hipLaunchKernelGGL(sim3_select_kernel, dim3(B), dim3(256), 0, s, prob, front, counts, hyps, N, H, T12, R, t, sc, inliers, best_inliers, stats);
}

}  // namespace rfe
