// two_view.hip -- TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:49-1221, GeometricTools::Triangulate) with
// every RANSAC iteration of both models evaluated at once, DESIGN.md 6o.  Five launches:
//   * tv_front_kernel:      one workgroup per problem: the index check, the matches as structure-of-arrays rows (u1, v1, u2, v2), Normalize of
//                           both frames over ALL their keypoints (T1, T2, T2inv), and one thread per iteration resolving its 8-set from the
//                           raw draws (the swap-with-back list of :99-115, its at most 8 displaced entries in registers).
//   * tv_hypothesis_kernel: ONE WAVE per (problem, iteration, model), four per workgroup: the 16 x 9 (ComputeH21) or 8 x 9 (ComputeF21) system
//                           and V in a per-wave LDS tile (900 bytes), a fixed-schedule one-sided Jacobi with one lane per row, the rank-2
//                           enforcement (F), the denormalisation, and the score with the 64 lanes strided over the matches (16-byte loads).
//                           Nine columns and data-dependent rotations: nothing here is matmul-shaped, so no MFMA.
//   * tv_select_kernel:     one workgroup per problem: the first maximum of each model, RH, the winner's flags through the device function the
//                           scores came from, and the 3 x 3 decomposition into 4 (DecomposeE) or 8 (Faugeras) motion hypotheses.
//   * tv_check_rt_kernel:   one thread per (motion hypothesis, match): CheckRT's Triangulate (jacobi_null.h, PIXEL units) and gates.
//   * tv_final_kernel:      one workgroup per problem: nGood, the min(50, size - 1)-th smallest cosine by a radix select on the ordered keys,
//                           ReconstructF's / ReconstructH's decision, the outputs.
// fp32 with one rounding per written operation (-ffp-contract=off, plain / and sqrtf), sums left to right.  tests/two_view_ref.py restates
// all of it operation by operation.
#include "rfe_internal.h"
#include "jacobi_null.h"
#include "lm_device.h"

namespace rfe {
namespace {

// sweep counts of departure (a): where every decision and output settles on the test generators, plus two
constexpr int TV_SWEEPS_H = 9, TV_SWEEPS_F = 10, TV_SWEEPS_3 = 6, TV_SWEEPS_TRI = 6;
constexpr float TV_TH_H = 5.991f, TV_TH_F = 3.841f, TV_TH_SCORE = 5.991f;
// `cosParallax < 0.99998` compares the float with a DOUBLE literal (:1090).  fl32(0.99998) = 0x1.fffd6p-1 lies BELOW its literal:
// `(double)c < 0.99998` is `c <= fl32(0.99998)`, that is `c <` its upper neighbour 0x1.fffd62p-1.  `d1 / d2 < 1.00001` (:777) likewise:
// fl32(1.00001) = 0x1.0000a8p+0 lies ABOVE its literal, so `(double)q < 1.00001` is `q < fl32(1.00001)`.
constexpr float TV_COS_99998 = 0x1.fffd62p-1f, TV_RATIO_100001 = 0x1.0000a8p+0f;
static_assert(0x1.fffd6p-1f == 0.99998f && (double)0x1.fffd6p-1f < 0.99998 && (double)TV_COS_99998 > 0.99998, "bound of cosParallax");
static_assert(TV_RATIO_100001 == 1.00001f && (double)TV_RATIO_100001 > 1.00001 && (double)0x1.0000a6p+0f < 1.00001, "bound of the singular-value ratios");
enum { TV_FLAG_FEW = 1, TV_FLAG_INDEX = 2, TV_FLAG_NONFINITE = 4 };
enum { TV_EXIT_OK = 0, TV_EXIT_NO_SCORE = 1, TV_EXIT_SINGULAR = 2, TV_EXIT_NO_WINNER = 3, TV_EXIT_FEW = 4, TV_EXIT_PARALLAX = 5 };

struct TvChunk { rfe_two_view_params p[TV_MAX_B]; };

__device__ __forceinline__ void tv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// C = A B, every sum left to right
__device__ __forceinline__ void tv_mul3(const float (&A)[9], const float (&B)[9], float (&C)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
__device__ __forceinline__ void tv_transpose3(const float (&A)[9], float (&T)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = A[3 * c + r];
}
__device__ __forceinline__ float tv_det3(const float (&M)[9]) {
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
// departure (b): the cofactor inverse, every entry divided by the determinant
__device__ __forceinline__ void tv_inv3(const float (&M)[9], float (&I)[9]) {
    const float c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const float det = (M[0] * c00 + M[1] * c01) + M[2] * c02;
    I[0] = c00 / det; I[1] = (M[2] * M[7] - M[1] * M[8]) / det; I[2] = (M[1] * M[5] - M[2] * M[4]) / det;
    I[3] = c01 / det; I[4] = (M[0] * M[8] - M[2] * M[6]) / det; I[5] = (M[2] * M[3] - M[0] * M[5]) / det;
    I[6] = c02 / det; I[7] = (M[1] * M[6] - M[0] * M[7]) / det; I[8] = (M[0] * M[4] - M[1] * M[3]) / det;
}
__device__ __forceinline__ void tv_tmat(const float (&T)[4], float (&M)[9]) {   // Normalize's T from (sX, sY, -meanX sX, -meanY sY)
    M[0] = T[0]; M[1] = 0.f; M[2] = T[2]; M[3] = 0.f; M[4] = T[1]; M[5] = T[3]; M[6] = 0.f; M[7] = 0.f; M[8] = 1.f;
}

// departure (a) for the 3 x 3 problems: one-sided Jacobi on the columns of M (row-major), pairs (0,1)(0,2)(1,2), a pair left alone when
// gamma^2 <= 2^-40 alpha beta (jacobi_null.h); the singular values are the norms of the rotated columns, sorted descending (a stable
// three-element network), U's columns the rotated columns over their norms, and u2 = u0 x u1 where the third singular value is zero.
// U, V row-major
__device__ __forceinline__ void tv_svd3(const float (&M)[9], float (&U)[9], float (&w)[3], float (&V)[9]) {
    float A[3][3], W[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) { A[r][c] = M[3 * r + c]; W[r][c] = r == c ? 1.f : 0.f; }
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SWEEPS_3; ++sweep)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const float alpha = (A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p];
                const float beta = (A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q];
                const float gamma = (A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q];
                const bool rot = !(gamma * gamma <= JACOBI_TOL2 * (alpha * beta));
                const float zeta = (beta - alpha) / (2.f * gamma);
                const float t = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
                const float c = 1.f / sqrtf(1.f + t * t);
                const float s = c * t;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float ap = A[r][p], aq = A[r][q], vp = W[r][p], vq = W[r][q];
                    A[r][p] = rot ? c * ap - s * aq : ap; A[r][q] = rot ? s * ap + c * aq : aq;
                    W[r][p] = rot ? c * vp - s * vq : vp; W[r][q] = rot ? s * vp + c * vq : vq;
                }
            }
    float n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = sqrtf((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
    const int net[3][2] = {{0, 1}, {1, 2}, {0, 1}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = net[k][0], b = net[k][1];
        const bool sw = n[b] > n[a];                                     // equal norms (and NaN) keep their order
        const float na = n[a], nb = n[b];
        n[a] = sw ? nb : na; n[b] = sw ? na : nb;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float x = A[r][a], y = A[r][b], u = W[r][a], v = W[r][b];
            A[r][a] = sw ? y : x; A[r][b] = sw ? x : y; W[r][a] = sw ? v : u; W[r][b] = sw ? u : v;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w[c] = n[c];
#pragma unroll
        for (int r = 0; r < 3; ++r) { U[3 * r + c] = A[r][c] / n[c]; V[3 * r + c] = W[r][c]; }
    }
    if (n[2] == 0.f) {
        U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

// CheckHomography (:382-466) / CheckFundamental (:474-556) of ONE match: adds to sc what the match adds to the score, returns bIn
__device__ __forceinline__ bool tv_check_h(const float (&H)[9], const float (&Hi)[9], float u1, float v1, float u2, float v2, float invs2, float& sc) {
    bool in = true;
    const float w2 = 1.f / ((Hi[6] * u2 + Hi[7] * v2) + Hi[8]);
    const float u2in1 = ((Hi[0] * u2 + Hi[1] * v2) + Hi[2]) * w2, v2in1 = ((Hi[3] * u2 + Hi[4] * v2) + Hi[5]) * w2;
    const float chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * invs2;
    if (chi1 > TV_TH_H) in = false; else sc = sc + (TV_TH_H - chi1);
    const float w1 = 1.f / ((H[6] * u1 + H[7] * v1) + H[8]);
    const float u1in2 = ((H[0] * u1 + H[1] * v1) + H[2]) * w1, v1in2 = ((H[3] * u1 + H[4] * v1) + H[5]) * w1;
    const float chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * invs2;
    if (chi2 > TV_TH_H) in = false; else sc = sc + (TV_TH_H - chi2);
    return in;
}
__device__ __forceinline__ bool tv_check_f(const float (&F)[9], float u1, float v1, float u2, float v2, float invs2, float& sc) {
    bool in = true;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2], b2 = (F[3] * u1 + F[4] * v1) + F[5], c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * invs2;
    if (chi1 > TV_TH_F) in = false; else sc = sc + (TV_TH_SCORE - chi1);
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7], c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * invs2;
    if (chi2 > TV_TH_F) in = false; else sc = sc + (TV_TH_SCORE - chi2);
    return in;
}
__device__ __forceinline__ bool tv_check(int model, const float (&M)[9], const float (&Mi)[9], float u1, float v1, float u2, float v2, float invs2,
                                         float& sc) {
    return model == 0 ? tv_check_h(M, Mi, u1, v1, u2, v2, invs2, sc) : tv_check_f(M, u1, v1, u2, v2, invs2, sc);
}

// CheckRT (:1016-1155) of ONE match: 0 = not counted, 1 = counted in nGood (p3d kept) without vbGood, 2 = counted and vbGood
__device__ __forceinline__ int tv_check_rt(const float (&R)[9], const float (&t)[3], float fx, float fy, float cx, float cy, float th2, float u1,
                                           float v1, float u2, float v2, float& cosp, float (&p)[3]) {
    // P1 = K [I | 0], P2 = K [R | t]
    const float P1[3][4] = {{fx, 0.f, cx, 0.f}, {0.f, fy, cy, 0.f}, {0.f, 0.f, 1.f, 0.f}};
    float P2[3][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float r0 = c < 3 ? R[c] : t[0], r1 = c < 3 ? R[3 + c] : t[1], r2 = c < 3 ? R[6 + c] : t[2];
        P2[0][c] = (fx * r0 + 0.f * r1) + cx * r2; P2[1][c] = (0.f * r0 + fy * r1) + cy * r2; P2[2][c] = (0.f * r0 + 0.f * r1) + 1.f * r2;
    }
    float A[4][4], h[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = u1 * P1[2][c] - P1[0][c]; A[1][c] = v1 * P1[2][c] - P1[1][c];
        A[2][c] = u2 * P2[2][c] - P2[0][c]; A[3][c] = v2 * P2[2][c] - P2[1][c];
    }
    jacobi_null4<TV_SWEEPS_TRI, true>(A, h);
    cosp = 0.f; p[0] = p[1] = p[2] = 0.f;
    if (h[3] == 0.f) return 0;                                           // departure (e)
    p[0] = h[0] / h[3]; p[1] = h[1] / h[3]; p[2] = h[2] / h[3];
    if (!((p[0] - p[0] == 0.f) && (p[1] - p[1] == 0.f) && (p[2] - p[2] == 0.f))) return 0;
    const float O2[3] = {-((R[0] * t[0] + R[3] * t[1]) + R[6] * t[2]), -((R[1] * t[0] + R[4] * t[1]) + R[7] * t[2]),
                         -((R[2] * t[0] + R[5] * t[1]) + R[8] * t[2])};
    const float dist1 = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    const float n2x = p[0] - O2[0], n2y = p[1] - O2[1], n2z = p[2] - O2[2];
    const float dist2 = sqrtf((n2x * n2x + n2y * n2y) + n2z * n2z);
    cosp = ((p[0] * n2x + p[1] * n2y) + p[2] * n2z) / (dist1 * dist2);
    const bool below = cosp < TV_COS_99998;
    if (p[2] <= 0.f && below) return 0;
    const float x2 = ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]) + t[0], y2 = ((R[3] * p[0] + R[4] * p[1]) + R[5] * p[2]) + t[1],
                z2 = ((R[6] * p[0] + R[7] * p[1]) + R[8] * p[2]) + t[2];
    if (z2 <= 0.f && below) return 0;
    const float iz1 = 1.f / p[2];
    const float e1x = ((fx * p[0]) * iz1 + cx) - u1, e1y = ((fy * p[1]) * iz1 + cy) - v1;
    if (e1x * e1x + e1y * e1y > th2) return 0;
    const float iz2 = 1.f / z2;
    const float e2x = ((fx * x2) * iz2 + cx) - u2, e2y = ((fy * y2) * iz2 + cy) - v2;
    if (e2x * e2x + e2y * e2y > th2) return 0;
    return below ? 2 : 1;
}

// sum of the workgroup's 256 values: the tree s = 128, 64, .., 1 with v[t] = v[t] + v[t + s]; every thread gets the result
__device__ __forceinline__ float tv_block_sum(float v, float* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// Normalize (:949-1000) of n keypoints: T = (sX, sY, -meanX sX, -meanY sY); the sums as thread-strided partials, then the tree
__device__ __forceinline__ void tv_normalize(const float* __restrict__ k, int n, float* sh, float (&T)[4]) {
    float sx = 0.f, sy = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { sx = sx + k[2 * i]; sy = sy + k[2 * i + 1]; }
    const float mx = tv_block_sum(sx, sh) / (float)n, my = tv_block_sum(sy, sh) / (float)n;
    float dx = 0.f, dy = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) { dx = dx + fabsf(k[2 * i] - mx); dy = dy + fabsf(k[2 * i + 1] - my); }
    const float ax = tv_block_sum(dx, sh) / (float)n, ay = tv_block_sum(dy, sh) / (float)n;
    T[0] = 1.f / ax; T[1] = 1.f / ay;
    T[2] = -mx * T[0]; T[3] = -my * T[1];
}

__global__ __launch_bounds__(256) void tv_front_kernel(const TvChunk K, const float* __restrict__ kpts1, const float* __restrict__ kpts2,
                                                       const int32_t* __restrict__ S, const int32_t* __restrict__ pairs,
                                                       const int32_t* __restrict__ draws, int N1max, int N2max, int Kmax, int Ks, int H,
                                                       TvProb* __restrict__ prob, float* __restrict__ soa, int32_t* __restrict__ sets) {
    __shared__ float sh[256];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const rfe_two_view_params& P = K.p[b];
    const int N = min(max(S[b], 0), Kmax), n1 = P.n1, n2 = P.n2;
    const int its = P.its == 0 ? 200 : P.its;
    const int32_t* pr = pairs + (size_t)b * Kmax * 2;
    const float* k1 = kpts1 + (size_t)b * N1max * 2;
    const float* k2 = kpts2 + (size_t)b * N2max * 2;
    float* F = soa + (size_t)b * 4 * Ks;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int k = tid; k < N; k += 256) {
        const int i = pr[2 * k], j = pr[2 * k + 1];
        const bool ok = i >= 0 && i < n1 && j >= 0 && j < n2;
        if (!ok) bad = 1;
        F[k] = ok ? k1[2 * i] : 0.f; F[Ks + k] = ok ? k1[2 * i + 1] : 0.f;
        F[2 * Ks + k] = ok ? k2[2 * j] : 0.f; F[3 * Ks + k] = ok ? k2[2 * j + 1] : 0.f;
    }
    float T1[4], T2[4];
    tv_normalize(k1, n1, sh, T1);
    tv_normalize(k2, n2, sh, T2);
    __syncthreads();
    const int flags = (N < 8 ? TV_FLAG_FEW : 0) | (bad ? TV_FLAG_INDEX : 0);
    if (tid == 0) {
        TvProb q;
        q.fx = P.fx; q.fy = P.fy; q.cx = P.cx; q.cy = P.cy;
        const float sigma = P.sigma == 0.f ? 1.f : P.sigma;
        const float sigma2 = sigma * sigma;
        q.invs2 = 1.f / sigma2; q.th2 = 4.f * sigma2;
        q.rh_threshold = P.rh_threshold == 0.f ? 0.5f : P.rh_threshold;
        q.min_parallax = P.min_parallax == 0.f ? 1.f : P.min_parallax;
        q.min_triangulated = P.min_triangulated == 0 ? 50 : P.min_triangulated;
        for (int k = 0; k < 4; ++k) { q.T1[k] = T1[k]; q.T2[k] = T2[k]; }
        float M[9];
        tv_tmat(T2, M);
        tv_inv3(M, q.T2inv);
        q.N = N; q.its = its; q.n1 = n1; q.n2 = n2; q.flags = flags;
        prob[b] = q;
    }
    if (flags) return;
    for (int h = tid; h < its; h += 256) {
        const int32_t* d = draws + ((size_t)b * H + h) * 8;
        int pos[8], val[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sz = N - j;
            int r = (int)(((double)d[j] / 2147483648.0) * (double)sz);      // RandomInt(0, sz - 1)
            r = r < 0 ? 0 : (r > sz - 1 ? sz - 1 : r);
            int idx = r, back = sz - 1;
#pragma unroll
            for (int e = 0; e < j; ++e) { idx = pos[e] == r ? val[e] : idx; back = pos[e] == sz - 1 ? val[e] : back; }
            pos[j] = r; val[j] = back;
            sets[((size_t)b * H + h) * 8 + j] = idx;
        }
    }
}

__global__ __launch_bounds__(256) void tv_hypothesis_kernel(const TvProb* __restrict__ prob, const float* __restrict__ kpts1,
                                                            const float* __restrict__ kpts2, const int32_t* __restrict__ pairs,
                                                            const float* __restrict__ soa, const int32_t* __restrict__ sets, int N1max,
                                                            int N2max, int Kmax, int Ks, int H, float* __restrict__ hmodels,
                                                            float* __restrict__ scores) {
    __shared__ float tile[4][25][9];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.x * 4 + wave, h = w >> 1, model = w & 1;
    const TvProb C = prob[b];
    if (h >= C.its || h >= H || C.flags) return;                          // wave-uniform
    float (*T)[9] = tile[wave];
    const int rows = model == 0 ? 16 : 8;
    const int32_t* set = sets + ((size_t)b * H + h) * 8;
    if (lane < 8) {                                                       // lane j builds the row(s) of the set's j-th match
        const int m = set[lane];
        const int i = pairs[((size_t)b * Kmax + m) * 2], j = pairs[((size_t)b * Kmax + m) * 2 + 1];
        const float* p1 = kpts1 + ((size_t)b * N1max + i) * 2;
        const float* p2 = kpts2 + ((size_t)b * N2max + j) * 2;
        const float u1 = p1[0] * C.T1[0] + C.T1[2], v1 = p1[1] * C.T1[1] + C.T1[3];
        const float u2 = p2[0] * C.T2[0] + C.T2[2], v2 = p2[1] * C.T2[1] + C.T2[3];
        if (model == 0) {
            float* a = T[2 * lane];
            a[0] = 0.f; a[1] = 0.f; a[2] = 0.f; a[3] = -u1; a[4] = -v1; a[5] = -1.f; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2;
            float* c = T[2 * lane + 1];
            c[0] = u1; c[1] = v1; c[2] = 1.f; c[3] = 0.f; c[4] = 0.f; c[5] = 0.f; c[6] = -u2 * u1; c[7] = -u2 * v1; c[8] = -u2;
        } else {
            float* a = T[lane];
            a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.f;
        }
    } else if (lane < 17) {
        float* v = T[16 + lane - 8];
#pragma unroll
        for (int c = 0; c < 9; ++c) v[c] = c == lane - 8 ? 1.f : 0.f;
    }
    tv_wave_sync();
    // one lane per row of A (rows) and of V (9): the column sums are read by every lane, top to bottom
    const int own = lane < rows ? lane : (lane < rows + 9 ? 16 + lane - rows : -1);
    const int sweeps = model == 0 ? TV_SWEEPS_H : TV_SWEEPS_F;
#pragma unroll 1
    for (int sweep = 0; sweep < sweeps; ++sweep)
#pragma unroll 1
        for (int p = 0; p < 8; ++p)
#pragma unroll 1
            for (int q = p + 1; q < 9; ++q) {
                float alpha = 0.f, beta = 0.f, gamma = 0.f;
                for (int r = 0; r < rows; ++r) {
                    const float ap = T[r][p], aq = T[r][q];
                    alpha = alpha + ap * ap; beta = beta + aq * aq; gamma = gamma + ap * aq;
                }
                if (!(gamma * gamma <= JACOBI_TOL2 * (alpha * beta))) {   // wave-uniform; NaN rotates (and spreads)
                    const float zeta = (beta - alpha) / (2.f * gamma);
                    const float t = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
                    const float c = 1.f / sqrtf(1.f + t * t);
                    const float s = c * t;
                    if (own >= 0) {
                        const float ap = T[own][p], aq = T[own][q];
                        T[own][p] = c * ap - s * aq; T[own][q] = s * ap + c * aq;
                    }
                }
                tv_wave_sync();
            }
    int cmin = 0;
    float nb = 0.f;
#pragma unroll 1
    for (int c = 0; c < 9; ++c) {
        float nc = 0.f;
        for (int r = 0; r < rows; ++r) nc = nc + T[r][c] * T[r][c];
        if (c == 0 || nc < nb) { nb = nc; cmin = c; }                     // the first minimum stays
    }
    float Mn[9], M[9], Mi[9], T1m[9], X[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Mn[k] = T[16 + k][cmin];
    tv_tmat(C.T1, T1m);
    if (model == 0) {                                                     // H21i = T2inv Hn T1, H12i its inverse
        tv_mul3(C.T2inv, Mn, X);
        tv_mul3(X, T1m, M);
        tv_inv3(M, Mi);
    } else {                                                              // rank 2, then F21i = T2^T Fn T1
        float U[9], sv[3], V[9], Fn[9], T2m[9], T2t[9];
        tv_svd3(Mn, U, sv, V);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Fn[3 * r + c] = (U[3 * r] * sv[0]) * V[3 * c] + (U[3 * r + 1] * sv[1]) * V[3 * c + 1];
        tv_tmat(C.T2, T2m);
        tv_transpose3(T2m, T2t);
        tv_mul3(T2t, Fn, X);
        tv_mul3(X, T1m, M);
#pragma unroll
        for (int k = 0; k < 9; ++k) Mi[k] = 0.f;
    }
    // the score: lane l takes the matches 4 (l + 64 j) .. + 3 in order, then the tree d = 32 .. 1 with v[l] = v[l] + v[l + d]
    const float* F = soa + (size_t)b * 4 * Ks;
    float sc = 0.f;
    for (int base = 0; base < C.N; base += 256) {
        const int i0 = base + 4 * lane;
        if (i0 < C.N) {
            const float4 a = *(const float4*)(F + i0), c = *(const float4*)(F + Ks + i0), d = *(const float4*)(F + 2 * Ks + i0),
                         e = *(const float4*)(F + 3 * Ks + i0);
            tv_check(model, M, Mi, a.x, c.x, d.x, e.x, C.invs2, sc);
            if (i0 + 1 < C.N) tv_check(model, M, Mi, a.y, c.y, d.y, e.y, C.invs2, sc);
            if (i0 + 2 < C.N) tv_check(model, M, Mi, a.z, c.z, d.z, e.z, C.invs2, sc);
            if (i0 + 3 < C.N) tv_check(model, M, Mi, a.w, c.w, d.w, e.w, C.invs2, sc);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sc = sc + __shfl_down(sc, d, 64);
    if (lane == 0) scores[((size_t)b * H + h) * 2 + model] = sc;
    if (lane < 9) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) v = lane == k ? M[k] : v;
        hmodels[(((size_t)b * H + h) * 2 + model) * 9 + lane] = v;
    }
}

__global__ __launch_bounds__(256) void tv_select_kernel(const TvProb* __restrict__ prob, const float* __restrict__ soa,
                                                        const float* __restrict__ hmodels, const float* __restrict__ scores, int Kmax, int Ks,
                                                        int H, TvSel* __restrict__ sel, uint8_t* __restrict__ winl,
                                                        uint8_t* __restrict__ inliers_h, uint8_t* __restrict__ inliers_f,
                                                        float* __restrict__ models) {
    __shared__ float bs[256];
    __shared__ int bh[256];
    __shared__ int cnt[2], nonfinite;
    const int b = blockIdx.x, tid = threadIdx.x;
    const TvProb C = prob[b];
    const int its = (C.flags || C.its > H) ? 0 : C.its;
    const float* F = soa + (size_t)b * 4 * Ks;
    if (tid == 0) { cnt[0] = cnt[1] = 0; nonfinite = 0; }
    __syncthreads();
    float best[2]; int win[2];
    for (int model = 0; model < 2; ++model) {
        float s = 0.f; int at = -1;
        for (int h = tid; h < its; h += 256) {
            const float v = scores[((size_t)b * H + h) * 2 + model];
            if (!(v - v == 0.f)) nonfinite = 1;
            if (v > s) { s = v; at = h; }                                 // the first maximum of this thread's ascending h
        }
        __syncthreads();
        bs[tid] = s; bh[tid] = at;
        __syncthreads();
        for (int st = 128; st >= 1; st >>= 1) {
            if (tid < st) {
                const float o = bs[tid + st]; const int oh = bh[tid + st];
                if (oh >= 0 && (o > bs[tid] || (o == bs[tid] && (bh[tid] < 0 || oh < bh[tid])))) { bs[tid] = o; bh[tid] = oh; }
            }
            __syncthreads();
        }
        best[model] = bh[0] >= 0 ? bs[0] : 0.f; win[model] = bh[0];
        __syncthreads();
    }
    // the winners' flags, by the device function their scores came from
    float Mw[2][9];
    for (int model = 0; model < 2; ++model) {
        float Mi[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { Mw[model][k] = win[model] >= 0 ? hmodels[(((size_t)b * H + win[model]) * 2 + model) * 9 + k] : 0.f; Mi[k] = 0.f; }
        if (model == 0) tv_inv3(Mw[0], Mi);
        uint8_t* out = model == 0 ? inliers_h : inliers_f;
        for (int k0 = 0; k0 < C.N; k0 += 256) {
            const int k = k0 + tid;
            bool in = false;
            if (k < C.N && win[model] >= 0) {
                float sc = 0.f;
                in = tv_check(model, Mw[model], Mi, F[k], F[Ks + k], F[2 * Ks + k], F[3 * Ks + k], C.invs2, sc);
            }
            if (k < C.N) {
                winl[((size_t)b * 2 + model) * Kmax + k] = in;
                if (out) out[(size_t)b * Kmax + k] = in;
            }
            const unsigned long long m = __ballot(in);
            if ((tid & 63) == 0 && m) atomicAdd(&cnt[model], (int)__popcll(m));
        }
    }
    __syncthreads();
    if (models && tid < 18) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 18; ++k) v = tid == k ? Mw[k / 9][k % 9] : v;
        models[(size_t)b * 18 + tid] = v;
    }
    if (tid != 0) return;
    TvSel o;
    o.SH = best[0]; o.SF = best[1]; o.RH = 0.f;
    o.win_h = win[0]; o.win_f = win[1]; o.cnt_h = cnt[0]; o.cnt_f = cnt[1];
    o.ncand = 0; o.model = 0; o.exit = TV_EXIT_OK; o.flags = C.flags | (nonfinite ? TV_FLAG_NONFINITE : 0);
    for (int c = 0; c < 8; ++c) for (int k = 0; k < 12; ++k) o.cand[c][k] = 0.f;
    const float Km[9] = {C.fx, 0.f, C.cx, 0.f, C.fy, C.cy, 0.f, 0.f, 1.f};
    if (o.SH + o.SF == 0.f) {
        o.exit = TV_EXIT_NO_SCORE;
    } else {
        o.RH = o.SH / (o.SH + o.SF);
        float U[9], w[3], V[9], Vt[9], X[9], A[9];
        if (o.RH > C.rh_threshold) {                                      // ReconstructH (:746-941)
            o.model = 1;
            float invK[9];
            tv_inv3(Km, invK);
            tv_mul3(invK, Mw[0], X);
            tv_mul3(X, Km, A);
            tv_svd3(A, U, w, V);
            tv_transpose3(V, Vt);
            const float s = tv_det3(U) * tv_det3(Vt);
            const float d1 = w[0], d2 = w[1], d3 = w[2];
            if (d1 / d2 < TV_RATIO_100001 || d2 / d3 < TV_RATIO_100001) {
                o.exit = TV_EXIT_SINGULAR;
            } else {
                const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
                const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
                const float root = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3));
                const float aux_st = root / ((d1 + d3) * d2), ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
                const float aux_sp = root / ((d1 - d3) * d2), cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
                const float sgn[4] = {1.f, -1.f, -1.f, 1.f};
                float sU[9];
                for (int k = 0; k < 9; ++k) sU[k] = s * U[k];
                for (int c = 0; c < 8; ++c) {
                    const int i = c & 3;
                    const bool second = c >= 4;
                    const float sn = sgn[i] * (second ? aux_sp : aux_st);
                    const float Rp[9] = {second ? cphi : ctheta, 0.f, second ? sn : -sn, 0.f, second ? -1.f : 1.f, 0.f, sn, 0.f, second ? -cphi : ctheta};
                    float R[9];
                    tv_mul3(sU, Rp, X);
                    tv_mul3(X, Vt, R);
                    const float scale = second ? d1 + d3 : d1 - d3;
                    const float tp0 = x1[i] * scale, tp1 = 0.f * scale, tp2 = (second ? x3[i] : -x3[i]) * scale;
                    const float t0 = (U[0] * tp0 + U[1] * tp1) + U[2] * tp2, t1 = (U[3] * tp0 + U[4] * tp1) + U[5] * tp2,
                                t2 = (U[6] * tp0 + U[7] * tp1) + U[8] * tp2;
                    const float nrm = sqrtf((t0 * t0 + t1 * t1) + t2 * t2);
                    for (int k = 0; k < 9; ++k) o.cand[c][k] = R[k];
                    o.cand[c][9] = t0 / nrm; o.cand[c][10] = t1 / nrm; o.cand[c][11] = t2 / nrm;
                }
                o.ncand = 8;
            }
        } else {                                                          // ReconstructF (:569-674), DecomposeE (:1194-1221)
            o.model = 2;
            float Kt[9], R1[9], R2[9], UW[9];
            tv_transpose3(Km, Kt);
            tv_mul3(Kt, Mw[1], X);
            tv_mul3(X, Km, A);
            tv_svd3(A, U, w, V);
            tv_transpose3(V, Vt);
            const float nrm = sqrtf((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8]);
            const float t[3] = {U[2] / nrm, U[5] / nrm, U[8] / nrm};
            for (int r = 0; r < 3; ++r) { UW[3 * r] = U[3 * r + 1]; UW[3 * r + 1] = -U[3 * r]; UW[3 * r + 2] = U[3 * r + 2]; }   // U W
            tv_mul3(UW, Vt, R1);
            if (tv_det3(R1) < 0.f) for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
            for (int r = 0; r < 3; ++r) { UW[3 * r] = -U[3 * r + 1]; UW[3 * r + 1] = U[3 * r]; UW[3 * r + 2] = U[3 * r + 2]; }   // U W^T
            tv_mul3(UW, Vt, R2);
            if (tv_det3(R2) < 0.f) for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
            for (int c = 0; c < 4; ++c) {
                for (int k = 0; k < 9; ++k) o.cand[c][k] = (c & 1) ? R2[k] : R1[k];
                for (int k = 0; k < 3; ++k) o.cand[c][9 + k] = c >= 2 ? -t[k] : t[k];
            }
            o.ncand = 4;
        }
    }
    sel[b] = o;
}

__global__ __launch_bounds__(256) void tv_check_rt_kernel(const TvProb* __restrict__ prob, const TvSel* __restrict__ sel,
                                                          const float* __restrict__ soa, const uint8_t* __restrict__ winl, int Kmax, int Ks,
                                                          uint8_t* __restrict__ rcode, float* __restrict__ rcos, float* __restrict__ rp) {
    const int b = blockIdx.z, c = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const TvSel& Q = sel[b];
    if (c >= Q.ncand) return;                                             // the launch shape does not depend on device data
    const TvProb& C = prob[b];
    if (k >= C.N) return;
    const size_t slot = ((size_t)b * 8 + c) * Kmax + k;
    int code = 0;
    float cosp = 0.f, p[3] = {0.f, 0.f, 0.f};
    if (winl[((size_t)b * 2 + (Q.model - 1)) * Kmax + k]) {
        float R[9], t[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = Q.cand[c][j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = Q.cand[c][9 + j];
        const float* F = soa + (size_t)b * 4 * Ks;
        code = tv_check_rt(R, t, C.fx, C.fy, C.cx, C.cy, C.th2, F[k], F[Ks + k], F[2 * Ks + k], F[3 * Ks + k], cosp, p);
    }
    rcode[slot] = (uint8_t)code; rcos[slot] = cosp;
    rp[3 * slot] = p[0]; rp[3 * slot + 1] = p[1]; rp[3 * slot + 2] = p[2];
}

// total order of the float bit patterns: negative values below positive ones, a (positive) NaN above +inf
__device__ __forceinline__ unsigned tv_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tv_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void tv_final_kernel(const TvProb* __restrict__ prob, const TvSel* __restrict__ sel,
                                                       const int32_t* __restrict__ pairs, const uint8_t* __restrict__ rcode,
                                                       const float* __restrict__ rcos, const float* __restrict__ rp, int N1max, int Kmax,
                                                       float* __restrict__ R21, float* __restrict__ t21, float* __restrict__ p3d,
                                                       uint8_t* __restrict__ triangulated, float* __restrict__ cand,
                                                       int32_t* __restrict__ stats) {
    __shared__ int s_cnt, s_good[8];
    __shared__ float s_par[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TvProb C = prob[b];
    const TvSel& Q = sel[b];
    const int ncand = Q.ncand, N = C.N;
    for (int c = 0; c < ncand; ++c) {
        const uint8_t* code = rcode + ((size_t)b * 8 + c) * Kmax;
        const float* cs = rcos + ((size_t)b * 8 + c) * Kmax;
        __syncthreads();
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        int mine = 0;
        for (int k = tid; k < N; k += 256) mine += code[k] != 0;
        if (mine) atomicAdd(&s_cnt, mine);
        __syncthreads();
        const int good = s_cnt;
        float parallax = 0.f;
        if (good > 0) {                                                   // wave- and workgroup-uniform
            int rem = min(50, good - 1);
            unsigned prefix = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned himask = bit == 31 ? 0u : ~((2u << bit) - 1u);    // the bits above `bit`
                __syncthreads();
                if (tid == 0) s_cnt = 0;
                __syncthreads();
                int z = 0;
                for (int k = tid; k < N; k += 256) {
                    const unsigned key = tv_key(cs[k]);
                    z += code[k] != 0 && (key & himask) == prefix && !((key >> bit) & 1u);
                }
                if (z) atomicAdd(&s_cnt, z);
                __syncthreads();
                const int zeros = s_cnt;
                if (rem >= zeros) { rem -= zeros; prefix |= 1u << bit; }
            }
            const float cv = tv_unkey(prefix);
            parallax = (float)((lm_acos((double)cv) * 180.0) / 3.141592653589793);      // departure (c)
        }
        if (tid == 0) { s_good[c] = good; s_par[c] = parallax; }
    }
    __syncthreads();
    // the decision
    int chosen = -1, exit_code = Q.exit;
    const int Ninl = Q.model == 1 ? Q.cnt_h : Q.cnt_f;
    if (Q.model == 2 && ncand == 4) {
        const int g0 = s_good[0], g1 = s_good[1], g2 = s_good[2], g3 = s_good[3];
        const int maxGood = max(g0, max(g1, max(g2, g3)));
        const int nMinGood = max((int)(0.9 * (double)Ninl), C.min_triangulated);
        const double lim = 0.7 * (double)maxGood;
        const int nsimilar = ((double)g0 > lim) + ((double)g1 > lim) + ((double)g2 > lim) + ((double)g3 > lim);
        if (maxGood < nMinGood) exit_code = TV_EXIT_FEW;
        else if (nsimilar > 1) exit_code = TV_EXIT_NO_WINNER;
        else {
            const int c = maxGood == g0 ? 0 : (maxGood == g1 ? 1 : (maxGood == g2 ? 2 : 3));
            if (s_par[c] > C.min_parallax) chosen = c; else exit_code = TV_EXIT_PARALLAX;
        }
    } else if (Q.model == 1 && ncand == 8) {
        int bestGood = 0, second = 0, bestIdx = -1;
        float bestPar = -1.f;
        for (int c = 0; c < 8; ++c) {
            const int g = s_good[c];
            if (g > bestGood) { second = bestGood; bestGood = g; bestIdx = c; bestPar = s_par[c]; }
            else if (g > second) second = g;
        }
        if (!((double)second < 0.75 * (double)bestGood)) exit_code = TV_EXIT_NO_WINNER;
        else if (!(bestPar >= C.min_parallax)) exit_code = TV_EXIT_PARALLAX;
        else if (!(bestGood > C.min_triangulated && (double)bestGood > 0.9 * (double)Ninl)) exit_code = TV_EXIT_FEW;
        else chosen = bestIdx;
    }
    // the outputs
    if (tid < 9) R21[(size_t)b * 9 + tid] = chosen >= 0 ? Q.cand[chosen][tid] : (tid % 4 == 0 ? 1.f : 0.f);
    if (tid < 3) t21[(size_t)b * 3 + tid] = chosen >= 0 ? Q.cand[chosen][9 + tid] : 0.f;
    for (int i = tid; i < C.n1; i += 256) {
        if (triangulated) triangulated[(size_t)b * N1max + i] = 0;
        if (p3d) { float* o = p3d + ((size_t)b * N1max + i) * 3; o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
    }
    __syncthreads();
    if (chosen >= 0) {
        const size_t base = ((size_t)b * 8 + chosen) * Kmax;
        for (int k = tid; k < N; k += 256) {
            const int code = rcode[base + k];
            if (!code) continue;
            const int i = pairs[((size_t)b * Kmax + k) * 2];              // inside 0..n1-1: the front checked it
            if (triangulated) triangulated[(size_t)b * N1max + i] = code == 2;
            if (p3d) { float* o = p3d + ((size_t)b * N1max + i) * 3; o[0] = rp[3 * (base + k)]; o[1] = rp[3 * (base + k) + 1]; o[2] = rp[3 * (base + k) + 2]; }
        }
    }
    if (cand && tid < 16 * ncand) {
        const int c = tid >> 4, k = tid & 15;
        cand[((size_t)b * 8 + c) * 16 + k] = k < 12 ? Q.cand[c][k] : (k == 12 ? (float)s_good[c] : (k == 13 ? s_par[c] : 0.f));
    }
    if (tid < 16) {
        int v = 0;
        switch (tid) {
            case 0: v = chosen >= 0; break;
            case 1: v = Q.model; break;
            case 2: v = N; break;
            case 3: v = Q.win_h; break;
            case 4: v = Q.win_f; break;
            case 5: v = Q.cnt_h; break;
            case 6: v = Q.cnt_f; break;
            case 7: v = chosen; break;
            case 8: v = __float_as_int(Q.SH); break;
            case 9: v = __float_as_int(Q.SF); break;
            case 10: v = __float_as_int(Q.RH); break;
            case 11: v = exit_code; break;
            case 12: v = Q.flags; break;
            default: break;
        }
        stats[(size_t)b * 16 + tid] = v;
    }
}

// the hooks: one model over given matches; one (R, t) over given matches
__global__ __launch_bounds__(256) void tv_hook_check_kernel(int model, const float* __restrict__ M9, float invs2, const float* __restrict__ pts, int n,
                                                            float* __restrict__ contrib, uint8_t* __restrict__ inl) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float M[9], Mi[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { M[j] = M9[j]; Mi[j] = 0.f; }
    if (model == 0) tv_inv3(M, Mi);
    float sc = 0.f;
    inl[k] = tv_check(model, M, Mi, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], invs2, sc);
    contrib[k] = sc;
}
__global__ __launch_bounds__(256) void tv_hook_check_rt_kernel(const float* __restrict__ Rt, float fx, float fy, float cx, float cy, float th2,
                                                               const float* __restrict__ pts, int n, uint8_t* __restrict__ code,
                                                               float* __restrict__ cosp, float* __restrict__ p3d) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float R[9], t[3], c, p[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = Rt[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = Rt[9 + j];
    code[k] = (uint8_t)tv_check_rt(R, t, fx, fy, cx, cy, th2, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], c, p);
    cosp[k] = c; p3d[3 * k] = p[0]; p3d[3 * k + 1] = p[1]; p3d[3 * k + 2] = p[2];
}

}  // namespace

void launch_two_view(hipStream_t s, const rfe_two_view_params* params, const float* kpts1, const float* kpts2, const int32_t* S,
                     const int32_t* pairs, const int32_t* draws, int B, int N1max, int N2max, int Kmax, int H, const TvBuffers& w, float* R21,
                     float* t21, float* p3d, uint8_t* triangulated, uint8_t* inliers_h, uint8_t* inliers_f, float* scores, float* models,
                     float* cand, int32_t* stats) {
    TvChunk K;
    for (int k = 0; k < TV_MAX_B; ++k) K.p[k] = params[k < B ? k : 0];
    const int Ks = tv_soa_stride(Kmax);
    hipLaunchKernelGGL(tv_front_kernel, dim3(B), dim3(256), 0, s, K, kpts1, kpts2, S, pairs, draws, N1max, N2max, Kmax, Ks, H, w.prob, w.soa, w.sets);
    hipLaunchKernelGGL(tv_hypothesis_kernel, dim3((2 * H + 3) / 4, B), dim3(256), 0, s, w.prob, kpts1, kpts2, pairs, w.soa, w.sets, N1max, N2max,
                       Kmax, Ks, H, w.hmodels, scores);
    hipLaunchKernelGGL(tv_select_kernel, dim3(B), dim3(256), 0, s, w.prob, w.soa, w.hmodels, scores, Kmax, Ks, H, w.sel, w.winl, inliers_h,
                       inliers_f, models);
    if (Kmax > 0)
        hipLaunchKernelGGL(tv_check_rt_kernel, dim3((Kmax + 255) / 256, 8, B), dim3(256), 0, s, w.prob, w.sel, w.soa, w.winl, Kmax, Ks, w.rcode,
                           w.rcos, w.rp);
    hipLaunchKernelGGL(tv_final_kernel, dim3(B), dim3(256), 0, s, w.prob, w.sel, pairs, w.rcode, w.rcos, w.rp, N1max, Kmax, R21, t21, p3d,
                       triangulated, cand, stats);
}

void launch_two_view_hook_check(hipStream_t s, int model, const float* M9, float invs2, const float* pts, int n, float* contrib, uint8_t* inl) {
    if (n > 0) hipLaunchKernelGGL(tv_hook_check_kernel, dim3((n + 255) / 256), dim3(256), 0, s, model, M9, invs2, pts, n, contrib, inl);
}
void launch_two_view_hook_check_rt(hipStream_t s, const float* Rt, float fx, float fy, float cx, float cy, float th2, const float* pts, int n,
                                   uint8_t* code, float* cosp, float* p3d) {
    if (n > 0) hipLaunchKernelGGL(tv_hook_check_rt_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Rt, fx, fy, cx, cy, th2, pts, n, code, cosp, p3d);
}

}  // namespace rfe
