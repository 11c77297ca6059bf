// triangulate.hip -- LocalMapping::CreateNewMapPoints behind the matcher (reference src/LocalMapping.cc:662-943, the filter of
// SPmatcher::SearchForTriangulation at src/Matchers/SPmatcher.cc:1376-1393, GeometricTools::Triangulate, KeyFrame::UnprojectStereo) for the
// matches of all neighbours at once:
//   * tri_eval_kernel:    one thread per match slot (n, k): the filter, parallax, Triangulate (jacobi_null.h: a one-sided Jacobi null vector, fully unrolled:
//                         A and V stay in registers) or UnprojectStereo, and every gate in the reference's order.  fp32, one rounding per
//                         written operation (-ffp-contract=off, plain / and sqrtf); the reference's three double expressions in double.  A
//                         slot that passes claims its feature with atomicMin(claim[i], n): integer, so the outcome has no order in it.
//   * tri_resolve_kernel: a passing slot whose feature a lower neighbour claimed gets code 16; writes code / x3d / point_stereo, counts the
//                         winners per neighbour (ballot + popcount) and the statistics.
//   * tri_compact_kernel: one workgroup per neighbour: the exclusive prefix of the neighbours' counts, then the winners in slot order by a
//                         workgroup scan -- the list in creation order.
#include "rfe_internal.h"
#include "jacobi_null.h"

namespace rfe {

// `cosParallaxRays < 0.9998` and `< 0.9996` compare the float with DOUBLE literals (LocalMapping.cc:792).  fl32(0.9998) = 0x1.ffe5cap-1 lies
// above its literal: `(double)c < 0.9998` is `c < fl32(0.9998)`.  fl32(0.9996) = 0x1.ffcb92p-1 lies BELOW its literal: `(double)c < 0.9996`
// is `c <= fl32(0.9996)`, that is `c <` its upper neighbour 0x1.ffcb94p-1.  (NaN is false in every form.)
constexpr float TRI_COS_9998 = 0x1.ffe5cap-1f, TRI_COS_9996 = 0x1.ffcb94p-1f;
static_assert(TRI_COS_9998 == 0.9998f && (double)TRI_COS_9998 > 0.9998 && (double)0x1.ffe5c8p-1f < 0.9998, "bound of cosParallaxRays, not inertial");
static_assert(0x1.ffcb92p-1f == 0.9996f && (double)0x1.ffcb92p-1f < 0.9996 && (double)TRI_COS_9996 > 0.9996, "bound of cosParallaxRays, inertial");
constexpr int TRI_SWEEPS = 6;                 // decisions and points settle at 4 sweeps on the test generators, plus two
constexpr int TRI_CLAIMED = 16;

__device__ __forceinline__ float tri_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ float tri_norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }
// cos(2 atan2(mb / 2, depth)) as (d d - h h) / (d d + h h)
__device__ __forceinline__ float tri_stereo_parallax(float mb, float d) {
    const float h = mb / 2.f, dd = d * d, hh = h * h;
    return (dd - hh) / (dd + hh);
}

// reprojection gate of one view (LocalMapping.cc:842-867 / 875-893): true = the slot fails.  mbf is the CURRENT keyframe's in both views (:886)
__device__ __forceinline__ bool tri_reproj_fails(const rfe_tri_view& V, float X, float Y, float Z, float z, float kx, float ky, float ur, bool stereo,
                                                 float mbf, float sigma2) {
    const float x = tri_dot3(V.rcw[0], V.rcw[1], V.rcw[2], X, Y, Z) + V.tcw[0];
    const float y = tri_dot3(V.rcw[3], V.rcw[4], V.rcw[5], X, Y, Z) + V.tcw[1];
    if (!stereo) {
        const float ex = ((V.fx * x) / z + V.cx) - kx, ey = ((V.fy * y) / z + V.cy) - ky;      // Pinhole::project
        return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    }
    const float invz = (float)(1.0 / (double)z);
    const float u = (V.fx * x) * invz + V.cx;
    const float u_r = u - mbf * invz;
    const float ex = u - kx, ey = ((V.fy * y) * invz + V.cy) - ky, er = u_r - ur;
    return (double)((ex * ex + ey * ey) + er * er) > 7.8 * (double)sigma2;
}

// KeyFrame::UnprojectStereo behind its z > 0 test
__device__ __forceinline__ void tri_unproject(const rfe_tri_view& V, float u, float v, float z, float& X, float& Y, float& Z) {
    const float x = ((u - V.cx) * z) * V.invfx, y = ((v - V.cy) * z) * V.invfy;
    X = ((V.rcw[0] * x + V.rcw[3] * y) + V.rcw[6] * z) + V.ow[0];        // mRwc = Rcw^T
    Y = ((V.rcw[1] * x + V.rcw[4] * y) + V.rcw[7] * z) + V.ow[1];
    Z = ((V.rcw[2] * x + V.rcw[5] * y) + V.rcw[8] * z) + V.ow[2];
}

__global__ __launch_bounds__(256) void tri_eval_kernel(const rfe_tri_params P, const rfe_tri_view V1, const float* __restrict__ kpts1,
                                                       const float* __restrict__ kraw1, const int32_t* __restrict__ oct1,
                                                       const float* __restrict__ ur1, const float* __restrict__ dep1,
                                                       const uint8_t* __restrict__ mp1, int N1, const rfe_tri_view* __restrict__ views2,
                                                       const float* __restrict__ kpts2, const float* __restrict__ kraw2,
                                                       const int32_t* __restrict__ oct2, const float* __restrict__ ur2,
                                                       const float* __restrict__ dep2, const uint8_t* __restrict__ mp2,
                                                       const int32_t* __restrict__ n2, const uint8_t* __restrict__ nvalid, int N2max,
                                                       const int32_t* __restrict__ S, const int32_t* __restrict__ pairs, int Kmax,
                                                       int32_t* __restrict__ wcode, float* __restrict__ wx3d, uint8_t* __restrict__ wstereo,
                                                       int32_t* __restrict__ claim) {
    const int n = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Kmax) return;
    const size_t slot = (size_t)n * Kmax + k;
    int code = -1, i = 0;
    float X = 0.f, Y = 0.f, Z = 0.f;
    bool point_stereo = false;
    if (k < min(max(S[n], 0), Kmax)) do {
        code = 1;
        if (nvalid && !nvalid[n]) break;
        i = pairs[2 * slot];
        const int j = pairs[2 * slot + 1];
        code = 2;
        if (i < 0 || i >= N1 || j < 0 || j >= min(n2[n], N2max)) break;
        const size_t f2 = (size_t)n * N2max + j;
        code = 3;
        if (mp1[i] || mp2[f2]) break;
        const rfe_tri_view V2 = views2[n];                               // the same for the whole workgroup
        const float k1x = kpts1[2 * i], k1y = kpts1[2 * i + 1], k2x = kpts2[2 * f2], k2y = kpts2[2 * f2 + 1];
        const float kp1_ur = ur1[i], kp2_ur = ur2[f2];
        const bool st1 = kp1_ur >= 0.f, st2 = kp2_ur >= 0.f;
        const float a1 = (k1x - V1.cx) / V1.fx, b1 = (k1y - V1.cy) / V1.fy;              // Pinhole::unprojectEig
        const float a2 = (k2x - V2.cx) / V2.fx, b2 = (k2y - V2.cy) / V2.fy;
        const float r1x = (V1.rcw[0] * a1 + V1.rcw[3] * b1) + V1.rcw[6], r1y = (V1.rcw[1] * a1 + V1.rcw[4] * b1) + V1.rcw[7],
                    r1z = (V1.rcw[2] * a1 + V1.rcw[5] * b1) + V1.rcw[8];
        const float r2x = (V2.rcw[0] * a2 + V2.rcw[3] * b2) + V2.rcw[6], r2y = (V2.rcw[1] * a2 + V2.rcw[4] * b2) + V2.rcw[7],
                    r2z = (V2.rcw[2] * a2 + V2.rcw[5] * b2) + V2.rcw[8];
        const float cosr = tri_dot3(r1x, r1y, r1z, r2x, r2y, r2z) / (tri_norm3(r1x, r1y, r1z) * tri_norm3(r2x, r2y, r2z));
        float cs1 = cosr + 1.f, cs2 = cs1;
        if (st1) cs1 = tri_stereo_parallax(V1.mb, dep1[i]);
        else if (st2) cs2 = tri_stereo_parallax(V2.mb, dep2[f2]);        // as written: not when the first view is stereo
        const float cst = cs2 < cs1 ? cs2 : cs1;                          // std::min
        if (cosr < cst && cosr > 0.f && (st1 || st2 || cosr < (P.inertial ? TRI_COS_9996 : TRI_COS_9998))) {
            float A[4][4], h[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float t10 = c < 3 ? V1.rcw[c] : V1.tcw[0], t11 = c < 3 ? V1.rcw[3 + c] : V1.tcw[1], t12 = c < 3 ? V1.rcw[6 + c] : V1.tcw[2];
                const float t20 = c < 3 ? V2.rcw[c] : V2.tcw[0], t21 = c < 3 ? V2.rcw[3 + c] : V2.tcw[1], t22 = c < 3 ? V2.rcw[6 + c] : V2.tcw[2];
                A[0][c] = a1 * t12 - t10; A[1][c] = b1 * t12 - t11;
                A[2][c] = a2 * t22 - t20; A[3][c] = b2 * t22 - t21;
            }
            jacobi_null4<TRI_SWEEPS>(A, h);
            code = 4;
            if (h[3] == 0.f) break;
            X = h[0] / h[3]; Y = h[1] / h[3]; Z = h[2] / h[3];
        } else if (st1 && cs1 < cs2) {
            point_stereo = true;
            const float z = dep1[i];
            code = 6;
            if (!(z > 0.f)) break;
            const float* raw = kraw1 ? kraw1 : kpts1;
            tri_unproject(V1, raw[2 * i], raw[2 * i + 1], z, X, Y, Z);
        } else if (st2 && cs2 < cs1) {
            point_stereo = true;
            const float z = dep2[f2];
            code = 6;
            if (!(z > 0.f)) break;
            const float* raw = kraw2 ? kraw2 : kpts2;
            tri_unproject(V2, raw[2 * f2], raw[2 * f2 + 1], z, X, Y, Z);
        } else {
            code = 5;
            break;
        }
        const float z1 = tri_dot3(V1.rcw[6], V1.rcw[7], V1.rcw[8], X, Y, Z) + V1.tcw[2];
        code = 7;
        if (z1 <= 0.f) break;
        const float z2 = tri_dot3(V2.rcw[6], V2.rcw[7], V2.rcw[8], X, Y, Z) + V2.tcw[2];
        code = 8;
        if (z2 <= 0.f) break;
        const int o1 = oct1[i], o2 = oct2[f2];
        code = st1 ? 10 : 9;
        if (tri_reproj_fails(V1, X, Y, Z, z1, k1x, k1y, kp1_ur, st1, V1.mbf, level_table(P.level_sigma2, o1))) break;
        code = st2 ? 12 : 11;
        if (tri_reproj_fails(V2, X, Y, Z, z2, k2x, k2y, kp2_ur, st2, V1.mbf, level_table(P.level_sigma2, o2))) break;
        const float dist1 = tri_norm3(X - V1.ow[0], Y - V1.ow[1], Z - V1.ow[2]);
        const float dist2 = tri_norm3(X - V2.ow[0], Y - V2.ow[1], Z - V2.ow[2]);
        code = 13;
        if (dist1 == 0.f || dist2 == 0.f) break;
        code = 14;
        if (P.far_points && (dist1 >= P.th_far || dist2 >= P.th_far)) break;
        const float ratio_dist = dist2 / dist1;
        const float ratio_octave = level_table(P.scale_factors, o1) / level_table(P.scale_factors, o2);
        code = 15;
        if (ratio_dist * P.ratio_factor < ratio_octave || ratio_dist > ratio_octave * P.ratio_factor) break;
        code = 0;
    } while (false);
    wcode[slot] = code;
    wx3d[3 * slot] = X; wx3d[3 * slot + 1] = Y; wx3d[3 * slot + 2] = Z;
    wstereo[slot] = point_stereo;
    if (code == 0) atomicMin(&claim[i], n);
}

__global__ __launch_bounds__(256) void tri_resolve_kernel(const int32_t* __restrict__ pairs, int Kmax, int32_t* __restrict__ wcode,
                                                          const float* __restrict__ wx3d, const uint8_t* __restrict__ wstereo,
                                                          const int32_t* __restrict__ claim, int32_t* __restrict__ count,
                                                          int32_t* __restrict__ code_out, float* __restrict__ x3d_out,
                                                          uint8_t* __restrict__ stereo_out, int32_t* __restrict__ stats) {
    const int n = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const size_t slot = (size_t)n * Kmax + k;
    int code = -1;
    bool stereo = false, attempt = false, finite = true;
    if (k < Kmax) {
        code = wcode[slot];
        stereo = wstereo[slot] != 0;
        const float X = wx3d[3 * slot], Y = wx3d[3 * slot + 1], Z = wx3d[3 * slot + 2];
        if (code >= 0 && (code == 0 || code >= 4)) {                     // the slot read its indices and found them in range
            const int owner = claim[pairs[2 * slot]];
            if (code == 0 && owner != n) wcode[slot] = code = TRI_CLAIMED;
            attempt = stereo && !(owner < n);                            // the reference never looks at a feature an earlier neighbour took
        }
        finite = (X - X == 0.f) && (Y - Y == 0.f) && (Z - Z == 0.f);
        if (code_out) code_out[slot] = code;
        if (x3d_out) { x3d_out[3 * slot] = X; x3d_out[3 * slot + 1] = Y; x3d_out[3 * slot + 2] = Z; }
        if (stereo_out) stereo_out[slot] = stereo;
    }
    const unsigned long long created = __ballot(code == 0), existing = __ballot(code == 3), cstereo = __ballot(code == 0 && stereo),
                             att = __ballot(attempt), nonfin = __ballot(code == 0 && !finite);
    if ((threadIdx.x & 63) == 0) {
        if (created) { atomicAdd(&count[n], (int)__popcll(created)); atomicAdd(&stats[0], (int)__popcll(created)); }
        if (existing) atomicAdd(&stats[2], (int)__popcll(existing));
        if (cstereo) atomicAdd(&stats[3], (int)__popcll(cstereo));
        if (att) atomicAdd(&stats[4], (int)__popcll(att));
        if (nonfin) atomicAdd(&stats[5], (int)__popcll(nonfin));
    }
}

// one workgroup per neighbour.  count [Nn <= 64]: the winners of every neighbour; cap: room in the out_* arrays
__global__ __launch_bounds__(256) void tri_compact_kernel(const int32_t* __restrict__ S, const uint8_t* __restrict__ nvalid,
                                                          const int32_t* __restrict__ pairs, int Nn, int Kmax, const int32_t* __restrict__ wcode,
                                                          const float* __restrict__ wx3d, const uint8_t* __restrict__ wstereo,
                                                          const int32_t* __restrict__ count, int cap, int32_t* __restrict__ out_n,
                                                          int32_t* __restrict__ out_idx1, int32_t* __restrict__ out_idx2,
                                                          float* __restrict__ out_x3d, uint8_t* __restrict__ out_stereo,
                                                          int32_t* __restrict__ matches, int32_t* __restrict__ stats) {
    __shared__ int s_base, s_wave[4];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave == 0) {                                                     // exclusive prefix over the neighbours in front of this one
        int v = lane < n ? count[lane] : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0) {
            s_base = v;
            const int s = (!nvalid || nvalid[n]) ? min(max(S[n], 0), Kmax) : 0;
            if (matches) matches[n] = s;
            if (s) atomicAdd(&stats[1], s);
        }
    }
    __syncthreads();
    int base = s_base;
    for (int k0 = 0; k0 < Kmax; k0 += 256) {
        const int k = k0 + tid;
        const size_t slot = (size_t)n * Kmax + k;
        const bool win = k < Kmax && wcode[slot] == 0;
        const unsigned long long b = __ballot(win);
        if (lane == 0) s_wave[wave] = (int)__popcll(b);
        __syncthreads();
        int pos = base + (int)__popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += s_wave[w];
        if (win && pos < cap) {
            if (out_n) out_n[pos] = n;
            if (out_idx1) out_idx1[pos] = pairs[2 * slot];
            if (out_idx2) out_idx2[pos] = pairs[2 * slot + 1];
            if (out_x3d) { out_x3d[3 * pos] = wx3d[3 * slot]; out_x3d[3 * pos + 1] = wx3d[3 * slot + 1]; out_x3d[3 * pos + 2] = wx3d[3 * slot + 2]; }
            if (out_stereo) out_stereo[pos] = wstereo[slot];
        }
        base += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        __syncthreads();
    }
}

void launch_tri_eval(hipStream_t s, const rfe_tri_params& P, const rfe_tri_view& V1, const float* kpts1, const float* kraw1, const int32_t* oct1,
                     const float* ur1, const float* dep1, const uint8_t* mp1, int N1, const rfe_tri_view* views2, const float* kpts2,
                     const float* kraw2, const int32_t* oct2, const float* ur2, const float* dep2, const uint8_t* mp2, const int32_t* n2,
                     const uint8_t* nvalid, int Nn, int N2max, const int32_t* S, const int32_t* pairs, int Kmax, int32_t* wcode, float* wx3d,
                     uint8_t* wstereo, int32_t* claim) {
    if (Nn <= 0 || Kmax <= 0) return;
    hipLaunchKernelGGL(tri_eval_kernel, dim3((Kmax + 255) / 256, Nn), dim3(256), 0, s, P, V1, kpts1, kraw1, oct1, ur1, dep1, mp1, N1, views2, kpts2,
                       kraw2, oct2, ur2, dep2, mp2, n2, nvalid, N2max, S, pairs, Kmax, wcode, wx3d, wstereo, claim);
}

void launch_tri_resolve(hipStream_t s, const int32_t* S, const uint8_t* nvalid, const int32_t* pairs, int N1, int Nn, int Kmax, int32_t* wcode,
                        const float* wx3d, const uint8_t* wstereo, const int32_t* claim, int32_t* count, int32_t* code, float* x3d,
                        uint8_t* point_stereo, int32_t* out_n, int32_t* out_idx1, int32_t* out_idx2, float* out_x3d, uint8_t* out_stereo,
                        int32_t* matches, int32_t* stats) {
    if (Nn <= 0) return;
    if (Kmax > 0)
        hipLaunchKernelGGL(tri_resolve_kernel, dim3((Kmax + 255) / 256, Nn), dim3(256), 0, s, pairs, Kmax, wcode, wx3d, wstereo, claim, count, code,
                           x3d, point_stereo, stats);
    hipLaunchKernelGGL(tri_compact_kernel, dim3(Nn), dim3(256), 0, s, S, nvalid, pairs, Nn, Kmax, wcode, wx3d, wstereo, count, N1, out_n, out_idx1,
                       out_idx2, out_x3d, out_stereo, matches, stats);
}

}  // namespace rfe
