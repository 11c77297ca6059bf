// pyramid.hip -- the scale pyramid of rfe_extract_pyramid_u8: level geometry and bilinear coefficient tables
// (host, double / float exactly as the contract states them), the resample kernel that builds one level of B frames from the level
// above, and the merge kernel that writes every level's SuperPoint rows into the ORB-SLAM layout (level order, level-0 pixels, octave).
#include <math.h>
#include "rfe_internal.h"

namespace rfe {

// s_0 = 1, s_l = (float)((double)s_{l-1} * scale_factor) -- SPextractor's constructor; W_l = lrintf((float)W * (1 / s_l)) -- ComputePyramid's cvRound
int pyramid_geometry(int H, int W, int nlevels, float scale_factor, int32_t* lh, int32_t* lw, float* ls) {
    if (H < 8 || W < 8 || nlevels < 1 || nlevels > RFE_MAX_LEVELS || !lh || !lw || !ls) return RFE_ERR_INVALID;
    if (nlevels > 1 && !(scale_factor > 1.0f && scale_factor <= 4.0f)) return RFE_ERR_INVALID;
    float s = 1.0f;
    bool empty = false;
    for (int l = 0; l < nlevels; ++l) {
        if (l > 0) s = (float)((double)s * (double)scale_factor);
        const float inv = 1.0f / s;
        ls[l] = s;
        lh[l] = (int32_t)lrintf((float)H * inv);
        lw[l] = (int32_t)lrintf((float)W * inv);
        if (lh[l] < 1 || lw[l] < 1) empty = true;
    }
    return empty ? RFE_ERR_INVALID : RFE_OK;
}

// one axis of the resampling rule: source index i0 and the 11-bit weight w1 of i0 + 1, per destination index
static void axis_coeffs(int S, int D, int2* out) {
    const double scale = 1.0 / ((double)D / (double)S);
    for (int d = 0; d < D; ++d) {
        const float f = (float)(((double)d + 0.5) * scale - 0.5);
        const float fl = floorf(f);
        int i0 = (int)fl;
        float t = f - fl;
        if (i0 < 0) { i0 = 0; t = 0.0f; }
        if (i0 >= S - 1) { i0 = S - 1; t = 0.0f; }
        out[d] = make_int2(i0, (int)lrintf(t * 2048.0f));
    }
}

void pyramid_tables(int nlevels, const int32_t* lh, const int32_t* lw, std::vector<int2>& tab, std::vector<size_t>& off) {
    tab.clear();
    off.assign((size_t)nlevels, 0);
    for (int l = 1; l < nlevels; ++l) {
        off[l] = tab.size();
        tab.resize(tab.size() + (size_t)lw[l] + (size_t)lh[l]);
        axis_coeffs(lw[l - 1], lw[l], tab.data() + off[l]);            // columns, then rows
        axis_coeffs(lh[l - 1], lh[l], tab.data() + off[l] + lw[l]);
    }
}

namespace {

constexpr int PYR_THREADS = 256;

// One 16-byte window of the destination plane per lane, aligned in the address space: windows wholly inside the plane are ONE dwordx4
// store, the partial windows at the plane's two ends store byte by byte (a level's plane need not start on 16 bytes: tight pitch).
// Each destination pixel reads source rows y0, y1 and columns x0, x1 of its table entries (weights summing to 2048 per axis), int32
// throughout (2048 * 2048 * 255 < 2^31).  copy != 0: the destination is the source itself (level 0 into the caller's level buffer).
__global__ __launch_bounds__(PYR_THREADS) void pyr_resample_kernel(const uint8_t* __restrict__ src, long long src_frame, int src_stride, int Hs,
                                                                   int Ws, uint8_t* __restrict__ dst, long long dst_frame, int Hd, int Wd,
                                                                   const int2* __restrict__ cx, const int2* __restrict__ cy, int copy) {
    const int b = blockIdx.y;
    const uint8_t* S = src + (long long)b * src_frame;
    uint8_t* base = dst + (long long)b * dst_frame;
    const long long plane = (long long)Hd * Wd;
    const uintptr_t first = (uintptr_t)base & ~(uintptr_t)15;
    uint8_t* w = (uint8_t*)(first + ((uintptr_t)blockIdx.x * PYR_THREADS + threadIdx.x) * 16);
    const long long i = (long long)(w - base);          // plane index of the window's first byte (negative inside window 0)
    if (i >= plane) return;
    const int j0 = i < 0 ? (int)(-i) : 0;               // the window's bytes [j0, j1) belong to the plane
    const int j1 = plane - i < 16 ? (int)(plane - i) : 16;
    int y = (int)((i + j0) / Wd), x = (int)((i + j0) - (long long)y * Wd);
    unsigned px[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        unsigned v = 0;
        if (j >= j0 && j < j1) {
            if (copy) {
                v = S[(long long)y * src_stride + x];
            } else {
                const int2 ex = cx[x], ey = cy[y];
                const int x1 = min(ex.x + 1, Ws - 1), y1 = min(ey.x + 1, Hs - 1);
                const int a1 = ex.y, a0 = 2048 - a1, b1 = ey.y, b0 = 2048 - b1;
                const uint8_t* r0 = S + (long long)ey.x * src_stride;
                const uint8_t* r1 = S + (long long)y1 * src_stride;
                const int t0 = a0 * (int)r0[ex.x] + a1 * (int)r0[x1];
                const int t1 = a0 * (int)r1[ex.x] + a1 * (int)r1[x1];
                v = (unsigned)((b0 * t0 + b1 * t1 + (1 << 21)) >> 22);
            }
            if (++x == Wd) { x = 0; ++y; }
        }
        px[j] = v;
    }
    if (j0 == 0 && j1 == 16) {
        uint4 q;
        q.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        q.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        q.z = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
        q.w = px[12] | (px[13] << 8) | (px[14] << 16) | (px[15] << 24);
        *(uint4*)w = q;
    } else {
        for (int j = j0; j < j1; ++j) w[j] = (uint8_t)px[j];
    }
}

// Merge: output row r of frame b belongs to the level l with pre_l <= r < pre_l + n_l (pre = prefix of the per-level counts, formed in
// registers from device memory -- the counts never visit the host).  One wave per row: lane 0 writes (x * s_l, y * s_l), octave and score,
// the 64 lanes move the 1 KB descriptor row as 16-byte loads / stores.  Rows past the frame's total are zeroed.
constexpr int MERGE_ROWS = 16;   // rows per workgroup (4 waves x 4)

__global__ __launch_bounds__(256) void pyr_merge_kernel(PyrMergeArgs a) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt[RFE_MAX_LEVELS], pre[RFE_MAX_LEVELS], total = 0;
#pragma unroll
    for (int l = 0; l < RFE_MAX_LEVELS; ++l) {
        cnt[l] = (l < a.L && a.n[l]) ? a.n[l][b] : 0;
        pre[l] = total;
        total += cnt[l];
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) a.n_out[b] = total;
#pragma unroll
        for (int l = 0; l < RFE_MAX_LEVELS; ++l)
            if (a.level_n && l < a.L && threadIdx.x == l + 1) a.level_n[(long long)b * a.L + l] = cnt[l];
    }
    for (int k = wave; k < MERGE_ROWS; k += 4) {
        const int r = blockIdx.x * MERGE_ROWS + k;
        if (r >= a.Ktot) return;
        const long long o = (long long)b * a.Ktot + r;
        float4* dd = (float4*)(a.desc + o * 256) + lane;
        if (r >= total) {
            *dd = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane == 0) { a.kpts[2 * o] = 0.f; a.kpts[2 * o + 1] = 0.f; a.octave[o] = 0; a.score[o] = 0.f; }
            continue;
        }
        const int32_t* kxy = nullptr; const float* sc = nullptr; const float* de = nullptr;
        float s = 1.0f; int lev = 0; long long i = 0;
#pragma unroll
        for (int l = 0; l < RFE_MAX_LEVELS; ++l)
            if (l < a.L && r >= pre[l] && r < pre[l] + cnt[l]) {
                lev = l; s = a.scale[l]; i = (long long)b * a.kmax[l] + (r - pre[l]);
                kxy = a.kxy[l]; sc = a.sc[l]; de = a.desc_l[l];
            }
        *dd = ((const float4*)(de + i * 256))[lane];
        if (lane == 0) {
            a.kpts[2 * o] = (float)kxy[2 * i] * s;
            a.kpts[2 * o + 1] = (float)kxy[2 * i + 1] * s;
            a.octave[o] = lev;
            a.score[o] = sc[i];
        }
    }
}

}  // namespace

void launch_pyr_resample(hipStream_t s, const uint8_t* src, long long src_frame, int src_stride, int Hs, int Ws, uint8_t* dst, long long dst_frame,
                         int Hd, int Wd, int B, const int2* cx, const int2* cy) {
    const bool copy = cx == nullptr;
    long long wins = 0;   // the largest window count over the B frames' planes
    for (int b = 0; b < B; ++b) {
        const uintptr_t p = (uintptr_t)dst + (uintptr_t)((long long)b * dst_frame);
        const long long n = (long long)((p + (uintptr_t)Hd * Wd - (p & ~(uintptr_t)15)) + 15) / 16;
        wins = n > wins ? n : wins;
    }
    const dim3 grid((unsigned)((wins + PYR_THREADS - 1) / PYR_THREADS), (unsigned)B);
    hipLaunchKernelGGL(pyr_resample_kernel, grid, dim3(PYR_THREADS), 0, s, src, src_frame, src_stride, Hs, Ws, dst, dst_frame, Hd, Wd, cx, cy,
                       copy ? 1 : 0);
}

void launch_pyr_merge(hipStream_t s, const PyrMergeArgs& a, int B) {
    const dim3 grid((unsigned)((a.Ktot + MERGE_ROWS - 1) / MERGE_ROWS), (unsigned)B);
    hipLaunchKernelGGL(pyr_merge_kernel, grid, dim3(256), 0, s, a);
}

}  // namespace rfe
