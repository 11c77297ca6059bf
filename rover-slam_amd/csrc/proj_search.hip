// proj_search.hip -- SPmatcher::SearchByProjection1 (left-camera branch, src/Matchers/SPmatcher.cc:1190-1283) for all map points of a
// frame at once, device resident from the feature grid to F.mvpMapPoints:
//   * proj_grid_kernel:    Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:488-523, 998-1014): 32 x 24 cells, roundf, features
//                          ascending inside a cell.  Cells are numbered ix * 24 + iy, so the cells (ix, cy0..cy1) of a search window are ONE
//                          contiguous run of cell_items, already in GetFeaturesInArea's visiting order (ix outer, iy inner, index ascending).
//   * proj_count_kernel:   Frame::GetFeaturesInArea (src/Frame.cc:895-987) per map point against the grid held in LDS: count, exclusive scan
//                          over the map points, then the same walk again writing the candidate indices in scan order.
//   * proj_fill_kernel:    the hot path -- one wave per map point, DescriptorDistance_sp (desc_dist_wave, rfe_internal.h) of every candidate,
//                          PS_INFLIGHT candidate rows loaded before the first one is reduced (the loop is latency bound).
//   * proj_resolve_kernel: the reference's sequential greedy assignment as a fixpoint of parallel rescans of the stored (index, distance)
//                          lists; no descriptor is read here.
// A feature with skip set stays in the lists (the candidate total is GetFeaturesInArea's) with distance +inf: it never beats 256.
#include <limits.h>
#include "rfe_internal.h"

namespace rfe {

constexpr int PS_COLS = 32, PS_ROWS = 24, PS_CELLS = PS_COLS * PS_ROWS;   // FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h:49-50)
constexpr int PS_MAX_F = 4096, PS_MAX_Q = 16384;
constexpr int PS_INFLIGHT = 8;

// ---------------------------------------------------------------- 1. grid
// one workgroup.  cell_start [PS_CELLS + 2]: exclusive scan of the cell populations, [PS_CELLS] = features inside the grid,
// [PS_CELLS + 1] = the feature count used (min(*nf_dev, Nf)); cell_items [Nf]; fxy [Nf]: the positions as float (kxy converted).
__global__ __launch_bounds__(1024) void proj_grid_kernel(const float* __restrict__ kpts, const int32_t* __restrict__ kxy, int Nf,
                                                         const int32_t* __restrict__ nf_dev, float min_x, float min_y, float inv_w,
                                                         float inv_h, int32_t* __restrict__ cell_start, int32_t* __restrict__ cell_items,
                                                         float2* __restrict__ fxy) {
    __shared__ __attribute__((aligned(16))) uint16_t cell[PS_MAX_F];
    __shared__ int cnt[1024];
    __shared__ int start[1024];
    const int tid = threadIdx.x;
    int nf = Nf;
    if (nf_dev) { const int v = *nf_dev; nf = v < 0 ? 0 : (v < Nf ? v : Nf); }
    cnt[tid] = 0;
    __syncthreads();
    for (int f = tid; f < PS_MAX_F; f += 1024) {
        int c = 0xFFFF;
        if (f < nf) {
            float x, y;
            if (kpts) { x = kpts[2 * f]; y = kpts[2 * f + 1]; }
            else { x = (float)kxy[2 * f]; y = (float)kxy[2 * f + 1]; }
            fxy[f] = make_float2(x, y);
            const float gx = roundf((x - min_x) * inv_w), gy = roundf((y - min_y) * inv_h);   // half away from zero, as PosInGrid
            if (gx >= 0.f && gx < (float)PS_COLS && gy >= 0.f && gy < (float)PS_ROWS) {       // NaN fails every comparison
                c = (int)gx * PS_ROWS + (int)gy;
                atomicAdd(&cnt[c], 1);
            }
        }
        cell[f] = (uint16_t)c;
    }
    __syncthreads();
    // exclusive scan of cnt[0, 1024) (entries >= PS_CELLS are zero)
    const int mine = cnt[tid];
    start[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? start[tid - off] : 0;
        __syncthreads();
        start[tid] += v;
        __syncthreads();
    }
    const int s0 = start[tid] - mine;
    if (tid <= PS_CELLS) cell_start[tid] = s0;
    if (tid == 0) cell_start[PS_CELLS + 1] = nf;
    // stable scatter: the thread of a cell walks the cell numbers in feature order (eight per LDS read) until it has its population
    if (tid < PS_CELLS && mine > 0) {
        int k = 0;
        const uint4* c8 = reinterpret_cast<const uint4*>(cell);
        for (int g = 0; g < nf && k < mine; g += 8) {
            const uint4 v = c8[g >> 3];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((int)(w[j] & 0xFFFFu) == tid) cell_items[s0 + k++] = g + 2 * j;
                if ((int)(w[j] >> 16) == tid) cell_items[s0 + k++] = g + 2 * j + 1;
            }
        }
    }
}

// ---------------------------------------------------------------- 2. count
struct PsWindow { int x0, x1, y0, y1; bool any; };

// one axis of GetFeaturesInArea's cell window; clamped in float, so no out-of-range value reaches a float -> int conversion
__device__ __forceinline__ bool ps_axis(float p, float mn, float r, float inv, int ncell, int& c0, int& c1) {
    const float lo = floorf((p - mn - r) * inv), hi = ceilf((p - mn + r) * inv);
    if (!(lo < (float)ncell) || !(hi >= 0.f)) return false;
    c0 = lo > 0.f ? (int)lo : 0;
    c1 = hi < (float)(ncell - 1) ? (int)hi : ncell - 1;
    return true;
}

__device__ __forceinline__ int ps_walk(const PsWindow& w, float px, float py, float r, int L, const int* cs, const uint16_t* items,
                                       const float2* xy, const int8_t* oc, int32_t* out) {
    int n = 0;
    if (!w.any) return 0;
    for (int ix = w.x0; ix <= w.x1; ++ix) {
        const int e = cs[ix * PS_ROWS + w.y1 + 1];
        for (int k = cs[ix * PS_ROWS + w.y0]; k < e; ++k) {
            const int f = items[k];
            const int o = oc[f];
            if (o < L - 1 || o > L) continue;
            const float2 p = xy[f];
            if (fabsf(p.x - px) < r && fabsf(p.y - py) < r) {
                if (out) out[n] = f;
                ++n;
            }
        }
    }
    return n;
}

__device__ __forceinline__ PsWindow ps_window(const float* proj, const float* radius, const int32_t* pred_level, int i, float min_x,
                                              float min_y, float inv_w, float inv_h, float& px, float& py, float& r, int& L) {
    PsWindow w;
    px = proj[2 * i]; py = proj[2 * i + 1]; r = radius[i];
    L = pred_level ? pred_level[i] : 0;
    w.x0 = w.x1 = w.y0 = w.y1 = 0;
    w.any = L >= 0 && L < RFE_MAX_LEVELS && isfinite(px) && isfinite(py) && isfinite(r);
    if (w.any) w.any = ps_axis(px, min_x, r, inv_w, PS_COLS, w.x0, w.x1) && ps_axis(py, min_y, r, inv_h, PS_ROWS, w.y0, w.y1) && w.y0 <= w.y1;
    return w;
}

// one workgroup; the grid (about 50 KB) is staged into LDS once and walked twice.  seg_off [Nq + 1]; stats[1] = candidates needed,
// stats[3] = 1 when that exceeds cand_cap -- every list is then left empty and nothing is written to cand_idx.
__global__ __launch_bounds__(1024) void proj_count_kernel(const float* __restrict__ proj, const float* __restrict__ radius,
                                                          const int32_t* __restrict__ pred_level, int Nq,
                                                          const int32_t* __restrict__ cell_start, const int32_t* __restrict__ cell_items,
                                                          const float2* __restrict__ fxy, const int32_t* __restrict__ octave, float min_x,
                                                          float min_y, float inv_w, float inv_h, int cand_cap, int32_t* __restrict__ seg_off,
                                                          int32_t* __restrict__ cand_idx, int32_t* __restrict__ stats) {
    __shared__ float2 xy[PS_MAX_F];
    __shared__ int cs[PS_CELLS + 1];
    __shared__ uint16_t items[PS_MAX_F];
    __shared__ int8_t oc[PS_MAX_F];
    __shared__ int sc[1024];
    const int tid = threadIdx.x;
    int nf = cell_start[PS_CELLS + 1];
    nf = nf < 0 ? 0 : (nf < PS_MAX_F ? nf : PS_MAX_F);
    int nin = cell_start[PS_CELLS];
    nin = nin < 0 ? 0 : (nin < nf ? nin : nf);
    if (tid <= PS_CELLS) { const int v = cell_start[tid]; cs[tid] = v < 0 ? 0 : (v < nin ? v : nin); }
    for (int f = tid; f < nf; f += 1024) {
        xy[f] = fxy[f];
        const int o = octave ? octave[f] : 0;
        oc[f] = (int8_t)(o < -100 ? -100 : (o > 100 ? 100 : o));     // the gate compares with levels 0..RFE_MAX_LEVELS-1 only
    }
    for (int k = tid; k < nin; k += 1024) { const int f = cell_items[k]; items[k] = (uint16_t)((unsigned)f < (unsigned)nf ? f : 0); }
    __syncthreads();
    const int per = (Nq + 1023) / 1024;
    const int i0 = tid * per, i1 = (i0 + per < Nq) ? i0 + per : Nq;
    int sum = 0;
    for (int i = i0; i < i1; ++i) {
        float px, py, r; int L;
        const PsWindow w = ps_window(proj, radius, pred_level, i, min_x, min_y, inv_w, inv_h, px, py, r, L);
        const int n = ps_walk(w, px, py, r, L, cs, items, xy, oc, nullptr);
        seg_off[i] = n;
        sum += n;
    }
    sc[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? sc[tid - off] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    const int total = sc[1023];
    const bool overflow = total > cand_cap;
    int run = overflow ? 0 : sc[tid] - sum;
    for (int i = i0; i < i1; ++i) {
        const int n = seg_off[i];          // this thread's own store above
        seg_off[i] = run;
        if (!overflow && n > 0) {
            float px, py, r; int L;
            const PsWindow w = ps_window(proj, radius, pred_level, i, min_x, min_y, inv_w, inv_h, px, py, r, L);
            ps_walk(w, px, py, r, L, cs, items, xy, oc, cand_idx + run);
            run += n;
        }
    }
    if (tid == 0) { seg_off[Nq] = overflow ? 0 : total; stats[1] = total; stats[3] = overflow ? 1 : 0; }
}

// ---------------------------------------------------------------- 3. fill + distance
// TRUNC: the `int dist = DescriptorDistance_sp(...)` of the second Sim3 SearchByProjection overload (SPmatcher.cc:2164): the
// distance is truncated toward zero once, where it is stored, and the resolve kernel's strict < keeps the first least one as the loop does.
template <bool TRUNC>
__global__ __launch_bounds__(256) void proj_fill_kernel(const float* __restrict__ q, int Nq, const float* __restrict__ f, int Nf,
                                                        const int32_t* __restrict__ seg_off, const int32_t* __restrict__ cand_idx,
                                                        const uint8_t* __restrict__ skip, float* __restrict__ cand_dist) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Nq) return;
    const int s = seg_off[i], e = seg_off[i + 1];
    if (e <= s) return;
    const float4 a = reinterpret_cast<const float4*>(q + (size_t)i * 256)[lane];
    for (int c = s; c < e; c += PS_INFLIGHT) {
        float4 b[PS_INFLIGHT];
        bool live[PS_INFLIGHT];
#pragma unroll
        for (int j = 0; j < PS_INFLIGHT; ++j) {
            const int idx = c + j < e ? cand_idx[c + j] : -1;
            live[j] = (unsigned)idx < (unsigned)Nf && !(skip && skip[idx]);
            b[j] = live[j] ? reinterpret_cast<const float4*>(f + (size_t)idx * 256)[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < PS_INFLIGHT; ++j) {
            if (c + j >= e) break;                       // wave-uniform
            const float d = live[j] ? desc_dist_wave(a, b[j]) : __builtin_inff();
            if (lane == 0) cand_dist[c + j] = TRUNC ? truncf(d) : d;
        }
    }
}

// ---------------------------------------------------------------- 4. resolve
// best / second-best scan of one stored list; feature fi is blocked for map point i when an observed accepted map point k < i holds it
__device__ __forceinline__ void ps_scan(const int32_t* __restrict__ cand_idx, const float* __restrict__ cand_dist, int s, int e,
                                        const int* minw, int i, int& bi, float& bd, float& sd) {
    bi = -1; bd = 256.f; sd = 256.f;
    for (int c = s; c < e; ++c) {
        const int fi = cand_idx[c];
        const float d = cand_dist[c];
        if ((unsigned)fi >= (unsigned)PS_MAX_F || minw[fi] < i) continue;
        if (d < bd) { sd = bd; bd = d; bi = fi; }
        else if (d < sd) sd = d;
    }
}

__global__ __launch_bounds__(1024) void proj_resolve_kernel(const int32_t* __restrict__ seg_off, const int32_t* __restrict__ cand_idx,
                                                            const float* __restrict__ cand_dist, const uint8_t* __restrict__ observed,
                                                            int Nq, int Nf, float th_high, int32_t* __restrict__ assign,
                                                            int32_t* __restrict__ best_idx, float* __restrict__ best_dist,
                                                            float* __restrict__ second_dist, int32_t* __restrict__ stats) {
    __shared__ int16_t pick[PS_MAX_Q];     // the ACCEPTED feature of each map point, -1 = none
    __shared__ int minw[PS_MAX_F];         // least observed accepted map point per feature; the greatest accepted one after the loop
    __shared__ int changed, nacc;
    const int tid = threadIdx.x;
    for (int fi = tid; fi < PS_MAX_F; fi += 1024) minw[fi] = INT_MAX;
    for (int i = tid; i < Nq; i += 1024) pick[i] = -1;
    if (tid == 0) nacc = 0;
    int rounds = 0;
    for (;;) {
        if (tid == 0) changed = 0;
        __syncthreads();
        bool ch = false;
        for (int i = tid; i < Nq; i += 1024) {
            int bi; float bd, sd;
            ps_scan(cand_idx, cand_dist, seg_off[i], seg_off[i + 1], minw, i, bi, bd, sd);
            const int acc = bd <= th_high ? bi : -1;
            if (acc != pick[i]) { pick[i] = (int16_t)acc; ch = true; }
        }
        if (ch) changed = 1;
        ++rounds;
        __syncthreads();
        if (!changed || rounds > Nq + 1) break;          // uniform: every thread reads the same LDS word behind the barrier
        for (int fi = tid; fi < PS_MAX_F; fi += 1024) minw[fi] = INT_MAX;
        __syncthreads();
        for (int i = tid; i < Nq; i += 1024)
            if (pick[i] >= 0 && (!observed || observed[i])) atomicMin(&minw[pick[i]], i);
        __syncthreads();
    }
    // the blockers are those of the last round: what every map point sees now is what it saw at its turn in the sequence
    int mine = 0;
    for (int i = tid; i < Nq; i += 1024) {
        int bi; float bd, sd;
        ps_scan(cand_idx, cand_dist, seg_off[i], seg_off[i + 1], minw, i, bi, bd, sd);
        if (best_idx) best_idx[i] = bi;
        if (best_dist) best_dist[i] = bd;
        if (second_dist) second_dist[i] = sd;
        if (pick[i] >= 0) ++mine;
    }
    if (mine) atomicAdd(&nacc, mine);
    __syncthreads();
    for (int fi = tid; fi < PS_MAX_F; fi += 1024) minw[fi] = -1;
    __syncthreads();
    for (int i = tid; i < Nq; i += 1024)
        if (pick[i] >= 0) atomicMax(&minw[pick[i]], i);   // F.mvpMapPoints[bestIdx] = pMP: the last writer stays
    __syncthreads();
    for (int fi = tid; fi < Nf; fi += 1024) assign[fi] = fi < PS_MAX_F ? minw[fi] : -1;
    if (tid == 0) { stats[0] = nacc; stats[2] = rounds; }
}

void launch_proj_grid(hipStream_t s, const float* kpts, const int32_t* kxy, int Nf, const int32_t* nf_dev, float min_x, float min_y,
                      float inv_w, float inv_h, int32_t* cell_start, int32_t* cell_items, float* fxy) {
    hipLaunchKernelGGL(proj_grid_kernel, dim3(1), dim3(1024), 0, s, kpts, kxy, Nf, nf_dev, min_x, min_y, inv_w, inv_h, cell_start,
                       cell_items, reinterpret_cast<float2*>(fxy));
}

void launch_proj_count(hipStream_t s, const float* proj, const float* radius, const int32_t* pred_level, int Nq, const int32_t* cell_start,
                       const int32_t* cell_items, const float* fxy, const int32_t* octave, float min_x, float min_y, float inv_w,
                       float inv_h, int cand_cap, int32_t* seg_off, int32_t* cand_idx, int32_t* stats) {
    hipLaunchKernelGGL(proj_count_kernel, dim3(1), dim3(1024), 0, s, proj, radius, pred_level, Nq, cell_start, cell_items,
                       reinterpret_cast<const float2*>(fxy), octave, min_x, min_y, inv_w, inv_h, cand_cap, seg_off, cand_idx, stats);
}

void launch_proj_fill(hipStream_t s, const float* q, int Nq, const float* f, int Nf, const int32_t* seg_off, const int32_t* cand_idx,
                      const uint8_t* skip, float* cand_dist) {
    if (Nq <= 0 || Nf <= 0) return;
    hipLaunchKernelGGL(proj_fill_kernel<false>, dim3((Nq + 3) / 4), dim3(256), 0, s, q, Nq, f, Nf, seg_off, cand_idx, skip, cand_dist);
}

void launch_proj_fill_trunc(hipStream_t s, const float* q, int Nq, const float* f, int Nf, const int32_t* seg_off, const int32_t* cand_idx,
                            const uint8_t* skip, float* cand_dist) {
    if (Nq <= 0 || Nf <= 0) return;
    hipLaunchKernelGGL(proj_fill_kernel<true>, dim3((Nq + 3) / 4), dim3(256), 0, s, q, Nq, f, Nf, seg_off, cand_idx, skip, cand_dist);
}

void launch_proj_resolve(hipStream_t s, const int32_t* seg_off, const int32_t* cand_idx, const float* cand_dist, const uint8_t* observed,
                         int Nq, int Nf, float th_high, int32_t* assign, int32_t* best_idx, float* best_dist, float* second_dist,
                         int32_t* stats) {
    hipLaunchKernelGGL(proj_resolve_kernel, dim3(1), dim3(1024), 0, s, seg_off, cand_idx, cand_dist, observed, Nq, Nf, th_high, assign,
                       best_idx, best_dist, second_dist, stats);
}

}  // namespace rfe
