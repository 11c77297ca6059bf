// tile_ldlt.h -- the left-looking tiled LDLT essential_graph.hip (DESIGN.md 6m, 28 x 28 tiles) and global_ba.hip (6n, 24 x 24) share:
// one launch per tile column, one workgroup per non-zero tile of the column; each thread owns its entries and subtracts
// L_ik (L_jk d_k) in ascending k, so the bits are those of the dense per-entry order whatever the tile side.  A tile the fill leaves
// out is structurally zero and is skipped (6m(g)).  The forward substitution rides in the column launches, the backward one takes one
// launch per tile row.  Everything is double, one rounding per operation.
#pragma once
#include "lm_device.h"

namespace rfe {

// mat [NP, NP]: H in the upper triangle with the diagonal, L strictly below; fill [NT, NT]; per tile column its non-zero tiles, the
// diagonal first, per tile row likewise; z the right-hand side (consumed), y / xs the substitutions, dvec the pivots; *fail is or-ed
struct TileLdlt {
    double *mat, *dvec, *z, *y, *xs;
    const uint8_t* fill;
    const int32_t *col_start, *col_tiles, *row_start, *row_tiles;
    int NT, NP;
    int32_t* fail;
};

// tile column J: workgroup w takes the column's w-th non-zero tile I (the diagonal tile first).  Every workgroup forms the diagonal
// tile's update and factor for itself -- the same operations on the same numbers -- and its own tile next to it; only the diagonal
// tile's workgroup stores d, the diagonal tile's L and the finished z of the column.  LM_LANES threads
template <int T>
__device__ __forceinline__ void tl_column(const TileLdlt& d, int J, double lambda) {
    constexpr int TT = T * T, M = (TT + LM_LANES - 1) / LM_LANES;
    __shared__ double sD[T][T + 1], sO[T][T + 1], sLJ[T][T + 1], sWJ[T][T + 1], sLI[T][T + 1];
    __shared__ double sd[T], sz[T];
    __shared__ int bad;
    const int lane = threadIdx.x, NT = d.NT;
    const size_t NP = d.NP;
    const int I = d.col_tiles[d.col_start[J] + blockIdx.x];
    const bool own = I != J;
    const size_t rJ = (size_t)J * T, rI = (size_t)I * T;
    if (lane == 0) bad = 0;
    double vD[M], vO[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int idx = lane + LM_LANES * m, r = idx / T, c = idx % T;
        vD[m] = 0.0; vO[m] = 0.0;
        if (idx < TT) {
            if (r >= c) { vD[m] = d.mat[(rJ + c) * NP + rJ + r]; if (r == c) vD[m] = vD[m] + lambda; }
            if (own) vO[m] = d.mat[(rJ + c) * NP + rI + r];
        }
    }
    for (int K = 0; K < J; ++K) {
        if (!d.fill[J * NT + K]) continue;
        const bool hasI = own && d.fill[I * NT + K];
        const size_t cK = (size_t)K * T;
        __syncthreads();
        for (int idx = lane; idx < TT; idx += LM_LANES) {
            const int r = idx / T, k = idx % T;
            const double l = d.mat[(rJ + r) * NP + cK + k];
            sLJ[r][k] = l; sWJ[r][k] = l * d.dvec[cK + k];
            if (hasI) sLI[r][k] = d.mat[(rI + r) * NP + cK + k];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int idx = lane + LM_LANES * m, r = idx / T, c = idx % T;
            if (idx >= TT) continue;
            if (r >= c)
                for (int k = 0; k < T; ++k) vD[m] = vD[m] - sLJ[r][k] * sWJ[c][k];
            if (hasI)
                for (int k = 0; k < T; ++k) vO[m] = vO[m] - sLI[r][k] * sWJ[c][k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int idx = lane + LM_LANES * m, r = idx / T, c = idx % T;
        if (idx < TT) { sD[r][c] = vD[m]; sO[r][c] = vO[m]; }
    }
    if (lane < T) sz[lane] = d.z[rJ + lane];
    __syncthreads();
    // the diagonal tile, right-looking inside the tile: entry (r, c') still subtracts in ascending k
    for (int c = 0; c < T; ++c) {
        const double dc = sD[c][c];
        if (lane == 0) sd[c] = dc;
        if (lane > c && lane < T) sD[lane][c] = sD[lane][c] / dc;
        __syncthreads();
        for (int idx = lane; idx < TT; idx += LM_LANES) {
            const int r = idx / T, c2 = idx % T;
            if (c2 > c && r >= c2) sD[r][c2] = sD[r][c2] - sD[r][c] * (sD[c2][c] * dc);
        }
        __syncthreads();
    }
    // the own tile's rows against the diagonal tile, one thread per row
    if (own && lane < T) {
        const int r = lane;
        for (int c = 0; c < T; ++c) {
            double v = sO[r][c];
            for (int k = 0; k < c; ++k) v = v - sO[r][k] * (sD[c][k] * sd[k]);
            sO[r][c] = v / sd[c];
        }
    }
    // forward substitution: the column's z, then its share of the own tile's rows
    for (int k = 0; k < T; ++k) {
        __syncthreads();
        if (lane > k && lane < T) sz[lane] = sz[lane] - sD[lane][k] * sz[k];
    }
    __syncthreads();
    int nf = 0;
    if (own) {
        if (lane < T) {
            double zi = d.z[rI + lane];
            for (int k = 0; k < T; ++k) zi = zi - sO[lane][k] * sz[k];
            d.z[rI + lane] = zi;
        }
        for (int idx = lane; idx < TT; idx += LM_LANES) {
            const int r = idx / T, c = idx % T;
            const double l = sO[r][c];
            d.mat[(rI + r) * NP + rJ + c] = l;
            if (!isfinite(l)) nf = 1;
        }
    } else {
        for (int idx = lane; idx < TT; idx += LM_LANES) {
            const int r = idx / T, c = idx % T;
            if (r > c) {
                const double l = sD[r][c];
                d.mat[(rJ + r) * NP + rJ + c] = l;
                if (!isfinite(l)) nf = 1;
            }
        }
        if (lane < T) {
            const double p = sd[lane];
            d.dvec[rJ + lane] = p;
            d.y[rJ + lane] = sz[lane];
            if (!isfinite(p) || p == 0.0) nf = 1;
        }
    }
    if (nf) atomicOr(&bad, 1);
    __syncthreads();
    if (lane == 0 && bad) atomicOr(d.fail, 1);
}

// tile row J of the backward substitution, J descending over the launches: workgroup w takes the row's w-th non-zero tile K (the
// diagonal first).  Every workgroup finishes the row's y for itself; the diagonal's stores it (to xs, the others still read y).  64 threads
template <int T>
__device__ __forceinline__ void tl_backward(const TileLdlt& d, int J) {
    __shared__ double sy[T];
    const int lane = threadIdx.x;
    const size_t NP = d.NP, rJ = (size_t)J * T;
    const int K = d.row_tiles[d.row_start[J] + blockIdx.x];
    if (lane < T) sy[lane] = d.y[rJ + lane];
    for (int k = T - 1; k >= 1; --k) {
        __syncthreads();
        if (lane < k) sy[lane] = sy[lane] - d.mat[(rJ + k) * NP + rJ + lane] * sy[k];
    }
    __syncthreads();
    if (lane >= T) return;
    if (K == J) { d.xs[rJ + lane] = sy[lane]; return; }
    const size_t i = (size_t)K * T + lane;
    double yi = d.y[i];
    for (int k = T - 1; k >= 0; --k) yi = yi - d.mat[(rJ + k) * NP + i] * sy[k];
    d.y[i] = yi;
}

}  // namespace rfe
