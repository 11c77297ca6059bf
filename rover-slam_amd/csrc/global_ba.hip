// global_ba.hip -- Optimizer::BundleAdjustment behind GlobalBundleAdjustemnt (reference src/Optimizer.cc:2832-3220 over g2o's
// BlockSolver_6_3 and Levenberg-Marquardt), DESIGN.md 6n.  The LM loop is the host's (api_global_ba.hip); every stage here is a plain launch.
//   front       validation, the free keyframes' numbering, the estimates, the per-point edge ranges; then per free edge the count of its
//               pose's list and of the Schur blocks its point's pairs fall in (integer atomics), one workgroup's prefix sums and the list
//               of non-empty blocks, the fill, and one workgroup per list that orders it -- so every list comes out ascending whatever
//               the scheduling, and the work scales with the pairs and the non-empty blocks
//   linearise   6l's: one thread per edge (lba_edge.h, Huber or not), one thread per (vertex, entry) for the sums in edge order
//   trial       6l's Dinv, db, B Dinv, B db and Schur blocks, written into the tiles of a dense matrix; 6m's left-looking tiled LDLT
//               (tile_ldlt.h) over the fill of the covisibility pattern; 6l's back-substitution, update and error pass
// Everything is double, one rounding per operation (-ffp-contract=off); tests/global_ba_ref.py restates it operation by operation.
#include <float.h>
#include "rfe_internal.h"
#include "lm_device.h"
#include "lba_edge.h"
#include "tile_ldlt.h"

namespace rfe {
namespace {

constexpr int GBA_T = 256, T = GBA_TILE, TV = GBA_TILE_V, TT = GBA_TILE * GBA_TILE;
constexpr int GBA_MAX_NT = RFE_GBA_MAX_KF / GBA_TILE_V;
constexpr int GBA_SORT_LDS = 2048;
inline int gba_grid(long long n) { return (int)((n + GBA_T - 1) / GBA_T); }

// ---------------------------------------------------------------- validation: the host reads ctl_i[GBA_I_STATUS] before anything indexes by the tables
__global__ __launch_bounds__(GBA_T) void gba_validate_kernel(GbaDev d) {
    const int t = blockIdx.x * GBA_T + threadIdx.x;
    int bad = 0;
    if (t < d.K) {
        const int nl = d.kf_nlevels[t];
        if (nl < 1 || nl > RFE_MAX_LEVELS) bad |= LBA_BAD_KF;
    }
    if (t <= d.K) {
        const int o = d.kf_feat_off[t];
        if (o < 0 || o > d.Nf) bad |= LBA_BAD_KF;
        if (t < d.K && d.kf_feat_off[t + 1] < o) bad |= LBA_BAD_KF;
    }
    if (t < d.E) {
        const int p = d.edge_point[t], k = d.edge_kf[t], f = d.edge_feat[t];
        if (p < 0 || p >= d.L || k < 0 || k >= d.K) {
            bad |= LBA_BAD_RANGE;
        } else {
            const int o0 = d.kf_feat_off[k], o1 = d.kf_feat_off[k + 1];
            if (f < 0 || o0 < 0 || o1 > d.Nf || f >= o1 - o0) bad |= LBA_BAD_RANGE;
        }
        if (t > 0) {
            const int pp = d.edge_point[t - 1], pk = d.edge_kf[t - 1];
            if (!(pp < p || (pp == p && pk < k))) bad |= LBA_BAD_ORDER;
        }
    }
    if (bad) atomicOr(&d.ctl_i[GBA_I_STATUS], bad);
}

// one workgroup: the free keyframes in ascending index (K <= 1024: four keyframes a lane)
__global__ __launch_bounds__(GBA_T) void gba_number_kernel(GbaDev d) {
    __shared__ int cnt[GBA_T];
    const int lane = threadIdx.x, k0 = 4 * lane;
    int n = 0;
    for (int k = k0; k < k0 + 4 && k < d.K; ++k) n += d.fixed[k] == 0;
    cnt[lane] = n;
    __syncthreads();
    if (lane == 0) {
        int acc = 0;
        for (int i = 0; i < GBA_T; ++i) { const int v = cnt[i]; cnt[i] = acc; acc += v; }
        d.ctl_i[GBA_I_NFREE] = acc;
    }
    __syncthreads();
    int at = cnt[lane];
    for (int k = k0; k < k0 + 4 && k < d.K; ++k) {
        const bool fr = d.fixed[k] == 0;
        d.free_index[k] = fr ? at : -1;
        if (fr) d.free_list[at++] = k;
    }
}

// the estimates and the per-point edge ranges (the binary search reads edge_point only, inside 0 .. E)
__global__ __launch_bounds__(GBA_T) void gba_init_kernel(GbaDev d) {
    const int t = blockIdx.x * GBA_T + threadIdx.x;
    if (t < d.K) {
        double q[7];
        for (int i = 0; i < 7; ++i) q[i] = (double)d.kf_pose[7 * t + i];
        po_normalize(q);
        for (int i = 0; i < 7; ++i) { d.pose[0][7 * t + i] = q[i]; d.pose[1][7 * t + i] = q[i]; }
        d.pose_cnt[t] = 0;
    }
    if (t < d.L)
        for (int i = 0; i < 3; ++i) { const double v = (double)d.xw[3 * (size_t)t + i]; d.pt[0][3 * (size_t)t + i] = v; d.pt[1][3 * (size_t)t + i] = v; }
    if (t <= d.L) {                                   // the first edge whose point is >= t
        int lo = 0, hi = d.E;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (d.edge_point[m] < t) lo = m + 1; else hi = m; }
        d.pt_start[t] = lo;
    }
}

__global__ __launch_bounds__(GBA_T) void gba_zero_kernel(int32_t* p, long long n) {
    const long long t = (long long)blockIdx.x * GBA_T + threadIdx.x;
    if (t < n) p[t] = 0;
}

// ---------------------------------------------------------------- structure front
// one thread per edge on a free keyframe: FILL false counts its pose's list and, for every later free edge of its point (itself first),
// the Schur block (i1 <= i2) the pair falls in; FILL true takes a slot in each list (the counts run back down to zero)
template <bool FILL>
__global__ __launch_bounds__(GBA_T) void gba_pairs_kernel(GbaDev d) {
    const int e = blockIdx.x * GBA_T + threadIdx.x;
    if (e >= d.E) return;
    const int f1 = d.free_index[d.edge_kf[e]];
    if (f1 < 0) return;
    if (FILL) d.pose_list[d.pose_start[f1] + atomicSub(&d.pose_cnt[f1], 1) - 1] = e;
    else atomicAdd(&d.pose_cnt[f1], 1);
    const int end = d.pt_start[d.edge_point[e] + 1];
    for (int e2 = e; e2 < end; ++e2) {
        const int f2 = d.free_index[d.edge_kf[e2]];
        if (f2 < 0) continue;
        const size_t key = (size_t)f1 * d.P + f2;        // f1 <= f2: the point's edges ascend in the keyframe
        if (FILL) d.pairs[(size_t)d.key_start[key] + atomicSub(&d.key_cnt[key], 1) - 1] = ((unsigned long long)e << 32) | (unsigned)e2;
        else atomicAdd(&d.key_cnt[key], 1);
    }
}

// one workgroup: the pose lists' offsets; the offsets of every dense block key and the list of the non-empty blocks (a diagonal block
// is never empty: it holds Hpp + lambda I) in ascending (i1, i2); their number and the number of pairs
__global__ __launch_bounds__(GBA_T) void gba_scan_kernel(GbaDev d) {
    __shared__ int sa[GBA_T], sb[GBA_T];
    __shared__ int tot[2];
    const int lane = threadIdx.x, P = d.P;
    {
        const int per = (P + GBA_T - 1) / GBA_T, i0 = min(lane * per, P), i1 = min(i0 + per, P);
        int s = 0;
        for (int i = i0; i < i1; ++i) s += d.pose_cnt[i];
        sa[lane] = s;
        __syncthreads();
        if (lane == 0) {
            int acc = 0;
            for (int i = 0; i < GBA_T; ++i) { const int v = sa[i]; sa[i] = acc; acc += v; }
            d.pose_start[P] = acc;
        }
        __syncthreads();
        int acc = sa[lane];
        for (int i = i0; i < i1; ++i) { d.pose_start[i] = acc; acc += d.pose_cnt[i]; }
        __syncthreads();
    }
    const long long NK = (long long)P * P, per = (NK + GBA_T - 1) / GBA_T;
    const long long k0 = min((long long)lane * per, NK), k1 = min(k0 + per, NK);
    int s = 0, nb = 0;
    for (long long k = k0; k < k1; ++k) {
        const int c = d.key_cnt[k];
        s += c;
        nb += (c > 0 || k / P == k % P) ? 1 : 0;
    }
    sa[lane] = s; sb[lane] = nb;
    __syncthreads();
    if (lane == 0) {
        int a = 0, b = 0;
        for (int i = 0; i < GBA_T; ++i) { const int va = sa[i], vb = sb[i]; sa[i] = a; sb[i] = b; a += va; b += vb; }
        tot[0] = a; tot[1] = b;
    }
    __syncthreads();
    s = sa[lane]; nb = sb[lane];
    for (long long k = k0; k < k1; ++k) {
        const int c = d.key_cnt[k];
        d.key_start[k] = s;
        if (c > 0 || k / P == k % P) { d.blk_key[nb] = (int)k; d.blk_start[nb] = s; ++nb; }
        s += c;
    }
    if (lane == 0) {
        d.blk_start[tot[1]] = tot[0];
        d.ctl_i[GBA_I_NPAIRS] = tot[0];
        d.ctl_i[GBA_I_NBLOCKS] = tot[1];
    }
}

// sh[0 .. m), m a power of two, ascending: a bitonic network, every thread of the workgroup calls it
template <typename V>
__device__ inline void gba_bitonic(V* sh, int m) {
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += GBA_T) {
                const int l = i ^ j;
                if (l > i) {
                    const V x = sh[i], y = sh[l];
                    if ((x > y) == ((i & k) == 0)) { sh[i] = y; sh[l] = x; }
                }
            }
            __syncthreads();
        }
}

// one workgroup per list: data[start[b] .. start[b + 1]) ascending.  The items of a list are distinct (an edge index; e1 << 32 | e2 with
// one pair per point and block), so the order does not depend on where the atomics put them.  Runs of GBA_SORT_LDS items are sorted in
// LDS behind all-ones padding (V is unsigned); a longer list is merged by rank: an item's place is its place in its own run plus, by
// binary search, the number of smaller items in every other run, and tmp takes the ordered copy
template <typename V>
__global__ __launch_bounds__(GBA_T) void gba_sort_kernel(V* data, V* tmp, const int32_t* start) {
    __shared__ V sh[GBA_SORT_LDS];
    const int lane = threadIdx.x;
    const int s0 = start[blockIdx.x], n = start[blockIdx.x + 1] - s0;
    if (n <= 1) return;
    V* a = data + s0;
    for (int c0 = 0; c0 < n; c0 += GBA_SORT_LDS) {
        const int len = min(GBA_SORT_LDS, n - c0);
        int m = 1;
        while (m < len) m <<= 1;
        __syncthreads();
        for (int i = lane; i < m; i += GBA_T) sh[i] = i < len ? a[c0 + i] : ~(V)0;
        __syncthreads();
        gba_bitonic(sh, m);
        for (int i = lane; i < len; i += GBA_T) a[c0 + i] = sh[i];
    }
    if (n <= GBA_SORT_LDS) return;
    __threadfence_block();
    __syncthreads();
    V* t = tmp + s0;
    for (int i = lane; i < n; i += GBA_T) {
        const V v = a[i];
        const int own = i / GBA_SORT_LDS;
        int rank = i - own * GBA_SORT_LDS;
        for (int c0 = 0, c = 0; c0 < n; c0 += GBA_SORT_LDS, ++c) {
            if (c == own) continue;
            int lo = c0, hi = min(c0 + GBA_SORT_LDS, n);
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
            rank += lo - c0;
        }
        t[rank] = v;
    }
    __threadfence_block();
    __syncthreads();
    for (int i = lane; i < n; i += GBA_T) a[i] = t[i];
}

// one workgroup: the tile-level fill of the block pattern by symbolic elimination, the tile lists of every column and row
__global__ __launch_bounds__(GBA_T) void gba_symbolic_kernel(GbaDev d) {
    __shared__ int list[GBA_MAX_NT];
    __shared__ int cnt;
    __shared__ int colc[GBA_MAX_NT + 1], rowc[GBA_MAX_NT + 1];
    const int lane = threadIdx.x, NT = d.NT, P = d.P;
    for (int i = lane; i < NT * NT; i += GBA_T) d.fill[i] = (i / NT == i % NT) ? 1 : 0;
    __syncthreads();
    for (int b = lane; b < d.NB; b += GBA_T) {
        const int key = d.blk_key[b], i1 = key / P, i2 = key % P;
        d.fill[(i2 / TV) * NT + i1 / TV] = 1;
    }
    __syncthreads();
    for (int J = 0; J < NT; ++J) {
        if (lane == 0) cnt = 0;
        __syncthreads();
        for (int I = J + 1 + lane; I < NT; I += GBA_T)
            if (d.fill[I * NT + J]) list[atomicAdd(&cnt, 1)] = I;
        __syncthreads();
        const int n = cnt;
        for (int p = lane; p < n * n; p += GBA_T) {
            const int I1 = list[p / n], I2 = list[p % n];
            if (I1 >= I2) d.fill[I1 * NT + I2] = 1;
        }
        __syncthreads();
    }
    for (int J = lane; J < NT; J += GBA_T) {
        int c = 0, r = 0;
        for (int I = J; I < NT; ++I) c += d.fill[I * NT + J];
        for (int K = 0; K <= J; ++K) r += d.fill[J * NT + K];
        colc[J] = c; rowc[J] = r;
    }
    __syncthreads();
    if (lane == 0) {
        int a = 0, b = 0;
        for (int J = 0; J < NT; ++J) {
            d.col_start[J] = a; d.row_start[J] = b;
            a += colc[J]; b += rowc[J];
            colc[J] = a - colc[J]; rowc[J] = b - rowc[J];
        }
        d.col_start[NT] = a; d.row_start[NT] = b;
        d.ctl_i[GBA_I_TILES] = a;
    }
    __syncthreads();
    for (int J = lane; J < NT; J += GBA_T) {
        int c = colc[J], r = rowc[J];
        for (int I = J; I < NT; ++I)
            if (d.fill[I * NT + J]) d.col_tiles[c++] = I;            // the diagonal tile comes first
        d.row_tiles[r++] = J;
        for (int K = 0; K < J; ++K)
            if (d.fill[J * NT + K]) d.row_tiles[r++] = K;
    }
}

// workgroup (I, J): the tile's place in the upper triangle is cleared when the fill holds it -- the matrix is a grow-only workspace and
// the Schur kernel writes the pattern's blocks only; a tile that only fills in reads H = +0.0.  Nothing else of the matrix is touched
__global__ __launch_bounds__(GBA_T) void gba_clear_kernel(GbaDev d) {
    const int I = blockIdx.x / d.NT, J = blockIdx.x % d.NT;
    if (I < J || !d.fill[I * d.NT + J]) return;
    const size_t NP = d.NP, rJ = (size_t)J * T, rI = (size_t)I * T;
    for (int idx = threadIdx.x; idx < TT; idx += GBA_T) d.mat[(rJ + idx / T) * NP + rI + idx % T] = 0.0;
}

// the padding behind 6 P: a unit diagonal, so that the padded rows factor to d = 1, L = 0 and touch nothing
__global__ __launch_bounds__(GBA_T) void gba_pad_kernel(GbaDev d) {
    const int r = 6 * d.P + blockIdx.x * GBA_T + threadIdx.x;
    if (r >= d.NP) return;
    d.mat[(size_t)r * d.NP + r] = 1.0;
    d.b[r] = 0.0;
}

// ---------------------------------------------------------------- linearise
template <bool ROBUST>
__global__ __launch_bounds__(GBA_T) void gba_error_kernel(GbaDev d, int cur) {
    const int e = blockIdx.x * GBA_T + threadIdx.x;
    if (e >= d.E) return;
    const LbaEdge E = lba_load(d, e, cur);
    double x, y, z, er[3], rho0, rho1;
    d.chi2[e] = lba_error<ROBUST>(d, E, x, y, z, er, rho0, rho1);
    d.rho0[e] = rho0;
}

template <bool ROBUST>
__global__ __launch_bounds__(GBA_T) void gba_linearise_kernel(GbaDev d, int cur) {
    const int e = blockIdx.x * GBA_T + threadIdx.x;
    if (e >= d.E) return;
    const LbaEdge E = lba_load(d, e, cur);
    lba_linearise_edge<ROBUST>(d, e, cur, E, d.free_index[E.k] >= 0);
}

// the sequential sums per vertex: thread (entry c, point p) for c < 9, then (entry c, free pose i) for c < 27
__global__ __launch_bounds__(GBA_T) void gba_vertex_sums_kernel(GbaDev d) {
    const long long t = (long long)blockIdx.x * GBA_T + threadIdx.x;
    const long long np = 9LL * d.L;
    const size_t S = (size_t)d.E;
    if (t < np) {
        const int c = (int)(t / d.L), p = (int)(t % d.L);
        const double* src = d.lin + S * c;
        double acc = 0.0;
        for (int e = d.pt_start[p], e1 = d.pt_start[p + 1]; e < e1; ++e) acc = acc + src[e];
        if (c < 6) d.Hll[(size_t)c * d.L + p] = acc; else d.bl[(size_t)(c - 6) * d.L + p] = acc;
    } else if (t < np + 27LL * d.P) {
        const int u = (int)(t - np), c = u / d.P, i = u % d.P;
        const double* src = d.lin + S * (9 + c);
        const int32_t* list = d.pose_list + d.pose_start[i];
        double acc = 0.0;
        for (int r = 0, n = d.pose_start[i + 1] - d.pose_start[i]; r < n; ++r) acc = acc + src[list[r]];
        if (c < 21) d.Hpp[c * d.P + i] = acc; else d.bp[(c - 21) * d.P + i] = acc;
    }
}

// computeLambdaInit's max |diagonal|: a NaN diagonal is ignored, so the order does not matter
__global__ __launch_bounds__(GBA_T) void gba_maxdiag_kernel(GbaDev d) {
    __shared__ double red[GBA_T];
    const int lane = threadIdx.x;
    double m = 0.0;
    for (int p = lane; p < d.L; p += GBA_T)
        for (int c = 0; c < 6; c += (c == 0 ? 3 : 2)) { const double a = fabs(d.Hll[(size_t)c * d.L + p]); if (a > m) m = a; }
    const int dg[6] = {0, 6, 11, 15, 18, 20};
    for (int i = lane; i < d.P; i += GBA_T)
        for (int c = 0; c < 6; ++c) { const double a = fabs(d.Hpp[dg[c] * d.P + i]); if (a > m) m = a; }
    red[lane] = m;
    __syncthreads();
    for (int s = GBA_T / 2; s >= 1; s >>= 1) {
        if (lane < s && red[lane + s] > red[lane]) red[lane] = red[lane + s];
        __syncthreads();
    }
    if (lane == 0) d.ctl_d[GBA_D_MAXDIAG] = red[0];
}

// 6l's departure (a): partial p adds src[i], i = p (mod 256), ascending from +0.0; lm_reduce combines the partials
__global__ __launch_bounds__(LM_LANES) void gba_reduce_kernel(const double* src, long long n, double* dst) {
    __shared__ double red[128];
    double acc[1] = {0.0};
    for (long long i = threadIdx.x; i < n; i += LM_LANES) acc[0] = acc[0] + src[i];
    lm_reduce<1>(acc, red, dst, threadIdx.x);
}

// ---------------------------------------------------------------- a trial
// per point: Dinv = (Hll + lambda I)^-1 by cofactors (6l's departure (d)), db = Dinv bl
__global__ __launch_bounds__(GBA_T) void gba_point_prep_kernel(GbaDev d, double lambda) {
    const int p = blockIdx.x * GBA_T + threadIdx.x;
    if (p >= d.L) return;
    const size_t L = (size_t)d.L;
    const double h0 = d.Hll[p], h1 = d.Hll[L + p], h2 = d.Hll[2 * L + p], h3 = d.Hll[3 * L + p], h4 = d.Hll[4 * L + p], h5 = d.Hll[5 * L + p];
    const double m00 = h0 + lambda, m01 = h1, m02 = h2, m10 = h1, m11 = h3 + lambda, m12 = h4, m20 = h2, m21 = h4, m22 = h5 + lambda;
    const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
    const double c10 = m02 * m21 - m01 * m22, c11 = m00 * m22 - m02 * m20, c12 = m01 * m20 - m00 * m21;
    const double c20 = m01 * m12 - m02 * m11, c21 = m02 * m10 - m00 * m12, c22 = m00 * m11 - m01 * m10;
    const double det = (m00 * c00 + m10 * c10) + m20 * c20;
    const double id = 1.0 / det;
    const double D[3][3] = {{c00 * id, c10 * id, c20 * id}, {c01 * id, c11 * id, c21 * id}, {c02 * id, c12 * id, c22 * id}};
    const double b0 = d.bl[p], b1 = d.bl[L + p], b2 = d.bl[2 * L + p];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d.Dinv[(size_t)(3 * r + c) * L + p] = D[r][c];
        d.db[(size_t)r * L + p] = (D[r][0] * b0 + D[r][1] * b1) + D[r][2] * b2;
    }
}

// per edge on a free pose: BDinv = B Dinv and B db
__global__ __launch_bounds__(GBA_T) void gba_edge_prep_kernel(GbaDev d) {
    const int e = blockIdx.x * GBA_T + threadIdx.x;
    if (e >= d.E || d.free_index[d.edge_kf[e]] < 0) return;
    const int p = d.edge_point[e];
    const size_t S = (size_t)d.E, L = (size_t)d.L;
    double D[3][3], db[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) D[r][c] = d.Dinv[(size_t)(3 * r + c) * L + p];
        db[r] = d.db[(size_t)r * L + p];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double b0 = d.lin[S * (36 + 3 * r) + e], b1 = d.lin[S * (37 + 3 * r) + e], b2 = d.lin[S * (38 + 3 * r) + e];
#pragma unroll
        for (int c = 0; c < 3; ++c) d.BDinv[S * (3 * r + c) + e] = (b0 * D[0][c] + b1 * D[1][c]) + b2 * D[2][c];
        d.Bdb[S * r + e] = (b0 * db[0] + b1 * db[1]) + b2 * db[2];
    }
}

// Hschur = Hpp + lambda I - sum B Dinv B^T, thread (non-empty block, entry) over its ascending pair list, into the upper triangle of the
// tiled matrix; then bschur = bp - sum B db, thread (pose, row) over the pose's ascending edge list
__global__ __launch_bounds__(GBA_T) void gba_schur_kernel(GbaDev d, double lambda) {
    const long long t = (long long)blockIdx.x * GBA_T + threadIdx.x;
    const int P = d.P, n = 6 * P;
    const long long nb = (long long)d.NB * 36;
    const size_t S = (size_t)d.E;
    if (t < nb) {
        const int blk = (int)(t / 36), ent = (int)(t % 36), r = ent / 6, c = ent % 6;
        const int key = d.blk_key[blk], i1 = key / P, i2 = key % P;
        if (i1 == i2 && r > c) return;
        double h = 0.0;
        if (i1 == i2) {
            h = d.Hpp[(r * 6 - (r * (r - 1)) / 2 + (c - r)) * P + i1];
            if (r == c) h = h + lambda;
        }
        const unsigned long long* pr = d.pairs + d.blk_start[blk];
        const double *a0 = d.BDinv + S * (3 * r), *a1 = a0 + S, *a2 = a1 + S;
        const double *b0 = d.lin + S * (36 + 3 * c), *b1 = b0 + S, *b2 = b1 + S;
        for (int k = 0, m = d.blk_start[blk + 1] - d.blk_start[blk]; k < m; ++k) {
            const unsigned long long pe = pr[k];
            const int e1 = (int)(pe >> 32), e2 = (int)(pe & 0xffffffffu);
            const double v = (a0[e1] * b0[e2] + a1[e1] * b1[e2]) + a2[e1] * b2[e2];
            h = h - v;
        }
        d.mat[(size_t)(6 * i1 + r) * d.NP + (6 * i2 + c)] = h;
    } else if (t < nb + n) {
        const int u = (int)(t - nb), i = u / 6, r = u % 6;
        const double* src = d.Bdb + S * r;
        const int32_t* list = d.pose_list + d.pose_start[i];
        double coeff = 0.0;
        for (int k = 0, m = d.pose_start[i + 1] - d.pose_start[i]; k < m; ++k) coeff = coeff + src[list[k]];
        d.b[u] = d.bp[r * P + i] - coeff;
    }
}

__global__ __launch_bounds__(LM_LANES) void gba_trial_begin_kernel(GbaDev d) {
    const int r = blockIdx.x * LM_LANES + threadIdx.x;
    if (r == 0) d.ctl_i[GBA_I_FAIL] = 0;
    if (r < d.NP) d.z[r] = d.b[r];
}

// the tile kernels are tile_ldlt.h's, on 24 x 24 tiles; lambda is inside Hschur already
__device__ __forceinline__ TileLdlt gba_tiles(const GbaDev& d) {
    return TileLdlt{d.mat, d.dvec, d.z, d.y, d.xs, d.fill, d.col_start, d.col_tiles, d.row_start, d.row_tiles, d.NT, d.NP, d.ctl_i + GBA_I_FAIL};
}
__global__ __launch_bounds__(LM_LANES) void gba_column_kernel(GbaDev d, int J) { tl_column<T>(gba_tiles(d), J, 0.0); }
__global__ __launch_bounds__(64) void gba_backward_kernel(GbaDev d, int J) { tl_backward<T>(gba_tiles(d), J); }

__global__ __launch_bounds__(LM_LANES) void gba_scale_kernel(GbaDev d) {
    const int r = blockIdx.x * LM_LANES + threadIdx.x;
    if (r < d.NP) d.y[r] = d.y[r] / d.dvec[r];
}

// one workgroup: the verdict -- a failed factor or a solution that is not finite leaves x as it was
__global__ __launch_bounds__(LM_LANES) void gba_commit_kernel(GbaDev d) {
    __shared__ int bad;
    const int lane = threadIdx.x, n = 6 * d.P;
    if (lane == 0) bad = d.ctl_i[GBA_I_FAIL];
    __syncthreads();
    int nf = 0;
    for (int r = lane; r < n; r += LM_LANES)
        if (!isfinite(d.xs[r])) nf = 1;
    if (nf) atomicOr(&bad, 1);
    __syncthreads();
    const int failed = bad;
    if (!failed)
        for (int r = lane; r < n; r += LM_LANES) d.xp[r] = d.xs[r] + 0.0;
    if (lane == 0) d.ctl_i[GBA_I_FAIL] = failed;
}

// the landmark part of the solution and the update: thread p < L: cl = bl + sum B^T (-xp), xl = Dinv cl, estimate + xl; thread L + i:
// exp(xp_i) estimate_i of free pose i.  Both leave their terms of computeScale in sterm (poses first).  After a failed solve x keeps its
// previous value
__global__ __launch_bounds__(GBA_T) void gba_update_kernel(GbaDev d, int cur, double lambda) {
    const int t = blockIdx.x * GBA_T + threadIdx.x;
    const int P = d.P;
    const size_t S = (size_t)d.E, L = (size_t)d.L;
    const bool solved = d.ctl_i[GBA_I_FAIL] == 0;
    if (t < d.L) {
        const int p = t;
        double xl[3];
        if (solved) {
            double cl[3] = {d.bl[p], d.bl[L + p], d.bl[2 * L + p]};
            for (int e = d.pt_start[p], e1 = d.pt_start[p + 1]; e < e1; ++e) {
                const int k = d.free_index[d.edge_kf[e]];
                if (k < 0) continue;
                double nx[6];
#pragma unroll
                for (int r = 0; r < 6; ++r) nx[r] = -d.xp[6 * k + r];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double v = d.lin[S * (36 + c) + e] * nx[0];
#pragma unroll
                    for (int r = 1; r < 6; ++r) v = v + d.lin[S * (36 + 3 * r + c) + e] * nx[r];
                    cl[c] = cl[c] + v;
                }
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double v = (d.Dinv[(size_t)(3 * r) * L + p] * cl[0] + d.Dinv[(size_t)(3 * r + 1) * L + p] * cl[1]) + d.Dinv[(size_t)(3 * r + 2) * L + p] * cl[2];
                xl[r] = 0.0 + v;
                d.xl[(size_t)r * L + p] = xl[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) xl[r] = d.xl[(size_t)r * L + p];
        }
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double v = d.pt[cur][3 * (size_t)p + r] + xl[r];
            d.pt[cur ^ 1][3 * (size_t)p + r] = v;
            fin = fin && isfinite(v);
            d.sterm[6 * P + 3 * (size_t)p + r] = xl[r] * (lambda * xl[r] + d.bl[(size_t)r * L + p]);
        }
        if (!fin) atomicOr(&d.ctl_i[GBA_I_FLAGS], RFE_GBA_FLAG_NONFINITE);
    } else if (t < d.L + P) {
        const int i = t - d.L, kf = d.free_list[i];
        double x[6], c[7], est[7];
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] = d.xp[6 * i + r];
#pragma unroll
        for (int r = 0; r < 7; ++r) c[r] = d.pose[cur][7 * kf + r];
        const bool fin = lm_se3_exp_mul(x, c, est);
#pragma unroll
        for (int r = 0; r < 7; ++r) d.pose[cur ^ 1][7 * kf + r] = est[r];
#pragma unroll
        for (int r = 0; r < 6; ++r) d.sterm[6 * i + r] = x[r] * (lambda * x[r] + d.bp[r * P + i]);
        if (!fin) atomicOr(&d.ctl_i[GBA_I_FLAGS], RFE_GBA_FLAG_NONFINITE);
    }
}

// ---------------------------------------------------------------- outputs
__global__ __launch_bounds__(GBA_T) void gba_finish_kernel(GbaDev d, int cur, double* pose, float* pose_f32, double* point, float* point_f32,
                                                           uint8_t* included, double* chi2) {
    const long long t = (long long)blockIdx.x * GBA_T + threadIdx.x;
    const long long n7 = 7LL * d.K, n3 = 3LL * d.L;
    bool fin = true;
    if (t < n7) {
        const double v = d.pose[cur][t];
        pose[t] = v;
        if (pose_f32) pose_f32[t] = (float)v;
        fin = isfinite(v);
    } else if (t < n7 + n3) {
        const long long u = t - n7;
        const double v = d.pt[cur][u];
        point[u] = v;
        if (point_f32) point_f32[u] = (float)v;
        fin = isfinite(v);
    }
    if (t < d.L) included[t] = d.pt_start[t + 1] > d.pt_start[t] ? 1 : 0;
    if (chi2 && t < d.E) chi2[t] = d.chi2[t];
    if (!fin) atomicOr(&d.ctl_i[GBA_I_FLAGS], RFE_GBA_FLAG_NONFINITE);
}

inline dim3 blocks(long long n, int per = LM_LANES) { return dim3((unsigned)((n + per - 1) / per)); }

}  // namespace

// the first kernels: the tables' verdict, the free keyframes' numbering, the estimates and the per-point ranges
void gba_launch_validate(hipStream_t s, const GbaDev& d) {
    hipLaunchKernelGGL(gba_validate_kernel, dim3(gba_grid(std::max(d.E, d.K + 1))), dim3(GBA_T), 0, s, d);
    hipLaunchKernelGGL(gba_number_kernel, dim3(1), dim3(GBA_T), 0, s, d);
    hipLaunchKernelGGL(gba_init_kernel, dim3(gba_grid(std::max(d.K, d.L + 1))), dim3(GBA_T), 0, s, d);
}

// with P known: the counts of every pose list and Schur block, their offsets and the non-empty blocks (ctl_i[GBA_I_NPAIRS], [GBA_I_NBLOCKS])
void gba_launch_count(hipStream_t s, const GbaDev& d) {
    if (d.P == 0) return;
    const long long nk = (long long)d.P * d.P;
    hipLaunchKernelGGL(gba_zero_kernel, dim3(gba_grid(nk)), dim3(GBA_T), 0, s, d.key_cnt, nk);
    if (d.E > 0) hipLaunchKernelGGL((gba_pairs_kernel<false>), dim3(gba_grid(d.E)), dim3(GBA_T), 0, s, d);
    hipLaunchKernelGGL(gba_scan_kernel, dim3(1), dim3(GBA_T), 0, s, d);
}

// with the pair workspace in place: the lists, ordered; the fill and the tile lists (ctl_i[GBA_I_TILES]); the cleared tiles and the padding
void gba_launch_structure(hipStream_t s, const GbaDev& d) {
    if (d.P == 0) return;
    if (d.E > 0) {
        hipLaunchKernelGGL((gba_pairs_kernel<true>), dim3(gba_grid(d.E)), dim3(GBA_T), 0, s, d);
        hipLaunchKernelGGL((gba_sort_kernel<uint32_t>), dim3(d.P), dim3(GBA_T), 0, s, (uint32_t*)d.pose_list, (uint32_t*)d.pose_tmp, (const int32_t*)d.pose_start);
        hipLaunchKernelGGL((gba_sort_kernel<unsigned long long>), dim3(d.NB), dim3(GBA_T), 0, s, d.pairs, d.pairs_tmp, (const int32_t*)d.blk_start);
    }
    hipLaunchKernelGGL(gba_symbolic_kernel, dim3(1), dim3(GBA_T), 0, s, d);
    hipLaunchKernelGGL(gba_clear_kernel, dim3(d.NT * d.NT), dim3(GBA_T), 0, s, d);
    if (d.NP > 6 * d.P) hipLaunchKernelGGL(gba_pad_kernel, dim3(gba_grid(d.NP - 6 * d.P)), dim3(GBA_T), 0, s, d);
}

// computeActiveErrors (+ buildSystem with `linearise`) at estimate `cur`; the (robust) chi2 summed into ctl_d[GBA_D_CHI]
void gba_launch_errors(hipStream_t s, const GbaDev& d, int cur, bool linearise, bool max_diagonal) {
    if (d.E > 0) {
        const dim3 g(gba_grid(d.E)), b(GBA_T);
        if (linearise) {
            if (d.robust) hipLaunchKernelGGL((gba_linearise_kernel<true>), g, b, 0, s, d, cur);
            else hipLaunchKernelGGL((gba_linearise_kernel<false>), g, b, 0, s, d, cur);
        } else {
            if (d.robust) hipLaunchKernelGGL((gba_error_kernel<true>), g, b, 0, s, d, cur);
            else hipLaunchKernelGGL((gba_error_kernel<false>), g, b, 0, s, d, cur);
        }
    }
    hipLaunchKernelGGL(gba_reduce_kernel, dim3(1), dim3(LM_LANES), 0, s, (const double*)d.rho0, (long long)d.E, d.ctl_d + GBA_D_CHI);
    if (linearise) {
        const long long n = 9LL * d.L + 27LL * d.P;
        if (n > 0) hipLaunchKernelGGL(gba_vertex_sums_kernel, dim3(gba_grid(n)), dim3(GBA_T), 0, s, d);
        if (max_diagonal) hipLaunchKernelGGL(gba_maxdiag_kernel, dim3(1), dim3(GBA_T), 0, s, d);
    }
}

// solve and update at lambda: the trial estimate goes to buffer cur ^ 1, computeScale's sum to ctl_d[GBA_D_SCALE]
void gba_launch_trial(hipStream_t s, const GbaDev& d, int cur, double lambda, const int32_t* col_start, const int32_t* row_start) {
    if (d.L > 0) hipLaunchKernelGGL(gba_point_prep_kernel, dim3(gba_grid(d.L)), dim3(GBA_T), 0, s, d, lambda);
    if (d.P > 0) {
        if (d.E > 0) hipLaunchKernelGGL(gba_edge_prep_kernel, dim3(gba_grid(d.E)), dim3(GBA_T), 0, s, d);
        hipLaunchKernelGGL(gba_schur_kernel, dim3(gba_grid(36LL * d.NB + 6 * d.P)), dim3(GBA_T), 0, s, d, lambda);
        hipLaunchKernelGGL(gba_trial_begin_kernel, blocks(d.NP), dim3(LM_LANES), 0, s, d);
        for (int J = 0; J < d.NT; ++J)
            hipLaunchKernelGGL(gba_column_kernel, dim3(col_start[J + 1] - col_start[J]), dim3(LM_LANES), 0, s, d, J);
        hipLaunchKernelGGL(gba_scale_kernel, blocks(d.NP), dim3(LM_LANES), 0, s, d);
        for (int J = d.NT - 1; J >= 0; --J)
            hipLaunchKernelGGL(gba_backward_kernel, dim3(row_start[J + 1] - row_start[J]), dim3(64), 0, s, d, J);
    } else {
        (void)hipMemsetAsync(d.ctl_i + GBA_I_FAIL, 0, sizeof(int32_t), s);
    }
    hipLaunchKernelGGL(gba_commit_kernel, dim3(1), dim3(LM_LANES), 0, s, d);
    if (d.L + d.P > 0) hipLaunchKernelGGL(gba_update_kernel, dim3(gba_grid((long long)d.L + d.P)), dim3(GBA_T), 0, s, d, cur, lambda);
    hipLaunchKernelGGL(gba_reduce_kernel, dim3(1), dim3(LM_LANES), 0, s, (const double*)d.sterm, 6LL * d.P + 3LL * d.L, d.ctl_d + GBA_D_SCALE);
}

void gba_launch_finish(hipStream_t s, const GbaDev& d, int cur, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* included,
                       double* chi2) {
    const long long n = std::max<long long>(7LL * d.K + 3LL * d.L, d.E);
    hipLaunchKernelGGL(gba_finish_kernel, dim3(gba_grid(n)), dim3(GBA_T), 0, s, d, cur, pose, pose_f32, point, point_f32, included, chi2);
}

}  // namespace rfe
