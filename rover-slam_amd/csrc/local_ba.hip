// local_ba.hip -- Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1857-2150 over g2o's BlockSolver_6_3 and Levenberg-Marquardt),
// DESIGN.md 6l.  The LM loop is driven by the host (api_local_ba.hip); every stage below is a plain launch whose threads own one edge, one
// (vertex, entry) or one (Schur block, entry) and add what they own in ascending edge / point order, so the sums do not depend on the
// launch.  The three sums over everything go through lm_reduce's 256 partials.  Everything is double, one rounding per operation
// (-ffp-contract=off); tests/local_ba_ref.py restates it operation by operation.
#include <float.h>
#include "rfe_internal.h"
#include "lm_device.h"
#include "lba_edge.h"

namespace rfe {
namespace {

constexpr int LBA_T = 256;
inline int lba_grid(long long n) { return (int)((n + LBA_T - 1) / LBA_T); }

// ---------------------------------------------------------------- validation: the first kernel; the host reads ctl_i[LBA_I_STATUS] before anything else runs
__global__ __launch_bounds__(LBA_T) void lba_validate_kernel(LbaDev d) {
    const int t = blockIdx.x * LBA_T + threadIdx.x;
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
    if (bad) atomicOr(&d.ctl_i[LBA_I_STATUS], bad);
}

// ---------------------------------------------------------------- estimates and per-point edge ranges
__global__ __launch_bounds__(LBA_T) void lba_init_kernel(LbaDev d) {
    const int t = blockIdx.x * LBA_T + threadIdx.x;
    if (t < d.K) {
        double q[7];
        for (int i = 0; i < 7; ++i) q[i] = (double)d.kf_pose[7 * t + i];
        po_normalize(q);
        for (int i = 0; i < 7; ++i) { d.pose[0][7 * t + i] = q[i]; d.pose[1][7 * t + i] = q[i]; }
    }
    if (t < d.L)
        for (int i = 0; i < 3; ++i) { const double v = (double)d.xw[3 * t + i]; d.pt[0][3 * t + i] = v; d.pt[1][3 * t + i] = v; }
    if (t <= d.L) {                                   // the first edge whose point is >= t
        int lo = 0, hi = d.E;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (d.edge_point[m] < t) lo = m + 1; else hi = m; }
        d.pt_start[t] = lo;
    }
}

// Schur block b -> (i1 <= i2): row i1 of the upper triangle holds the P - i1 blocks (i1, i1) .. (i1, P - 1)
__device__ inline void lba_unblock(int b, int P, int& i1, int& i2) {
    int i = 0, rem = b;
    while (i < P - 1 && rem >= P - i) { rem -= P - i; ++i; }
    i1 = i; i2 = i + rem;
}

// Stable selection, one workgroup per list.  KIND 0: pose b's edges among all E, ascending.  KIND 1: Schur block b = (i1, i2): the edges
// of pose i1 whose point also has an edge on pose i2, as (e1, e2), ascending in the point.  FILL false counts, true writes
template <int KIND, bool FILL>
__global__ __launch_bounds__(LBA_T) void lba_select_kernel(LbaDev d) {
    __shared__ int wsum[LBA_T / 64];
    const int b = blockIdx.x, lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
    int i1 = b, i2 = b;
    if (KIND == 1) lba_unblock(b, d.P, i1, i2);
    const int n = KIND == 0 ? d.E : d.pose_cnt[i1];
    const int32_t* src = KIND == 0 ? nullptr : d.pose_list + d.pose_start[i1];
    const int start = FILL ? (KIND == 0 ? d.pose_start[b] : d.blk_start[b]) : 0;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += LBA_T) {
        const int idx = c0 + lane;
        bool f = false; int e1 = -1, e2 = -1;
        if (idx < n) {
            if (KIND == 0) {
                e1 = idx; f = d.edge_kf[idx] == b;
            } else {
                e1 = src[idx];
                const int p = d.edge_point[e1];
                int lo = d.pt_start[p], hi = d.pt_start[p + 1];
                const int end = hi;
                while (lo < hi) { const int m = (lo + hi) >> 1; if (d.edge_kf[m] < i2) lo = m + 1; else hi = m; }
                if (lo < end && d.edge_kf[lo] == i2) { f = true; e2 = lo; }
            }
        }
        const unsigned long long m = __ballot(f);
        const int rank = __popcll(m & ((1ull << wl) - 1ull));
        if (wl == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < LBA_T / 64; ++w) { if (w < wave) off += wsum[w]; tot += wsum[w]; }
        if (FILL && f) {
            const int at = start + base + off + rank;
            if (KIND == 0) d.pose_list[at] = e1;
            else { d.pairs[2 * (size_t)at] = e1; d.pairs[2 * (size_t)at + 1] = e2; }
        }
        base += tot;
        __syncthreads();
    }
    if (!FILL && lane == 0) { if (KIND == 0) d.pose_cnt[b] = base; else d.blk_cnt[b] = base; }
}

// exclusive prefix sums of n counts; the total goes to ctl_i[slot]
__global__ void lba_prefix_kernel(const int32_t* cnt, int32_t* start, int n, int32_t* total) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < n; ++i) { start[i] = s; s += cnt[i]; }
        start[n] = s;
        *total = s;
    }
}

// ---------------------------------------------------------------- one edge: lba_edge.h, the Huber branch
// computeActiveErrors at estimate `cur`: the stored chi2 and the robust chi2 of every edge
__global__ __launch_bounds__(LBA_T) void lba_error_kernel(LbaDev d, int cur) {
    const int e = blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E) return;
    const LbaEdge E = lba_load(d, e, cur);
    double x, y, z, er[3], rho0, rho1;
    d.chi2[e] = lba_error<true>(d, E, x, y, z, er, rho0, rho1);
    d.rho0[e] = rho0;
}

// computeActiveErrors, linearizeOplus and constructQuadraticForm of one edge at estimate `cur`: its finished contributions go to
// lin [LBA_LIN][E]: 0-5 Hll's upper triangle, 6-8 bl, 9-29 Hpp's upper triangle, 30-35 bp, 36-53 the 6 x 3 Hpl block (Xj^T wOmega) Xi
__global__ __launch_bounds__(LBA_T) void lba_linearise_kernel(LbaDev d, int cur) {
    const int e = blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E) return;
    const LbaEdge E = lba_load(d, e, cur);
    lba_linearise_edge<true>(d, e, cur, E, E.k < d.P);
}

// the sequential sums per vertex: thread (entry c, point p) for c < 9, then (entry c, pose i) for c < 27
__global__ __launch_bounds__(LBA_T) void lba_vertex_sums_kernel(LbaDev d) {
    const long long t = (long long)blockIdx.x * LBA_T + threadIdx.x;
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
        for (int r = 0, n = d.pose_cnt[i]; r < n; ++r) acc = acc + src[list[r]];
        if (c < 21) d.Hpp[c * d.P + i] = acc; else d.bp[(c - 21) * d.P + i] = acc;
    }
}

// computeLambdaInit's max |diagonal|: a NaN diagonal is ignored, so the order does not matter
__global__ __launch_bounds__(LBA_T) void lba_maxdiag_kernel(LbaDev d) {
    __shared__ double red[LBA_T];
    const int lane = threadIdx.x;
    double m = 0.0;
    for (int p = lane; p < d.L; p += LBA_T)
        for (int c = 0; c < 6; c += (c == 0 ? 3 : 2)) { const double a = fabs(d.Hll[(size_t)c * d.L + p]); if (a > m) m = a; }
    const int dg[6] = {0, 6, 11, 15, 18, 20};
    for (int i = lane; i < d.P; i += LBA_T)
        for (int c = 0; c < 6; ++c) { const double a = fabs(d.Hpp[dg[c] * d.P + i]); if (a > m) m = a; }
    red[lane] = m;
    __syncthreads();
    for (int s = LBA_T / 2; s >= 1; s >>= 1) {
        if (lane < s && red[lane + s] > red[lane]) red[lane] = red[lane + s];
        __syncthreads();
    }
    if (lane == 0) d.ctl_d[LBA_D_MAXDIAG] = red[0];
}

// departure (a): partial p adds src[i], i = p (mod 256), ascending from +0.0; lm_reduce combines the partials
__global__ __launch_bounds__(LM_LANES) void lba_reduce_kernel(const double* src, int n, double* dst) {
    __shared__ double red[128];
    double acc[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += LM_LANES) acc[0] = acc[0] + src[i];
    lm_reduce<1>(acc, red, dst, threadIdx.x);
}

// ---------------------------------------------------------------- a trial
// per point: Dinv = (Hll + lambda I)^-1 by cofactors (departure (d)), db = Dinv bl
__global__ __launch_bounds__(LBA_T) void lba_point_prep_kernel(LbaDev d, double lambda) {
    const int p = blockIdx.x * LBA_T + threadIdx.x;
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
__global__ __launch_bounds__(LBA_T) void lba_edge_prep_kernel(LbaDev d) {
    const int e = blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E || d.edge_kf[e] >= d.P) return;
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

// Hschur = Hpp + lambda I - sum B Dinv B^T, thread (block, entry) over its ascending pair list, into the upper triangle of the dense
// S [6P, 6P]; then bschur = bp - sum B db, thread (pose, row) over the pose's ascending edge list
__global__ __launch_bounds__(LBA_T) void lba_schur_kernel(LbaDev d, double lambda) {
    const long long t = (long long)blockIdx.x * LBA_T + threadIdx.x;
    const int P = d.P, n = 6 * P;
    const long long nb = (long long)d.NB * 36;
    const size_t S = (size_t)d.E;
    if (t < nb) {
        const int blk = (int)(t / 36), ent = (int)(t % 36), r = ent / 6, c = ent % 6;
        int i1, i2;
        lba_unblock(blk, P, i1, i2);
        if (i1 == i2 && r > c) return;
        double h = 0.0;
        if (i1 == i2) {
            h = d.Hpp[(r * 6 - (r * (r - 1)) / 2 + (c - r)) * P + i1];
            if (r == c) h = h + lambda;
        }
        const int32_t* pr = d.pairs + 2 * (size_t)d.blk_start[blk];
        const double *a0 = d.BDinv + S * (3 * r), *a1 = a0 + S, *a2 = a1 + S;
        const double *b0 = d.lin + S * (36 + 3 * c), *b1 = b0 + S, *b2 = b1 + S;
        for (int k = 0, m = d.blk_cnt[blk]; k < m; ++k) {
            const int e1 = pr[2 * k], e2 = pr[2 * k + 1];
            const double v = (a0[e1] * b0[e2] + a1[e1] * b1[e2]) + a2[e1] * b2[e2];
            h = h - v;
        }
        d.S[(size_t)(6 * i1 + r) * n + (6 * i2 + c)] = h;
    } else if (t < nb + n) {
        const int u = (int)(t - nb), i = u / 6, r = u % 6;
        const double* src = d.Bdb + S * r;
        const int32_t* list = d.pose_list + d.pose_start[i];
        double coeff = 0.0;
        for (int k = 0, m = d.pose_cnt[i]; k < m; ++k) coeff = coeff + src[list[k]];
        d.bs[u] = d.bp[r * P + i] - coeff;
    }
}

// departure (c): dense unpivoted LDLT of S's upper triangle in place (row k right of the diagonal ends as L's column k), forward
// substitution ascending, y / d, back substitution descending.  One workgroup; lane l owns rows l and l + 256.  A pivot that is zero or
// not finite: ctl_i[LBA_I_SOLVED] = 0 and xp is left alone
constexpr int LBA_MAX_N = 6 * RFE_LBA_MAX_FREE;
__global__ __launch_bounds__(LBA_T) void lba_ldlt_kernel(LbaDev d) {
    __shared__ double w[LBA_MAX_N], dd[LBA_MAX_N];
    __shared__ int fail;
    const int lane = threadIdx.x, n = 6 * d.P;
    double* A = d.S;
    if (lane == 0) fail = 0;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        for (int k = lane; k < j; k += LBA_T) w[k] = A[(size_t)k * n + j] * dd[k];
        __syncthreads();
        for (int i = j + lane; i < n; i += LBA_T) {
            double a = A[(size_t)j * n + i];
            for (int k = 0; k < j; ++k) a = a - A[(size_t)k * n + i] * w[k];
            if (i == j) { dd[j] = a; if (!isfinite(a) || a == 0.0) fail = 1; }
            else A[(size_t)j * n + i] = a;
        }
        __syncthreads();
        if (fail) break;
        const double dj = dd[j];
        for (int i = j + lane; i < n; i += LBA_T)
            if (i > j) A[(size_t)j * n + i] = A[(size_t)j * n + i] / dj;
        __syncthreads();
    }
    if (fail) { if (lane == 0) d.ctl_i[LBA_I_SOLVED] = 0; return; }
    const int i0 = lane, i1 = lane + LBA_T;
    double a0 = i0 < n ? d.bs[i0] : 0.0, a1 = i1 < n ? d.bs[i1] : 0.0;
    for (int k = 0; k < n; ++k) {
        if (i0 == k) w[k] = a0;
        if (i1 == k) w[k] = a1;
        __syncthreads();
        const double yk = w[k];
        if (i0 > k && i0 < n) a0 = a0 - A[(size_t)k * n + i0] * yk;
        if (i1 > k && i1 < n) a1 = a1 - A[(size_t)k * n + i1] * yk;
    }
    __syncthreads();
    if (i0 < n) a0 = a0 / dd[i0];
    if (i1 < n) a1 = a1 / dd[i1];
    for (int k = n - 1; k >= 0; --k) {
        if (i0 == k) w[k] = a0;
        if (i1 == k) w[k] = a1;
        __syncthreads();
        const double xk = w[k];
        if (i0 < k) a0 = a0 - A[(size_t)i0 * n + k] * xk;
        if (i1 < k && i1 < n) a1 = a1 - A[(size_t)i1 * n + k] * xk;
    }
    if (i0 < n) d.xp[i0] = a0;
    if (i1 < n) d.xp[i1] = a1;
    if (lane == 0) d.ctl_i[LBA_I_SOLVED] = 1;
}

// the landmark part of the solution and the update: thread p < L: cl = bl + sum B^T (-xp), xl = Dinv cl, estimate + xl; thread L + i:
// exp(xp_i) estimate_i.  Both leave their terms of computeScale in sterm (poses first).  After a failed solve x keeps its previous value
__global__ __launch_bounds__(LBA_T) void lba_update_kernel(LbaDev d, int cur, double lambda) {
    const int t = blockIdx.x * LBA_T + threadIdx.x;
    const int P = d.P;
    const size_t S = (size_t)d.E, L = (size_t)d.L;
    const bool solved = d.ctl_i[LBA_I_SOLVED] != 0;
    if (t < d.L) {
        const int p = t;
        double xl[3];
        if (solved) {
            double cl[3] = {d.bl[p], d.bl[L + p], d.bl[2 * L + p]};
            for (int e = d.pt_start[p], e1 = d.pt_start[p + 1]; e < e1; ++e) {
                const int k = d.edge_kf[e];
                if (k >= P) break;                    // sorted by keyframe: the free ones come first
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
        if (!fin) atomicOr(&d.ctl_i[LBA_I_FLAGS], RFE_LBA_FLAG_NONFINITE);
    } else if (t < d.L + P) {
        const int i = t - d.L;
        double x[6], c[7], est[7];
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] = d.xp[6 * i + r];
#pragma unroll
        for (int r = 0; r < 7; ++r) c[r] = d.pose[cur][7 * i + r];
        const bool fin = lm_se3_exp_mul(x, c, est);
#pragma unroll
        for (int r = 0; r < 7; ++r) d.pose[cur ^ 1][7 * i + r] = est[r];
#pragma unroll
        for (int r = 0; r < 6; ++r) d.sterm[6 * i + r] = x[r] * (lambda * x[r] + d.bp[r * P + i]);
        if (!fin) atomicOr(&d.ctl_i[LBA_I_FLAGS], RFE_LBA_FLAG_NONFINITE);
    }
}

// ---------------------------------------------------------------- classification and outputs
// erase[e] = chi2_e > th2 || !isDepthPositive, the stored chi2 against the double threshold, the depth at estimate `cur`
__global__ __launch_bounds__(LBA_T) void lba_classify_kernel(LbaDev d, int cur, uint8_t* erase, double* chi2_out) {
    const int e = blockIdx.x * LBA_T + threadIdx.x;
    if (e >= d.E) return;
    const LbaEdge E = lba_load(d, e, cur);
    double x, y, z;
    po_rotate(E.q, E.X[0], E.X[1], E.X[2], x, y, z);
    z = z + E.q[6];
    const double c = d.chi2[e];
    const bool out = c > (E.stereo ? d.th2_stereo : d.th2_mono) || !(z > 0.0);
    erase[e] = out ? 1 : 0;
    if (chi2_out) chi2_out[e] = c;
    if (out) atomicAdd(&d.ctl_i[LBA_I_ERASED], 1);
}

__global__ __launch_bounds__(LBA_T) void lba_finish_kernel(LbaDev d, int cur, double* pose, float* pose_f32, double* point, float* point_f32) {
    const int t = blockIdx.x * LBA_T + threadIdx.x;
    bool fin = true;
    if (t < 7 * d.P) {
        const double v = d.pose[cur][t];
        pose[t] = v;
        if (pose_f32) pose_f32[t] = (float)v;
        fin = isfinite(v);
    } else if (t < 7 * d.P + 3 * d.L) {
        const int u = t - 7 * d.P;
        const double v = d.pt[cur][u];
        point[u] = v;
        if (point_f32) point_f32[u] = (float)v;
        fin = isfinite(v);
    }
    if (!fin) atomicOr(&d.ctl_i[LBA_I_FLAGS], RFE_LBA_FLAG_NONFINITE);
}

}  // namespace

void lba_launch_validate(hipStream_t s, const LbaDev& d) {
    hipLaunchKernelGGL(lba_validate_kernel, dim3(lba_grid(std::max(d.E, d.K + 1))), dim3(LBA_T), 0, s, d);
}

// the estimates, the per-point ranges and the per-pose lists; leaves the number of pairs per Schur block counted and summed (ctl_i[LBA_I_NPAIRS])
void lba_launch_structure(hipStream_t s, const LbaDev& d) {
    hipLaunchKernelGGL(lba_init_kernel, dim3(lba_grid(std::max(d.K, d.L + 1))), dim3(LBA_T), 0, s, d);
    if (d.P > 0) {
        hipLaunchKernelGGL((lba_select_kernel<0, false>), dim3(d.P), dim3(LBA_T), 0, s, d);
        hipLaunchKernelGGL(lba_prefix_kernel, dim3(1), dim3(1), 0, s, (const int32_t*)d.pose_cnt, d.pose_start, d.P, d.ctl_i + LBA_I_NFREE);
        hipLaunchKernelGGL((lba_select_kernel<0, true>), dim3(d.P), dim3(LBA_T), 0, s, d);
        hipLaunchKernelGGL((lba_select_kernel<1, false>), dim3(d.NB), dim3(LBA_T), 0, s, d);
        hipLaunchKernelGGL(lba_prefix_kernel, dim3(1), dim3(1), 0, s, (const int32_t*)d.blk_cnt, d.blk_start, d.NB, d.ctl_i + LBA_I_NPAIRS);
    }
}
void lba_launch_pairs(hipStream_t s, const LbaDev& d) {
    if (d.P > 0) hipLaunchKernelGGL((lba_select_kernel<1, true>), dim3(d.NB), dim3(LBA_T), 0, s, d);
}

// computeActiveErrors (+ buildSystem with `linearise`) at estimate `cur`; the robust chi2 summed into ctl_d[LBA_D_CHI]
void lba_launch_errors(hipStream_t s, const LbaDev& d, int cur, bool linearise, bool max_diagonal) {
    if (d.E > 0) {
        if (linearise) hipLaunchKernelGGL(lba_linearise_kernel, dim3(lba_grid(d.E)), dim3(LBA_T), 0, s, d, cur);
        else hipLaunchKernelGGL(lba_error_kernel, dim3(lba_grid(d.E)), dim3(LBA_T), 0, s, d, cur);
    }
    hipLaunchKernelGGL(lba_reduce_kernel, dim3(1), dim3(LM_LANES), 0, s, (const double*)d.rho0, d.E, d.ctl_d + LBA_D_CHI);
    if (linearise) {
        const long long n = 9LL * d.L + 27LL * d.P;
        if (n > 0) hipLaunchKernelGGL(lba_vertex_sums_kernel, dim3(lba_grid(n)), dim3(LBA_T), 0, s, d);
        if (max_diagonal) hipLaunchKernelGGL(lba_maxdiag_kernel, dim3(1), dim3(LBA_T), 0, s, d);
    }
}

// solve and update at lambda: the trial estimate goes to buffer cur ^ 1, computeScale's sum to ctl_d[LBA_D_SCALE]
void lba_launch_trial(hipStream_t s, const LbaDev& d, int cur, double lambda) {
    if (d.L > 0) hipLaunchKernelGGL(lba_point_prep_kernel, dim3(lba_grid(d.L)), dim3(LBA_T), 0, s, d, lambda);
    if (d.P > 0) {
        if (d.E > 0) hipLaunchKernelGGL(lba_edge_prep_kernel, dim3(lba_grid(d.E)), dim3(LBA_T), 0, s, d);
        hipLaunchKernelGGL(lba_schur_kernel, dim3(lba_grid(36LL * d.NB + 6 * d.P)), dim3(LBA_T), 0, s, d, lambda);
    }
    hipLaunchKernelGGL(lba_ldlt_kernel, dim3(1), dim3(LBA_T), 0, s, d);
    if (d.L + d.P > 0) hipLaunchKernelGGL(lba_update_kernel, dim3(lba_grid(d.L + d.P)), dim3(LBA_T), 0, s, d, cur, lambda);
    hipLaunchKernelGGL(lba_reduce_kernel, dim3(1), dim3(LM_LANES), 0, s, (const double*)d.sterm, 6 * d.P + 3 * d.L, d.ctl_d + LBA_D_SCALE);
}

void lba_launch_finish(hipStream_t s, const LbaDev& d, int cur, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* erase,
                       double* chi2) {
    if (d.E > 0) hipLaunchKernelGGL(lba_classify_kernel, dim3(lba_grid(d.E)), dim3(LBA_T), 0, s, d, cur, erase, chi2);
    const int n = 7 * d.P + 3 * d.L;
    if (n > 0) hipLaunchKernelGGL(lba_finish_kernel, dim3(lba_grid(n)), dim3(LBA_T), 0, s, d, cur, pose, pose_f32, point, point_f32);
}

}  // namespace rfe
