// essential_graph.hip -- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:4509-4840 over g2o's BlockSolver_7_3 and
// Levenberg-Marquardt), DESIGN.md 6m.  The LM loop is the host's (api_essential_graph.hip); every stage here is a plain launch.
//   front       validation, the free vertices' numbering, Sim3(+-delta e_d), the measurements, the per-vertex edge lists, the tile fill
//   linearise   one thread per edge: the error and its 28 perturbed errors (eg_errors), one thread per (entry, edge): the 119 finished
//               contributions (eg_products), one thread per (vertex, entry): their sums in edge order into the dense matrix (eg_assemble)
//   solve       left-looking LDLT over 28 x 28 tiles, one launch per tile column, one workgroup per non-zero tile of the column; each
//               thread owns its entries and subtracts L_ik (L_jk d_k) in ascending k, so the bits are those of the dense per-entry order.
//               The forward substitution rides in the same launches, the backward one takes one launch per tile row
//   update, error pass, the two 256-partial sums, the outputs and the map-point correction
// Everything is double, one rounding per operation (-ffp-contract=off); tests/essential_graph_ref.py restates it operation by operation.
#include <float.h>
#include "rfe_internal.h"
#include "lm_device.h"
#include "tile_ldlt.h"

namespace rfe {
namespace {

constexpr int T = EG_TILE, TV = EG_TILE_V;
constexpr int EG_MAX_N = 1024, EG_MAX_NT = EG_MAX_N / EG_TILE_V;

__device__ inline bool eg_finite8(const double* v) {
    bool f = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) f = f && isfinite(v[i]);
    return f;
}

// (M Si) Sj^-1 .log()
__device__ __forceinline__ void eg_error(const double* M, const double* Si, const double* Sj, double* e) {
    double a[8], inv[8], b[8];
    lm_sim3_mul(M, Si, a);
    lm_sim3_inverse(Sj, inv);
    lm_sim3_mul(a, inv, b);
    lm_sim3_log(b, e);
}

// ---------------------------------------------------------------- front
// one workgroup: the edge table's verdict, the free vertices in ascending index, the 14 perturbations, the estimate's first copy
__global__ __launch_bounds__(LM_LANES) void eg_front_kernel(EgDev d) {
    __shared__ int status;
    const int lane = threadIdx.x;
    if (lane == 0) status = 0;
    __syncthreads();
    int st = 0;
    for (int e = lane; e < d.E; e += LM_LANES) {
        const int i = d.edge_i[e], j = d.edge_j[e];
        if (i < 0 || i >= d.N || j < 0 || j >= d.N || i == j) st |= EG_BAD_RANGE;
        if (e > 0) {
            const int pi = d.edge_i[e - 1], pj = d.edge_j[e - 1];
            if (pi > i || (pi == i && pj > j)) st |= EG_BAD_ORDER;
        }
    }
    if (st) atomicOr(&status, st);
    for (int v = lane; v < d.N * 8; v += LM_LANES) d.est[0][v] = d.s_est[v];
    if (lane >= 1 && lane <= 14) {
        const int k = lane - 1, dd = k >> 1;
        double u[7], q[4], t[3], s;
#pragma unroll
        for (int j = 0; j < 7; ++j) u[j] = (j == dd) ? ((k & 1) ? -1e-9 : 1e-9) : 0.0;
        if (d.fix_scale) u[6] = 0.0;
        lm_sim3_exp(u, q, t, s);
        double* o = d.pert + 8 * k;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = t[0]; o[5] = t[1]; o[6] = t[2]; o[7] = s;
    }
    if (lane == 0) {
        int nf = 0;
        for (int v = 0; v < d.N; ++v) {
            const bool fr = d.fixed[v] == 0;
            d.free_index[v] = fr ? nf : -1;
            if (fr) d.free_list[nf++] = v;
        }
        d.ctl_i[EG_I_NFREE] = nf;
    }
    __syncthreads();
    if (lane == 0 && status) atomicOr(&d.ctl_i[EG_I_STATUS], status);
}

__global__ __launch_bounds__(LM_LANES) void eg_check_points_kernel(EgDev d) {
    const int l = blockIdx.x * LM_LANES + threadIdx.x;
    if (l >= d.L) return;
    const int r = d.point_ref[l];
    if (r < -1 || r >= d.N) atomicOr(&d.ctl_i[EG_I_STATUS], EG_BAD_REF);
}

// Sji = Sjw Swi from the table the edge names
__global__ __launch_bounds__(LM_LANES) void eg_meas_kernel(EgDev d) {
    const int e = blockIdx.x * LM_LANES + threadIdx.x;
    if (e >= d.E) return;
    const double* tab = d.edge_src[e] ? d.s_est : d.s_meas;
    double Si[8], Sj[8], inv[8], M[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { Si[k] = tab[8 * (size_t)d.edge_i[e] + k]; Sj[k] = tab[8 * (size_t)d.edge_j[e] + k]; }
    lm_sim3_inverse(Si, inv);
    lm_sim3_mul(Sj, inv, M);
#pragma unroll
    for (int k = 0; k < 8; ++k) d.meas[8 * (size_t)e + k] = M[k];
}

// one thread per free vertex: how many edge ends it has (pass 0) or their list in ascending edge index (pass 1)
__global__ __launch_bounds__(LM_LANES) void eg_incidence_kernel(EgDev d, int pass) {
    const int f = blockIdx.x * LM_LANES + threadIdx.x;
    if (f >= d.Nf) return;
    const int v = d.free_list[f];
    int n = 0;
    int32_t* out = pass ? d.inc_list + d.inc_start[f] : nullptr;
    for (int e = 0; e < d.E; ++e) {
        const int side = d.edge_i[e] == v ? 0 : (d.edge_j[e] == v ? 1 : -1);
        if (side < 0) continue;
        if (pass) out[n] = 2 * e + side;
        ++n;
    }
    if (!pass) d.inc_start[f + 1] = n;               // counts for now; eg_symbolic_kernel turns them into offsets
}

// one workgroup: the lists' offsets, the tile-level fill of the pattern by symbolic elimination, the tile lists of every column and row
__global__ __launch_bounds__(LM_LANES) void eg_symbolic_kernel(EgDev d) {
    __shared__ int list[EG_MAX_NT];
    __shared__ int cnt;
    __shared__ int colc[EG_MAX_NT + 1], rowc[EG_MAX_NT + 1];
    const int lane = threadIdx.x, NT = d.NT;
    if (lane == 0) {
        int acc = 0;
        d.inc_start[0] = 0;
        for (int f = 0; f < d.Nf; ++f) { acc += d.inc_start[f + 1]; d.inc_start[f + 1] = acc; }
    }
    for (int i = lane; i < NT * NT; i += LM_LANES) d.fill[i] = (i / NT == i % NT) ? 1 : 0;
    __syncthreads();
    for (int e = lane; e < d.E; e += LM_LANES) {
        const int fi = d.free_index[d.edge_i[e]], fj = d.free_index[d.edge_j[e]];
        if (fi < 0 || fj < 0) continue;
        const int a = (fi > fj ? fi : fj) / TV, b = (fi > fj ? fj : fi) / TV;
        d.fill[a * NT + b] = 1;
    }
    __syncthreads();
    for (int J = 0; J < NT; ++J) {
        if (lane == 0) cnt = 0;
        __syncthreads();
        for (int I = J + 1 + lane; I < NT; I += LM_LANES)
            if (d.fill[I * NT + J]) list[atomicAdd(&cnt, 1)] = I;
        __syncthreads();
        const int n = cnt;
        for (int p = lane; p < n * n; p += LM_LANES) {
            const int I1 = list[p / n], I2 = list[p % n];
            if (I1 >= I2) d.fill[I1 * NT + I2] = 1;
        }
        __syncthreads();
    }
    for (int J = lane; J < NT; J += LM_LANES) {
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
        d.ctl_i[EG_I_TILES] = a;
    }
    __syncthreads();
    for (int J = lane; J < NT; J += LM_LANES) {
        int c = colc[J], r = rowc[J];
        for (int I = J; I < NT; ++I)
            if (d.fill[I * NT + J]) d.col_tiles[c++] = I;            // the diagonal tile comes first
        d.row_tiles[r++] = J;
        for (int K = 0; K < J; ++K)
            if (d.fill[J * NT + K]) d.row_tiles[r++] = K;
    }
}

// the padding behind 7 Nf: a unit diagonal, so that the padded rows factor to d = 1 + lambda, L = 0 and touch nothing
__global__ __launch_bounds__(LM_LANES) void eg_pad_kernel(EgDev d) {
    const int r = 7 * d.Nf + blockIdx.x * LM_LANES + threadIdx.x;
    if (r >= d.NP) return;
    d.mat[(size_t)r * d.NP + r] = 1.0;
    d.b[r] = 0.0;
}

// the numeric Jacobian with respect to vertex SIDE of one edge, one column at a time: (e(+delta) - e(-delta)) / (2 delta) through oplus
template <int SIDE>
__device__ __forceinline__ void eg_jacobian(const EgDev& d, int e, const double (&M)[8], const double (&Si)[8], const double (&Sj)[8]) {
    const size_t E = d.E;
    const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll 1
    for (int c = 0; c < 7; ++c) {
        double P[8], Q[8], ep[7], em[7];
#pragma unroll
        for (int k = 0; k < 8; ++k) P[k] = d.pert[8 * (2 * c) + k];
        lm_sim3_mul(P, SIDE ? Sj : Si, Q);
        eg_error(M, SIDE ? Si : Q, SIDE ? Q : Sj, ep);
#pragma unroll
        for (int k = 0; k < 8; ++k) P[k] = d.pert[8 * (2 * c + 1) + k];
        lm_sim3_mul(P, SIDE ? Sj : Si, Q);
        eg_error(M, SIDE ? Si : Q, SIDE ? Q : Sj, em);
#pragma unroll
        for (int k = 0; k < 7; ++k) d.jac[(7 + 49 * SIDE + 7 * k + c) * E + e] = scalar * (ep[k] - em[k]);
    }
}

// ---------------------------------------------------------------- linearise
// one thread per edge: the error and chi2; when linearising also the numeric Jacobians (base_binary_edge.hpp:131-205), one column at a
// time through global memory so that no more than two errors live in registers
__global__ __launch_bounds__(LM_LANES) void eg_errors_kernel(EgDev d, int cur, int linearise) {
    const int e = blockIdx.x * LM_LANES + threadIdx.x;
    if (e >= d.E) return;
    const size_t E = d.E;
    const int vi = d.edge_i[e], vj = d.edge_j[e];
    const double* est = cur ? d.est[1] : d.est[0];
    double M[8], Si[8], Sj[8], err[7];
#pragma unroll
    for (int k = 0; k < 8; ++k) { M[k] = d.meas[8 * (size_t)e + k]; Si[k] = est[8 * (size_t)vi + k]; Sj[k] = est[8 * (size_t)vj + k]; }
    eg_error(M, Si, Sj, err);
    double chi2 = err[0] * err[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) chi2 = chi2 + err[k] * err[k];
    d.chi2[e] = chi2;
    if (!linearise) return;
#pragma unroll
    for (int k = 0; k < 7; ++k) d.jac[k * E + e] = err[k];
    eg_jacobian<0>(d, e, M, Si, Sj);
    eg_jacobian<1>(d, e, M, Si, Sj);
}

// one thread per (entry, edge): Hii's upper triangle (28), bi (7), Hjj (28), bj (7), Hij (49, rows of i); every sum over the 7 error rows
// in ascending row from the first product.  Information is the identity: A^T Omega is A^T, omega_r is -e
__global__ __launch_bounds__(LM_LANES) void eg_products_kernel(EgDev d) {
    const size_t E = d.E;
    const size_t idx = (size_t)blockIdx.x * LM_LANES + threadIdx.x;
    if (idx >= E * EG_CON) return;
    const int q = (int)(idx / E), e = (int)(idx % E);
    const double* err = d.jac + e;
    const double* A = d.jac + 7 * E + e;
    const double* B = d.jac + 56 * E + e;
    const double *X, *Y;
    int a, b;
    bool grad = false;
    if (q < 70) {
        const int side = q >= 35, r = q - 35 * side;
        X = side ? B : A; Y = X;
        if (r < 28) {
            a = 0; b = r;
            while (b >= 7 - a) { b -= 7 - a; ++a; }
            b += a;
        } else { a = r - 28; b = 0; grad = true; }
    } else { X = A; Y = B; a = (q - 70) / 7; b = (q - 70) % 7; }
    double v;
    if (grad) {
        v = X[(size_t)a * E] * (-err[0]);
        for (int k = 1; k < 7; ++k) v = v + X[(7 * k + a) * E] * (-err[k * E]);
    } else {
        v = X[(size_t)a * E] * Y[(size_t)b * E];
        for (int k = 1; k < 7; ++k) v = v + X[(7 * k + a) * E] * Y[(7 * k + b) * E];
    }
    d.con[idx] = v;
}

// one thread per (free vertex, entry): 28 of the diagonal block, 7 of b, 49 of every block right of the diagonal in the vertex's row.
// Each sum runs over the vertex's edge list, that is in ascending edge index, from +0.0
__global__ __launch_bounds__(LM_LANES) void eg_assemble_kernel(EgDev d) {
    const int idx = blockIdx.x * LM_LANES + threadIdx.x;
    if (idx >= d.Nf * 84) return;
    const int f = idx / 84, q = idx % 84;
    const size_t E = d.E, NP = d.NP;
    const int32_t* lst = d.inc_list + d.inc_start[f];
    const int n = d.inc_start[f + 1] - d.inc_start[f];
    if (q < 35) {
        double v = 0.0;
        for (int m = 0; m < n; ++m) {
            const int e = lst[m] >> 1, side = lst[m] & 1;
            v = v + d.con[(size_t)(35 * side + q) * E + e];
        }
        if (q < 28) {
            int a = 0, b = q;
            while (b >= 7 - a) { b -= 7 - a; ++a; }
            b += a;
            d.mat[(size_t)(7 * f + a) * NP + 7 * f + b] = v;
        } else d.b[7 * f + q - 28] = v;
        return;
    }
    const int a = (q - 35) / 7, b = (q - 35) % 7;
    for (int pass = 0; pass < 2; ++pass)
        for (int m = 0; m < n; ++m) {
            const int e = lst[m] >> 1, side = lst[m] & 1;
            const int fw = d.free_index[side ? d.edge_i[e] : d.edge_j[e]];
            if (fw <= f) continue;                   // fixed (-1), or the block belongs to the other vertex's row
            double* t = d.mat + (size_t)(7 * f + a) * NP + 7 * fw + b;
            if (pass == 0) *t = 0.0;
            else *t = *t + d.con[(size_t)(70 + (side ? 7 * b + a : 7 * a + b)) * E + e];
        }
}

// one workgroup: a vector's sum in the 256-partial order of departure (a); optionally the largest |diagonal| of H, NaN ignored
__global__ __launch_bounds__(LM_LANES) void eg_reduce_kernel(EgDev d, const double* src, int n, int slot, int max_diagonal) {
    __shared__ double red[128];
    const int lane = threadIdx.x;
    double acc[1] = {0.0};
    for (int i = lane; i < n; i += LM_LANES) acc[0] = acc[0] + src[i];
    lm_reduce<1>(acc, red, d.ctl_d + slot, lane);
    if (!max_diagonal) return;
    __syncthreads();
    double m = 0.0;
    for (int r = lane; r < 7 * d.Nf; r += LM_LANES) {
        const double a = fabs(d.mat[(size_t)r * d.NP + r]);
        if (a > m) m = a;
    }
    if (lane >= 128) red[lane - 128] = m;
    __syncthreads();
    if (lane < 128 && red[lane] > m) m = red[lane];
    __syncthreads();
    for (int s = 64; s >= 1; s >>= 1) {
        if (lane < 2 * s && lane >= s) red[lane - s] = m;
        __syncthreads();
        if (lane < s && red[lane] > m) m = red[lane];
        __syncthreads();
    }
    if (lane == 0) d.ctl_d[EG_D_MAXDIAG] = m;
}

// ---------------------------------------------------------------- the solve
__global__ __launch_bounds__(LM_LANES) void eg_trial_begin_kernel(EgDev d) {
    const int r = blockIdx.x * LM_LANES + threadIdx.x;
    if (r == 0) d.ctl_i[EG_I_FAIL] = 0;
    if (r < d.NP) d.z[r] = d.b[r];
}

// the tile kernels are tile_ldlt.h's, on 28 x 28 tiles
__device__ __forceinline__ TileLdlt eg_tiles(const EgDev& d) {
    return TileLdlt{d.mat, d.dvec, d.z, d.y, d.xs, d.fill, d.col_start, d.col_tiles, d.row_start, d.row_tiles, d.NT, d.NP, d.ctl_i + EG_I_FAIL};
}
__global__ __launch_bounds__(LM_LANES) void eg_column_kernel(EgDev d, int J, double lambda) { tl_column<T>(eg_tiles(d), J, lambda); }

__global__ __launch_bounds__(LM_LANES) void eg_scale_kernel(EgDev d) {
    const int r = blockIdx.x * LM_LANES + threadIdx.x;
    if (r < d.NP) d.y[r] = d.y[r] / d.dvec[r];
}

__global__ __launch_bounds__(64) void eg_backward_kernel(EgDev d, int J) { tl_backward<T>(eg_tiles(d), J); }

// one workgroup: the verdict (a failed factor or a solution that is not finite leaves x as it was), oplusImpl's zeroing of the scale
// entries in the solver's x, and computeScale's terms
__global__ __launch_bounds__(LM_LANES) void eg_commit_kernel(EgDev d, double lambda) {
    __shared__ int bad;
    const int lane = threadIdx.x, n = 7 * d.Nf;
    if (lane == 0) bad = d.ctl_i[EG_I_FAIL];
    __syncthreads();
    int nf = 0;
    for (int r = lane; r < n; r += LM_LANES)
        if (!isfinite(d.xs[r])) nf = 1;
    if (nf) atomicOr(&bad, 1);
    __syncthreads();
    const int failed = bad;
    for (int r = lane; r < n; r += LM_LANES) {
        double x = failed ? d.x[r] : d.xs[r] + 0.0;
        if (d.fix_scale && r % 7 == 6) x = 0.0;
        d.x[r] = x;
        d.sterm[r] = x * (lambda * x + d.b[r]);
    }
    if (lane == 0) d.ctl_i[EG_I_FAIL] = failed;
}

// Sim3(x) * estimate for the free vertices, a copy for the fixed ones
__global__ __launch_bounds__(64) void eg_update_kernel(EgDev d, int cur) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= d.N) return;
    const int f = d.free_index[v];
    double base[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) base[k] = d.est[cur][8 * (size_t)v + k];
    if (f < 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = base[k];
    } else {
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = d.x[7 * f + k];
        lm_sim3_oplus(u, base, out);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) d.est[cur ^ 1][8 * (size_t)v + k] = out[k];
    if (!eg_finite8(out)) atomicOr(&d.ctl_i[EG_I_FLAGS], RFE_EG_FLAG_NONFINITE);
}

// ---------------------------------------------------------------- outputs
__global__ __launch_bounds__(64) void eg_finish_kernel(EgDev d, int cur, double* siw, float* tiw_f32, double* swi, double* swi_ws) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= d.N) return;
    double S[8], inv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = d.est[cur][8 * (size_t)v + k];
    lm_sim3_inverse(S, inv);
#pragma unroll
    for (int k = 0; k < 8; ++k) { siw[8 * (size_t)v + k] = S[k]; swi_ws[8 * (size_t)v + k] = inv[k]; }
    if (swi)
#pragma unroll
        for (int k = 0; k < 8; ++k) swi[8 * (size_t)v + k] = inv[k];
    if (tiw_f32) {
        // Sophus::SE3f(rotation().cast<float>(), translation().cast<float>() / s): the quaternion as cast, the division in float
        const float sf = (float)S[7];
#pragma unroll
        for (int k = 0; k < 4; ++k) tiw_f32[7 * (size_t)v + k] = (float)S[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tiw_f32[7 * (size_t)v + 4 + k] = (float)S[4 + k] / sf;
    }
    if (!eg_finite8(S)) atomicOr(&d.ctl_i[EG_I_FLAGS], RFE_EG_FLAG_NONFINITE);
}

// correctedSwr.map(Srw.map(Xw)) in double from the float point, Srw the INPUT estimate of the reference keyframe; -1: a copy
__global__ __launch_bounds__(LM_LANES) void eg_points_kernel(EgDev d, const double* swi, float* xw_out) {
    const size_t l = (size_t)blockIdx.x * LM_LANES + threadIdx.x;
    if (l >= (size_t)d.L) return;
    const int r = d.point_ref[l];
    const float x0 = d.xw[3 * l], x1 = d.xw[3 * l + 1], x2 = d.xw[3 * l + 2];
    if (r < 0) { xw_out[3 * l] = x0; xw_out[3 * l + 1] = x1; xw_out[3 * l + 2] = x2; return; }
    double Srw[8], Swr[8], a0, a1, a2, b0, b1, b2;
#pragma unroll
    for (int k = 0; k < 8; ++k) { Srw[k] = d.s_est[8 * (size_t)r + k]; Swr[k] = swi[8 * (size_t)r + k]; }
    lm_sim3_map(Srw, (double)x0, (double)x1, (double)x2, a0, a1, a2);
    lm_sim3_map(Swr, a0, a1, a2, b0, b1, b2);
    xw_out[3 * l] = (float)b0; xw_out[3 * l + 1] = (float)b1; xw_out[3 * l + 2] = (float)b2;
}

__global__ __launch_bounds__(LM_LANES) void eg_copy_kernel(const double* src, double* dst, int n) {
    const int i = blockIdx.x * LM_LANES + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

inline dim3 blocks(size_t n, int per = LM_LANES) { return dim3((unsigned)((n + per - 1) / per)); }

}  // namespace

void eg_launch_front(hipStream_t s, const EgDev& d) {
    hipLaunchKernelGGL(eg_front_kernel, dim3(1), dim3(LM_LANES), 0, s, d);
    if (d.L > 0) hipLaunchKernelGGL(eg_check_points_kernel, blocks(d.L), dim3(LM_LANES), 0, s, d);
}

void eg_launch_structure(hipStream_t s, const EgDev& d) {
    if (d.E > 0) hipLaunchKernelGGL(eg_meas_kernel, blocks(d.E), dim3(LM_LANES), 0, s, d);
    if (d.Nf > 0) hipLaunchKernelGGL(eg_incidence_kernel, blocks(d.Nf), dim3(LM_LANES), 0, s, d, 0);
    hipLaunchKernelGGL(eg_symbolic_kernel, dim3(1), dim3(LM_LANES), 0, s, d);
    if (d.Nf > 0) hipLaunchKernelGGL(eg_incidence_kernel, blocks(d.Nf), dim3(LM_LANES), 0, s, d, 1);
    if (d.NP > 7 * d.Nf) hipLaunchKernelGGL(eg_pad_kernel, blocks(d.NP - 7 * d.Nf), dim3(LM_LANES), 0, s, d);
}

void eg_launch_errors(hipStream_t s, const EgDev& d, int cur, bool linearise, bool max_diagonal) {
    if (d.E > 0) hipLaunchKernelGGL(eg_errors_kernel, blocks(d.E), dim3(LM_LANES), 0, s, d, cur, linearise ? 1 : 0);
    if (linearise) {
        if (d.E > 0) hipLaunchKernelGGL(eg_products_kernel, blocks((size_t)d.E * EG_CON), dim3(LM_LANES), 0, s, d);
        if (d.Nf > 0) hipLaunchKernelGGL(eg_assemble_kernel, blocks((size_t)d.Nf * 84), dim3(LM_LANES), 0, s, d);
    }
    hipLaunchKernelGGL(eg_reduce_kernel, dim3(1), dim3(LM_LANES), 0, s, d, (const double*)d.chi2, d.E, (int)EG_D_CHI, max_diagonal ? 1 : 0);
}

void eg_launch_trial(hipStream_t s, const EgDev& d, int cur, double lambda, const int32_t* col_start, const int32_t* row_start) {
    if (d.NP > 0) {
        hipLaunchKernelGGL(eg_trial_begin_kernel, blocks(d.NP), dim3(LM_LANES), 0, s, d);
        for (int J = 0; J < d.NT; ++J)
            hipLaunchKernelGGL(eg_column_kernel, dim3(col_start[J + 1] - col_start[J]), dim3(LM_LANES), 0, s, d, J, lambda);
        hipLaunchKernelGGL(eg_scale_kernel, blocks(d.NP), dim3(LM_LANES), 0, s, d);
        for (int J = d.NT - 1; J >= 0; --J)
            hipLaunchKernelGGL(eg_backward_kernel, dim3(row_start[J + 1] - row_start[J]), dim3(64), 0, s, d, J);
    } else {
        (void)hipMemsetAsync(d.ctl_i + EG_I_FAIL, 0, sizeof(int32_t), s);
    }
    hipLaunchKernelGGL(eg_commit_kernel, dim3(1), dim3(LM_LANES), 0, s, d, lambda);
    hipLaunchKernelGGL(eg_update_kernel, blocks(d.N, 64), dim3(64), 0, s, d, cur);
    eg_launch_errors(s, d, cur ^ 1, false, false);
    hipLaunchKernelGGL(eg_reduce_kernel, dim3(1), dim3(LM_LANES), 0, s, d, (const double*)d.sterm, 7 * d.Nf, (int)EG_D_SCALE, 0);
}

void eg_launch_finish(hipStream_t s, const EgDev& d, int cur, double* siw, float* tiw_f32, double* swi, float* xw_out, double* chi2) {
    eg_launch_errors(s, d, cur, false, false);
    // est[cur ^ 1] is free now: it takes the inverses the point correction reads
    hipLaunchKernelGGL(eg_finish_kernel, blocks(d.N, 64), dim3(64), 0, s, d, cur, siw, tiw_f32, swi, d.est[cur ^ 1]);
    if (d.L > 0) hipLaunchKernelGGL(eg_points_kernel, blocks(d.L), dim3(LM_LANES), 0, s, d, (const double*)d.est[cur ^ 1], xw_out);
    if (chi2 && d.E > 0) hipLaunchKernelGGL(eg_copy_kernel, blocks(d.E), dim3(LM_LANES), 0, s, (const double*)d.chi2, chi2, d.E);
}

}  // namespace rfe
