// api_essential_graph.hip -- C ABI of librover_fe.so: Optimizer::OptimizeEssentialGraph, one pose graph per call (essential_graph.hip,
// DESIGN.md 6m).  The Levenberg-Marquardt loop of optimization_algorithm_levenberg.cpp:61-169 and sparse_optimizer.cpp's optimize() runs
// HERE, on the host: each stage is a plain launch on the ctx stream and each linearisation and each trial costs one 128-byte pinned read
// (chi2, computeScale's sum, the solve's verdict).  The front costs two more: the status word with the number of free vertices, then the
// tile lists' offsets, from which the launches of the factorisation are sized.
#include <float.h>
#include <math.h>
#include <string.h>
#include "api_internal.h"

using namespace rfe;

namespace {

constexpr int EG_MAX_NT = RFE_EG_MAX_KF / EG_TILE_V;
struct EgCtl { double d[EG_CTL_D]; int32_t i[EG_CTL_I]; };
struct EgPin { EgCtl ctl; int32_t stats[8]; int32_t col_start[EG_MAX_NT + 1], row_start[EG_MAX_NT + 1]; double trace[RFE_EG_MAX_ITERATIONS * 4]; };

// what is sized from the inputs alone; the vectors and lists sized from Nf are carved for N free vertices
void eg_layout(Bump& a, EgDev& d) {
    const size_t N = d.N, E = std::max(d.E, 1), NT = (N + EG_TILE_V - 1) / EG_TILE_V, NP = NT * EG_TILE;
    EgCtl* ctl = a.take<EgCtl>(1);
    d.ctl_d = ctl ? ctl->d : nullptr; d.ctl_i = ctl ? ctl->i : nullptr;
    for (int b = 0; b < 2; ++b) d.est[b] = a.take<double>(N * 8);
    d.meas = a.take<double>(E * 8); d.pert = a.take<double>(14 * 8);
    d.free_index = a.take<int32_t>(N); d.free_list = a.take<int32_t>(N); d.inc_start = a.take<int32_t>(N + 1); d.inc_list = a.take<int32_t>(2 * E);
    d.col_start = a.take<int32_t>(NT + 1); d.row_start = a.take<int32_t>(NT + 1);
    d.col_tiles = a.take<int32_t>(NT * (NT + 1) / 2); d.row_tiles = a.take<int32_t>(NT * (NT + 1) / 2);
    d.fill = a.take<uint8_t>(NT * NT);
    d.jac = a.take<double>(E * EG_JAC); d.con = a.take<double>(E * EG_CON); d.chi2 = a.take<double>(E);
    d.b = a.take<double>(NP); d.x = a.take<double>(NP); d.z = a.take<double>(NP); d.y = a.take<double>(NP); d.xs = a.take<double>(NP);
    d.dvec = a.take<double>(NP); d.sterm = a.take<double>(NP);
}

int eg_check(rfe_ctx* c, const rfe_essential_graph_params& p, const void* s_est, const void* s_meas, const void* fixed, const void* ei,
             const void* ej, const void* src, const void* xw, const void* ref, int N, int E, int L, const void* siw, const void* xw_out,
             const void* stats) {
    if (N < 1 || N > RFE_EG_MAX_KF) return fail(c, RFE_ERR_INVALID, "essential_graph: N outside 1..1024");
    if (E < 0 || E > RFE_EG_MAX_EDGES) return fail(c, RFE_ERR_INVALID, "essential_graph: E outside 0..16384");
    if (L < 0 || L > RFE_EG_MAX_POINTS) return fail(c, RFE_ERR_INVALID, "essential_graph: L outside 0..1048576");
    if (p.iterations < 0 || p.iterations > RFE_EG_MAX_ITERATIONS) return fail(c, RFE_ERR_INVALID, "essential_graph: iterations outside 0..64");
    if (p.max_trials < 0) return fail(c, RFE_ERR_INVALID, "essential_graph: negative max_trials");
    if (!isfinite(p.user_lambda_init)) return fail(c, RFE_ERR_INVALID, "essential_graph: non-finite user_lambda_init");
    if (!s_est || !s_meas || !fixed || !siw || !stats || (E > 0 && (!ei || !ej || !src)) || (L > 0 && (!xw || !ref || !xw_out)))
        return fail(c, RFE_ERR_INVALID, "essential_graph: null pointer");
    return RFE_OK;
}

}  // namespace

extern "C" int rfe_essential_graph_dev(rfe_ctx* c, rfe_essential_graph_params prm, const double* s_est, const double* s_meas, const uint8_t* fixed,
                                       const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_from_est, const float* xw,
                                       const int32_t* point_ref, int N, int E, int L, double* siw, float* tiw_f32, double* swi, float* xw_out,
                                       double* chi2, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = eg_check(c, prm, s_est, s_meas, fixed, edge_i, edge_j, edge_from_est, xw, point_ref, N, E, L, siw, xw_out, stats);
    if (rc) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    EgDev d;
    memset(&d, 0, sizeof d);
    d.s_est = s_est; d.s_meas = s_meas; d.fixed = fixed; d.edge_src = edge_from_est; d.edge_i = edge_i; d.edge_j = edge_j; d.point_ref = point_ref;
    d.xw = xw; d.N = N; d.E = E; d.L = L; d.fix_scale = prm.fix_scale != 0;
    if ((rc = ws_carve(c, &c->ws_eg, &c->ws_eg_bytes, [&](Bump& a) { eg_layout(a, d); }))) return rc;
    if (!c->h_eg) {
        const hipError_t e = hipHostMalloc(&c->h_eg, sizeof(EgPin), hipHostMallocDefault);
        if (e != hipSuccess) { c->h_eg = nullptr; return fail(c, RFE_ERR_OOM, std::string("essential_graph: hipHostMalloc: ") + hipGetErrorString(e)); }
    }
    EgPin* pin = (EgPin*)c->h_eg;
    auto read_ctl = [&]() -> int {
        RFE_HIP(c, hipMemcpyAsync(&pin->ctl, d.ctl_d, sizeof(EgCtl), hipMemcpyDeviceToHost, s));
        RFE_HIP(c, hipStreamSynchronize(s));
        return RFE_OK;
    };

    // the first kernels: validation; their verdict is read before anything indexes by an edge
    RFE_HIP(c, hipMemsetAsync(d.ctl_d, 0, sizeof(EgCtl), s));
    { ProfScope ps(c, "eg_front"); eg_launch_front(s, d); }
    if ((rc = read_ctl())) return rc;
    if (pin->ctl.i[EG_I_STATUS]) {
        const int st = pin->ctl.i[EG_I_STATUS];
        return fail(c, RFE_ERR_INVALID, st & EG_BAD_RANGE   ? "essential_graph: edge index out of range or an edge from a keyframe to itself"
                                        : st & EG_BAD_ORDER ? "essential_graph: edges not ascending in (i, j)"
                                                            : "essential_graph: point_ref outside -1..N-1");
    }
    d.Nf = pin->ctl.i[EG_I_NFREE];
    d.NT = (d.Nf + EG_TILE_V - 1) / EG_TILE_V; d.NP = d.NT * EG_TILE;
    // the matrix, sized from Nf: zero everywhere (a tile that only fills in reads H = +0.0), then the unit diagonal of the padding
    const size_t mat_bytes = (size_t)d.NP * d.NP * sizeof(double);
    if ((rc = ensure_ws(c, &c->ws_eg_mat, &c->ws_eg_mat_bytes, al(std::max(mat_bytes, (size_t)1))))) return rc;
    d.mat = (double*)c->ws_eg_mat;
    if (mat_bytes) RFE_HIP(c, hipMemsetAsync(d.mat, 0, mat_bytes, s));
    RFE_HIP(c, hipMemsetAsync(d.x, 0, (size_t)std::max(d.NP, 1) * sizeof(double), s));      // g2o's x starts at zero: a failed first solve updates by it
    { ProfScope ps(c, "eg_structure"); eg_launch_structure(s, d); }
    RFE_HIP(c, hipMemcpyAsync(pin->col_start, d.col_start, (size_t)(d.NT + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RFE_HIP(c, hipMemcpyAsync(pin->row_start, d.row_start, (size_t)(d.NT + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if ((rc = read_ctl())) return rc;
    const int tiles = pin->ctl.i[EG_I_TILES];

    const int max_trials = prm.max_trials > 0 ? prm.max_trials : 10;
    int cur = 0, iters = 0, trials = 0, rejected = 0, failed = 0, flags = 0;
    bool ended_rejected = false;
    double lambda = 0.0, ni = 2.0;
    int nbad = 0;
    memset(pin->trace, 0, sizeof pin->trace);
    for (int it = 0; it < prm.iterations; ++it) {
        ++iters;
        const bool want_max = it == 0 && !(prm.user_lambda_init > 0);
        { ProfScope ps(c, "eg_linearise"); eg_launch_errors(s, d, cur, true, want_max); }
        if ((rc = read_ctl())) return rc;
        double current = pin->ctl.d[EG_D_CHI];
        const double ini = current;
        if (it == 0) { lambda = prm.user_lambda_init > 0 ? prm.user_lambda_init : 1e-5 * pin->ctl.d[EG_D_MAXDIAG]; ni = 2.0; nbad = 0; }
        double rho = 0.0;
        int qmax = 0;
        do {
            ++trials;
            { ProfScope ps(c, "eg_trial"); eg_launch_trial(s, d, cur, lambda, pin->col_start, pin->row_start); }
            if ((rc = read_ctl())) return rc;
            double temp = pin->ctl.d[EG_D_CHI];
            if (pin->ctl.i[EG_I_FAIL]) { temp = DBL_MAX; ++failed; flags |= RFE_EG_FLAG_SOLVE_FAILED; }
            const double scale = pin->ctl.d[EG_D_SCALE] + 1e-3;
            rho = (current - temp) / scale;
            if (rho > 0 && isfinite(temp)) {
                const double v = 2 * rho - 1;
                double alpha = 1.0 - (v * v) * v;
                alpha = ((2.0 / 3.0) < alpha) ? (2.0 / 3.0) : alpha;
                lambda = lambda * (((1.0 / 3.0) < alpha) ? alpha : (1.0 / 3.0));
                ni = 2.0;
                current = temp;
                cur ^= 1;                            // discardTop: the trial estimate is the estimate
                ended_rejected = false;
            } else {
                lambda = lambda * ni;
                ni = ni * 2;
                ++rejected;
                ended_rejected = true;               // pop: the estimate stays
            }
            ++qmax;
        } while (rho < 0 && qmax < max_trials);
        double* tr = pin->trace + 4 * it;
        tr[0] = (double)qmax; tr[1] = lambda; tr[2] = current; tr[3] = 0.0;
        if (qmax == max_trials || rho == 0) break;
        if ((ini - current) * 1e3 < ini) ++nbad; else nbad = 0;
        if (nbad >= 3) break;
    }
    if (iters == 0) flags |= RFE_EG_FLAG_NO_ITERATION;
    if (ended_rejected) flags |= RFE_EG_FLAG_ENDED_REJECTED;
    { ProfScope ps(c, "eg_finish"); eg_launch_finish(s, d, cur, siw, tiw_f32, swi, xw_out, chi2); }
    if ((rc = read_ctl())) return rc;
    flags |= pin->ctl.i[EG_I_FLAGS];
    const int32_t st[8] = {iters, trials, rejected, failed, flags, d.Nf, tiles, d.NT * (d.NT + 1) / 2};
    memcpy(pin->stats, st, sizeof st);
    RFE_HIP(c, hipMemcpyAsync(stats, pin->stats, sizeof st, hipMemcpyHostToDevice, s));
    if (trace && prm.iterations > 0)
        RFE_HIP(c, hipMemcpyAsync(trace, pin->trace, (size_t)prm.iterations * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    RFE_HIP(c, hipStreamSynchronize(s));
    RFE_HIP(c, hipGetLastError());
    return iters;
}

extern "C" int rfe_essential_graph(rfe_ctx* c, rfe_essential_graph_params prm, const double* s_est, const double* s_meas, const uint8_t* fixed,
                                   const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_from_est, const float* xw,
                                   const int32_t* point_ref, int N, int E, int L, double* siw, float* tiw_f32, double* swi, float* xw_out,
                                   double* chi2, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = eg_check(c, prm, s_est, s_meas, fixed, edge_i, edge_j, edge_from_est, xw, point_ref, N, E, L, siw, xw_out, stats);
    if (rc) return rc;
    for (int e = 0; e < E; ++e) {
        const int i = edge_i[e], j = edge_j[e];
        if (i < 0 || i >= N || j < 0 || j >= N || i == j)
            return fail(c, RFE_ERR_INVALID, "essential_graph: edge index out of range or an edge from a keyframe to itself");
        if (e > 0 && (edge_i[e - 1] > i || (edge_i[e - 1] == i && edge_j[e - 1] > j)))
            return fail(c, RFE_ERR_INVALID, "essential_graph: edges not ascending in (i, j)");
    }
    for (int l = 0; l < L; ++l)
        if (point_ref[l] < -1 || point_ref[l] >= N) return fail(c, RFE_ERR_INVALID, "essential_graph: point_ref outside -1..N-1");
    RFE_HIP(c, hipSetDevice(c->device));
    double *de, *dm, *dsiw, *dswi, *dchi, *dtr; uint8_t *dfx, *dsrc; int32_t *dei, *dej, *dref, *dst; float *dxw, *dtiw, *dxo;
    HostIo io(c, HostIo::DIRECT);
    io.in(de, s_est, (size_t)N * 8); io.in(dm, s_meas, (size_t)N * 8); io.in(dfx, fixed, (size_t)N);
    io.in_opt(dei, edge_i, (size_t)E); io.in_opt(dej, edge_j, (size_t)E); io.in_opt(dsrc, edge_from_est, (size_t)E);
    io.in_opt(dxw, xw, (size_t)L * 3); io.in_opt(dref, point_ref, (size_t)L);
    io.out(dsiw, siw, (size_t)N * 8); io.out_opt(dtiw, tiw_f32, (size_t)N * 7); io.out_opt(dswi, swi, (size_t)N * 8);
    io.out_opt(dxo, xw_out, (size_t)L * 3); io.out_opt(dchi, chi2, (size_t)E); io.out_opt(dtr, trace, (size_t)prm.iterations * 4); io.out(dst, stats, 8);
    if ((rc = io.upload())) return rc;
    const int iters = rfe_essential_graph_dev(c, prm, de, dm, dfx, dei, dej, dsrc, dxw, dref, N, E, L, dsiw, dtiw, dswi, dxo, dchi, dtr, dst);
    if (iters < 0) return iters;
    if ((rc = io.download())) return rc;
    return iters;
}
