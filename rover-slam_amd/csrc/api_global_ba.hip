// api_global_ba.hip -- C ABI of librover_fe.so: Optimizer::GlobalBundleAdjustemnt / BundleAdjustment, one problem per call (global_ba.hip,
// DESIGN.md 6n).  The Levenberg-Marquardt loop of optimization_algorithm_levenberg.cpp:61-169 and sparse_optimizer.cpp's optimize() runs
// HERE, on the host: each stage is a plain launch on the ctx stream, each linearisation and each trial costs one 128-byte pinned read, and
// `stop` is read where terminate() is.  The front costs three more: the tables' verdict with the number of free keyframes, the number of
// Schur pairs and non-empty blocks (from which the pair workspace is sized, and a problem over the cap refused), then the tile lists'
// offsets, from which the launches of the factorisation are sized.
#include <float.h>
#include <math.h>
#include <string.h>
#include "api_internal.h"

using namespace rfe;

namespace {

constexpr int GBA_MAX_NT = RFE_GBA_MAX_KF / GBA_TILE_V;
struct GbaCtl { double d[GBA_CTL_D]; int32_t i[GBA_CTL_I]; };
struct GbaPin { GbaCtl ctl; int32_t stats[8]; int32_t col_start[GBA_MAX_NT + 1], row_start[GBA_MAX_NT + 1]; double trace[RFE_GBA_MAX_ITERATIONS * 4]; };

// what is sized from the inputs alone; everything sized from the free keyframes is carved for K of them
void gba_layout(Bump& a, GbaDev& d) {
    const size_t E = std::max(d.E, 1), L = std::max(d.L, 1), K = d.K, NT = (K + GBA_TILE_V - 1) / GBA_TILE_V, NP = NT * GBA_TILE;
    GbaCtl* ctl = a.take<GbaCtl>(1);
    d.ctl_d = ctl ? ctl->d : nullptr; d.ctl_i = ctl ? ctl->i : nullptr;
    for (int b = 0; b < 2; ++b) { d.pose[b] = a.take<double>(K * 7); d.pt[b] = a.take<double>(L * 3); }
    d.free_index = a.take<int32_t>(K); d.free_list = a.take<int32_t>(K);
    d.pt_start = a.take<int32_t>(L + 1); d.pose_start = a.take<int32_t>(K + 1); d.pose_cnt = a.take<int32_t>(K);
    d.pose_list = a.take<int32_t>(E); d.pose_tmp = a.take<int32_t>(E);
    d.key_cnt = a.take<int32_t>(K * K); d.key_start = a.take<int32_t>(K * K);
    d.blk_key = a.take<int32_t>(K * (K + 1) / 2); d.blk_start = a.take<int32_t>(K * (K + 1) / 2 + 1);
    d.col_start = a.take<int32_t>(NT + 1); d.row_start = a.take<int32_t>(NT + 1);
    d.col_tiles = a.take<int32_t>(NT * (NT + 1) / 2); d.row_tiles = a.take<int32_t>(NT * (NT + 1) / 2);
    d.fill = a.take<uint8_t>(NT * NT);
    d.lin = a.take<double>(E * LBA_LIN); d.chi2 = a.take<double>(E); d.rho0 = a.take<double>(E);
    d.Hll = a.take<double>(L * 6); d.bl = a.take<double>(L * 3); d.Dinv = a.take<double>(L * 9); d.db = a.take<double>(L * 3); d.xl = a.take<double>(L * 3);
    d.Hpp = a.take<double>(K * 21); d.bp = a.take<double>(K * 6); d.xp = a.take<double>(K * 6);
    d.BDinv = a.take<double>(E * 18); d.Bdb = a.take<double>(E * 6); d.sterm = a.take<double>(K * 6 + 3 * L);
    d.b = a.take<double>(NP); d.z = a.take<double>(NP); d.y = a.take<double>(NP); d.xs = a.take<double>(NP); d.dvec = a.take<double>(NP);
}

int gba_check(rfe_ctx* c, const rfe_global_ba_params& p, const void* kf_pose, const void* kf_cam, const void* kf_nlevels, const void* kf_sigma2,
              const void* kf_feat_off, const void* fixed, const void* kpts, const void* xw, const void* ep, const void* ek, const void* ef, int K,
              int L, int E, int Nf, const void* pose, const void* point, const void* included, const void* stats) {
    if (K < 1 || K > RFE_GBA_MAX_KF) return fail(c, RFE_ERR_INVALID, "global_ba: K outside 1..1024");
    if (L < 0 || L > RFE_GBA_MAX_POINTS) return fail(c, RFE_ERR_INVALID, "global_ba: L outside 0..262144");
    if (E < 0 || E > RFE_GBA_MAX_EDGES) return fail(c, RFE_ERR_INVALID, "global_ba: E outside 0..2097152");
    if (Nf < 0) return fail(c, RFE_ERR_INVALID, "global_ba: negative Nf");
    if (p.iterations < 0 || p.iterations > RFE_GBA_MAX_ITERATIONS) return fail(c, RFE_ERR_INVALID, "global_ba: iterations outside 0..64");
    if (p.max_trials < 0) return fail(c, RFE_ERR_INVALID, "global_ba: negative max_trials");
    if (!(isfinite(p.user_lambda_init) && isfinite(p.huber2_mono) && isfinite(p.huber2_stereo)))
        return fail(c, RFE_ERR_INVALID, "global_ba: non-finite huber2 or user_lambda_init");
    if (!kf_pose || !kf_cam || !kf_nlevels || !kf_sigma2 || !kf_feat_off || !fixed || !stats || !pose || (L > 0 && (!xw || !point || !included)) ||
        (E > 0 && (!ep || !ek || !ef)) || (Nf > 0 && !kpts))
        return fail(c, RFE_ERR_INVALID, "global_ba: null pointer");
    return RFE_OK;
}

}  // namespace

extern "C" int rfe_global_ba_dev(rfe_ctx* c, rfe_global_ba_params prm, const float* kf_pose, const float* kf_cam, const int32_t* kf_nlevels,
                                 const float* kf_sigma2, const int32_t* kf_feat_off, const uint8_t* fixed, const float* kpts, const int32_t* octave,
                                 const float* uright, const float* xw, const int32_t* edge_point, const int32_t* edge_kf, const int32_t* edge_feat,
                                 int K, int L, int E, int Nf, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* included,
                                 double* chi2, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = gba_check(c, prm, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, fixed, kpts, xw, edge_point, edge_kf, edge_feat, K, L, E, Nf,
                       pose, point, included, stats);
    if (rc) return rc;
    const int stop_after = c->gba_stop_after;       // rfe_k_global_ba_stop_after: one shot, taken by the first call that passes its checks
    c->gba_stop_after = 0;
    RFE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    GbaDev d;
    memset(&d, 0, sizeof d);
    d.kf_pose = kf_pose; d.kf_cam = kf_cam; d.kf_sigma2 = kf_sigma2; d.kpts = kpts; d.uright = uright; d.xw = xw; d.kf_nlevels = kf_nlevels;
    d.kf_feat_off = kf_feat_off; d.octave = octave; d.edge_point = edge_point; d.edge_kf = edge_kf; d.edge_feat = edge_feat; d.fixed = fixed;
    d.K = K; d.L = L; d.E = E; d.Nf = Nf; d.robust = prm.robust != 0;
    // `const float thHuber2D = sqrt(5.99)`; RobustKernelHuber keeps delta as a double and dsqr in a float member, as 6l
    d.delta_mono = (double)(float)sqrt(prm.huber2_mono); d.dsqr_mono = (double)(float)(d.delta_mono * d.delta_mono);
    d.delta_stereo = (double)(float)sqrt(prm.huber2_stereo); d.dsqr_stereo = (double)(float)(d.delta_stereo * d.delta_stereo);
    if ((rc = ws_carve(c, &c->ws_gba, &c->ws_gba_bytes, [&](Bump& a) { gba_layout(a, d); }))) return rc;
    if (!c->h_gba) {
        const hipError_t e = hipHostMalloc(&c->h_gba, sizeof(GbaPin), hipHostMallocDefault);
        if (e != hipSuccess) { c->h_gba = nullptr; return fail(c, RFE_ERR_OOM, std::string("global_ba: hipHostMalloc: ") + hipGetErrorString(e)); }
    }
    GbaPin* pin = (GbaPin*)c->h_gba;
    auto read_ctl = [&]() -> int {
        RFE_HIP(c, hipMemcpyAsync(&pin->ctl, d.ctl_d, sizeof(GbaCtl), hipMemcpyDeviceToHost, s));
        RFE_HIP(c, hipStreamSynchronize(s));
        return RFE_OK;
    };
    auto stopped = [&]() { return prm.stop && *prm.stop; };

    // the first kernels: validation; their verdict is read before anything indexes by an edge or a keyframe offset
    RFE_HIP(c, hipMemsetAsync(d.ctl_d, 0, sizeof(GbaCtl), s));
    { ProfScope ps(c, "gba_validate"); gba_launch_validate(s, d); }
    if ((rc = read_ctl())) return rc;
    if (pin->ctl.i[GBA_I_STATUS]) {
        const int st = pin->ctl.i[GBA_I_STATUS];
        return fail(c, RFE_ERR_INVALID, st & LBA_BAD_KF      ? "global_ba: nlevels outside 1..16 or kf_feat_off not ascending inside 0..Nf"
                                        : st & LBA_BAD_RANGE ? "global_ba: edge index out of range"
                                                             : "global_ba: edges not strictly ascending in (point, keyframe)");
    }
    d.P = pin->ctl.i[GBA_I_NFREE];
    d.NT = (d.P + GBA_TILE_V - 1) / GBA_TILE_V; d.NP = d.NT * GBA_TILE;
    // structure, once per call: the counts, then -- the pair workspace sized from them -- the lists, the fill and the cleared tiles
    { ProfScope ps(c, "gba_structure"); gba_launch_count(s, d); }
    if ((rc = read_ctl())) return rc;
    const int n_pairs = pin->ctl.i[GBA_I_NPAIRS];
    d.NB = pin->ctl.i[GBA_I_NBLOCKS];
    if (n_pairs < 0 || n_pairs > RFE_GBA_MAX_PAIRS) return fail(c, RFE_ERR_INVALID, "global_ba: more than 33554432 Schur pair entries");
    const size_t pair_bytes = al((size_t)std::max(n_pairs, 1) * sizeof(unsigned long long));
    if ((rc = ensure_ws(c, &c->ws_gba_pairs, &c->ws_gba_pairs_bytes, 2 * pair_bytes))) return rc;
    d.pairs = (unsigned long long*)c->ws_gba_pairs; d.pairs_tmp = (unsigned long long*)((char*)c->ws_gba_pairs + pair_bytes);
    if ((rc = ensure_ws(c, &c->ws_gba_mat, &c->ws_gba_mat_bytes, al(std::max((size_t)d.NP * d.NP * sizeof(double), (size_t)1))))) return rc;
    d.mat = (double*)c->ws_gba_mat;
    RFE_HIP(c, hipMemsetAsync(d.xp, 0, (size_t)std::max(6 * d.P, 1) * sizeof(double), s));      // g2o's x starts at zero: a failed first solve updates by it
    RFE_HIP(c, hipMemsetAsync(d.xl, 0, (size_t)std::max(3 * L, 1) * sizeof(double), s));
    { ProfScope ps(c, "gba_structure"); gba_launch_structure(s, d); }
    int tiles = 0;
    if (d.P > 0) {
        RFE_HIP(c, hipMemcpyAsync(pin->col_start, d.col_start, (size_t)(d.NT + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RFE_HIP(c, hipMemcpyAsync(pin->row_start, d.row_start, (size_t)(d.NT + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if ((rc = read_ctl())) return rc;
        tiles = pin->ctl.i[GBA_I_TILES];
    }

    const int max_trials = prm.max_trials > 0 ? prm.max_trials : 10;
    int cur = 0, iters = 0, trials = 0, rejected = 0, failed = 0, flags = 0;
    bool ended_rejected = false;
    double lambda = 0.0, ni = 2.0;
    int nbad = 0;
    memset(pin->trace, 0, sizeof pin->trace);
    for (int it = 0; it < prm.iterations; ++it) {
        if (stopped()) { flags |= RFE_GBA_FLAG_STOPPED; break; }
        ++iters;
        const bool want_max = it == 0 && !(prm.user_lambda_init > 0);
        { ProfScope ps(c, "gba_linearise"); gba_launch_errors(s, d, cur, true, want_max); }
        if ((rc = read_ctl())) return rc;
        double current = pin->ctl.d[GBA_D_CHI];
        const double ini = current;
        if (it == 0) { lambda = prm.user_lambda_init > 0 ? prm.user_lambda_init : 1e-5 * pin->ctl.d[GBA_D_MAXDIAG]; ni = 2.0; nbad = 0; }
        double rho = 0.0;
        int qmax = 0;
        bool stop_seen = false;
        do {
            ++trials;
            { ProfScope ps(c, "gba_trial"); gba_launch_trial(s, d, cur, lambda, pin->col_start, pin->row_start); }
            { ProfScope ps(c, "gba_errors"); gba_launch_errors(s, d, cur ^ 1, false, false); }
            if ((rc = read_ctl())) return rc;
            double temp = pin->ctl.d[GBA_D_CHI];
            if (pin->ctl.i[GBA_I_FAIL]) { temp = DBL_MAX; ++failed; flags |= RFE_GBA_FLAG_SOLVE_FAILED; }
            const double scale = pin->ctl.d[GBA_D_SCALE] + 1e-3;
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
                ended_rejected = true;               // pop: the estimate stays; the edges keep the trial's errors
            }
            ++qmax;
            if (prm.stop && stop_after > 0 && trials == stop_after) *const_cast<volatile uint8_t*>(prm.stop) = 1;
            stop_seen = stopped();
        } while (rho < 0 && qmax < max_trials && !stop_seen);
        if (stop_seen) flags |= RFE_GBA_FLAG_STOPPED;
        double* tr = pin->trace + 4 * it;
        tr[0] = (double)qmax; tr[1] = lambda; tr[2] = current; tr[3] = 0.0;
        if (qmax == max_trials || rho == 0) break;
        if ((ini - current) * 1e3 < ini) ++nbad; else nbad = 0;
        if (nbad >= 3) break;
    }
    if (iters == 0) {
        flags |= RFE_GBA_FLAG_NO_ITERATION;
        ProfScope ps(c, "gba_errors");
        gba_launch_errors(s, d, cur, false, false);
    }
    if (ended_rejected) flags |= RFE_GBA_FLAG_ENDED_REJECTED;
    { ProfScope ps(c, "gba_finish"); gba_launch_finish(s, d, cur, pose, pose_f32, point, point_f32, included, chi2); }
    if ((rc = read_ctl())) return rc;
    flags |= pin->ctl.i[GBA_I_FLAGS];
    const int32_t st[8] = {iters, trials, rejected, failed, flags, d.P, tiles, d.NT * (d.NT + 1) / 2};
    memcpy(pin->stats, st, sizeof st);
    RFE_HIP(c, hipMemcpyAsync(stats, pin->stats, sizeof st, hipMemcpyHostToDevice, s));
    if (trace && prm.iterations > 0)
        RFE_HIP(c, hipMemcpyAsync(trace, pin->trace, (size_t)prm.iterations * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    RFE_HIP(c, hipStreamSynchronize(s));
    RFE_HIP(c, hipGetLastError());
    return iters;
}

// test hook: the NEXT rfe_global_ba / _dev of this ctx that is given a stop pointer writes 1 through it behind its `trials`-th trial,
// in front of the read that follows the trial -- the one way to place "pbStopFlag set while the optimisation runs" at a known trial
extern "C" int rfe_k_global_ba_stop_after(rfe_ctx* c, int trials) {
    if (!c) return RFE_ERR_INVALID;
    c->gba_stop_after = trials > 0 ? trials : 0;
    return RFE_OK;
}

extern "C" int rfe_global_ba(rfe_ctx* c, rfe_global_ba_params prm, const float* kf_pose, const float* kf_cam, const int32_t* kf_nlevels,
                             const float* kf_sigma2, const int32_t* kf_feat_off, const uint8_t* fixed, const float* kpts, const int32_t* octave,
                             const float* uright, const float* xw, const int32_t* edge_point, const int32_t* edge_kf, const int32_t* edge_feat, int K,
                             int L, int E, int Nf, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* included, double* chi2,
                             double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = gba_check(c, prm, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, fixed, kpts, xw, edge_point, edge_kf, edge_feat, K, L, E, Nf,
                       pose, point, included, stats);
    if (rc) return rc;
    for (int k = 0; k < K; ++k)
        if (kf_nlevels[k] < 1 || kf_nlevels[k] > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, "global_ba: nlevels outside 1..16");
    for (int k = 0; k <= K; ++k)
        if (kf_feat_off[k] < 0 || kf_feat_off[k] > Nf || (k < K && kf_feat_off[k + 1] < kf_feat_off[k]))
            return fail(c, RFE_ERR_INVALID, "global_ba: kf_feat_off not ascending inside 0..Nf");
    for (int e = 0; e < E; ++e) {
        const int p = edge_point[e], k = edge_kf[e], f = edge_feat[e];
        if (p < 0 || p >= L || k < 0 || k >= K || f < 0 || f >= kf_feat_off[k + 1] - kf_feat_off[k])
            return fail(c, RFE_ERR_INVALID, "global_ba: edge index out of range");
        if (e > 0 && !(edge_point[e - 1] < p || (edge_point[e - 1] == p && edge_kf[e - 1] < k)))
            return fail(c, RFE_ERR_INVALID, "global_ba: edges not strictly ascending in (point, keyframe)");
    }
    // the pair cap, before anything is staged: sum over the points of n (n + 1) / 2, n the point's edges on free keyframes
    {
        long long pairs = 0, n = 0;
        for (int e = 0; e < E; ++e) {
            if (e > 0 && edge_point[e] != edge_point[e - 1]) { pairs += n * (n + 1) / 2; n = 0; }
            if (!fixed[edge_kf[e]]) ++n;
        }
        pairs += n * (n + 1) / 2;
        if (pairs > RFE_GBA_MAX_PAIRS) return fail(c, RFE_ERR_INVALID, "global_ba: more than 33554432 Schur pair entries");
    }
    RFE_HIP(c, hipSetDevice(c->device));
    float *dkp, *dkc, *dks, *dk, *du, *dx, *dpf, *dqf; int32_t *dnl, *dfo, *doc, *dep, *dek, *def, *dst; double *dpo, *dpt, *dc, *dtr; uint8_t *dfx, *din;
    HostIo io(c, HostIo::DIRECT);
    io.in(dkp, kf_pose, (size_t)K * 7); io.in(dkc, kf_cam, (size_t)K * 5); io.in(dnl, kf_nlevels, (size_t)K);
    io.in(dks, kf_sigma2, (size_t)K * RFE_MAX_LEVELS); io.in(dfo, kf_feat_off, (size_t)K + 1); io.in(dfx, fixed, (size_t)K);
    io.in(dk, kpts, (size_t)Nf * 2); io.in_opt(doc, octave, (size_t)Nf); io.in_opt(du, uright, (size_t)Nf); io.in(dx, xw, (size_t)L * 3);
    io.in(dep, edge_point, (size_t)E); io.in(dek, edge_kf, (size_t)E); io.in(def, edge_feat, (size_t)E);
    io.out(dpo, pose, (size_t)K * 7); io.out_opt(dpf, pose_f32, (size_t)K * 7); io.out(dpt, point, (size_t)L * 3); io.out_opt(dqf, point_f32, (size_t)L * 3);
    io.out(din, included, (size_t)L); io.out_opt(dc, chi2, (size_t)E); io.out_opt(dtr, trace, (size_t)prm.iterations * 4); io.out(dst, stats, 8);
    if ((rc = io.upload())) return rc;
    const int iters = rfe_global_ba_dev(c, prm, dkp, dkc, dnl, dks, dfo, dfx, dk, doc, du, dx, dep, dek, def, K, L, E, Nf, dpo, dpf, dpt, dqf, din, dc,
                                        dtr, dst);
    if (iters < 0) return iters;
    if ((rc = io.download())) return rc;
    return iters;
}
