// api_local_ba.hip -- C ABI of librover_fe.so: Optimizer::LocalBundleAdjustment, one problem per call (local_ba.hip).
// The Levenberg-Marquardt loop of optimization_algorithm_levenberg.cpp:61-169 and sparse_optimizer.cpp's optimize() runs HERE, on the
// host: each stage is a plain launch on the ctx stream, each trial costs one 128-byte pinned read (tempChi, computeScale's sum, the
// solve's verdict), and `stop` is read where terminate() is.
#include <float.h>
#include <math.h>
#include <string.h>
#include "api_internal.h"

using namespace rfe;

namespace {

struct LbaCtl { double d[LBA_CTL_D]; int32_t i[LBA_CTL_I]; };
struct LbaPin { LbaCtl ctl; int32_t stats[8]; double trace[RFE_LBA_MAX_ITERATIONS * 4]; };

void lba_layout(Bump& a, LbaDev& d) {
    const size_t E = std::max(d.E, 1), L = std::max(d.L, 1), P = std::max(d.P, 1), K = d.K, NB = std::max(d.NB, 1), n = 6 * P;
    LbaCtl* ctl = a.take<LbaCtl>(1);
    d.ctl_d = ctl ? ctl->d : nullptr; d.ctl_i = ctl ? ctl->i : nullptr;
    for (int b = 0; b < 2; ++b) { d.pose[b] = a.take<double>(K * 7); d.pt[b] = a.take<double>(L * 3); }
    d.pt_start = a.take<int32_t>(L + 1); d.pose_start = a.take<int32_t>(P + 1); d.pose_cnt = a.take<int32_t>(P); d.pose_list = a.take<int32_t>(E);
    d.blk_start = a.take<int32_t>(NB + 1); d.blk_cnt = a.take<int32_t>(NB);
    d.lin = a.take<double>(E * LBA_LIN); d.chi2 = a.take<double>(E); d.rho0 = a.take<double>(E);
    d.Hll = a.take<double>(L * 6); d.bl = a.take<double>(L * 3); d.Dinv = a.take<double>(L * 9); d.db = a.take<double>(L * 3); d.xl = a.take<double>(L * 3);
    d.Hpp = a.take<double>(P * 21); d.bp = a.take<double>(P * 6); d.bs = a.take<double>(n); d.xp = a.take<double>(n);
    d.BDinv = a.take<double>(E * 18); d.Bdb = a.take<double>(E * 6); d.S = a.take<double>(n * n); d.sterm = a.take<double>(n + 3 * L);
}

int lba_check(rfe_ctx* c, const rfe_local_ba_params& p, const void* kf_pose, const void* kf_cam, const void* kf_nlevels, const void* kf_sigma2,
              const void* kf_feat_off, const void* kpts, const void* xw, const void* ep, const void* ek, const void* ef, int P, int F, int L, int E,
              int Nf, const void* pose, const void* point, const void* erase, const void* stats) {
    if (P < 0 || P > RFE_LBA_MAX_FREE) return fail(c, RFE_ERR_INVALID, "local_ba: P outside 0..64");
    if (F < 0 || P + F < 1 || P + F > RFE_LBA_MAX_KF) return fail(c, RFE_ERR_INVALID, "local_ba: K = P + F outside 1..256");
    if (L < 0 || L > RFE_LBA_MAX_POINTS) return fail(c, RFE_ERR_INVALID, "local_ba: L outside 0..16384");
    if (E < 0 || E > RFE_LBA_MAX_EDGES) return fail(c, RFE_ERR_INVALID, "local_ba: E outside 0..131072");
    if (Nf < 0) return fail(c, RFE_ERR_INVALID, "local_ba: negative Nf");
    if (p.iterations < 0 || p.iterations > RFE_LBA_MAX_ITERATIONS) return fail(c, RFE_ERR_INVALID, "local_ba: iterations outside 0..64");
    if (p.max_trials < 0) return fail(c, RFE_ERR_INVALID, "local_ba: negative max_trials");
    if (!(isfinite(p.user_lambda_init) && isfinite(p.th2_mono) && isfinite(p.th2_stereo)))
        return fail(c, RFE_ERR_INVALID, "local_ba: non-finite th2 or user_lambda_init");
    if (!kf_pose || !kf_cam || !kf_nlevels || !kf_sigma2 || !kf_feat_off || !stats || (P > 0 && !pose) || (L > 0 && (!xw || !point)) ||
        (E > 0 && (!ep || !ek || !ef || !erase)) || (Nf > 0 && !kpts))
        return fail(c, RFE_ERR_INVALID, "local_ba: null pointer");
    return RFE_OK;
}

}  // namespace

extern "C" int rfe_local_ba_dev(rfe_ctx* c, rfe_local_ba_params prm, const float* kf_pose, const float* kf_cam, const int32_t* kf_nlevels,
                                const float* kf_sigma2, const int32_t* kf_feat_off, const float* kpts, const int32_t* octave, const float* uright,
                                const float* xw, const int32_t* edge_point, const int32_t* edge_kf, const int32_t* edge_feat, int P, int F, int L,
                                int E, int Nf, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* erase, double* chi2,
                                double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = lba_check(c, prm, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, kpts, xw, edge_point, edge_kf, edge_feat, P, F, L, E, Nf, pose,
                       point, erase, stats);
    if (rc) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    LbaDev d;
    memset(&d, 0, sizeof d);
    d.kf_pose = kf_pose; d.kf_cam = kf_cam; d.kf_sigma2 = kf_sigma2; d.kpts = kpts; d.uright = uright; d.xw = xw; d.kf_nlevels = kf_nlevels;
    d.kf_feat_off = kf_feat_off; d.octave = octave; d.edge_point = edge_point; d.edge_kf = edge_kf; d.edge_feat = edge_feat;
    d.P = P; d.K = P + F; d.L = L; d.E = E; d.Nf = Nf; d.NB = P * (P + 1) / 2;
    // `const float thHuberMono = sqrt(5.991)`; RobustKernelHuber keeps delta as a double and dsqr in a float member, as 6i
    d.delta_mono = (double)(float)sqrt(prm.th2_mono); d.dsqr_mono = (double)(float)(d.delta_mono * d.delta_mono);
    d.delta_stereo = (double)(float)sqrt(prm.th2_stereo); d.dsqr_stereo = (double)(float)(d.delta_stereo * d.delta_stereo);
    d.th2_mono = prm.th2_mono; d.th2_stereo = prm.th2_stereo;
    if ((rc = ws_carve(c, &c->ws_lba, &c->ws_lba_bytes, [&](Bump& a) { lba_layout(a, d); }))) return rc;
    if (!c->h_lba) {
        const hipError_t e = hipHostMalloc(&c->h_lba, sizeof(LbaPin), hipHostMallocDefault);
        if (e != hipSuccess) { c->h_lba = nullptr; return fail(c, RFE_ERR_OOM, std::string("local_ba: hipHostMalloc: ") + hipGetErrorString(e)); }
    }
    LbaPin* pin = (LbaPin*)c->h_lba;
    auto read_ctl = [&]() -> int {
        RFE_HIP(c, hipMemcpyAsync(&pin->ctl, d.ctl_d, sizeof(LbaCtl), hipMemcpyDeviceToHost, s));
        RFE_HIP(c, hipStreamSynchronize(s));
        return RFE_OK;
    };
    auto stopped = [&]() { return prm.stop && *prm.stop; };

    // the first kernel: validation; its verdict is read before anything else is launched
    RFE_HIP(c, hipMemsetAsync(d.ctl_d, 0, sizeof(LbaCtl), s));
    RFE_HIP(c, hipMemsetAsync(d.xp, 0, (size_t)std::max(6 * P, 1) * sizeof(double), s));      // g2o's x starts at zero: a failed first solve updates by it
    RFE_HIP(c, hipMemsetAsync(d.xl, 0, (size_t)std::max(3 * L, 1) * sizeof(double), s));
    { ProfScope ps(c, "lba_validate"); lba_launch_validate(s, d); }
    if ((rc = read_ctl())) return rc;
    if (pin->ctl.i[LBA_I_STATUS]) {
        const int st = pin->ctl.i[LBA_I_STATUS];
        return fail(c, RFE_ERR_INVALID, st & LBA_BAD_KF      ? "local_ba: nlevels outside 1..16 or kf_feat_off not ascending inside 0..Nf"
                                        : st & LBA_BAD_RANGE ? "local_ba: edge index out of range"
                                                             : "local_ba: edges not strictly ascending in (point, keyframe)");
    }
    // structure, once per call
    { ProfScope ps(c, "lba_structure"); lba_launch_structure(s, d); }
    if ((rc = read_ctl())) return rc;
    const int n_free = pin->ctl.i[LBA_I_NFREE], n_pairs = pin->ctl.i[LBA_I_NPAIRS];
    if ((rc = ensure_ws(c, &c->ws_lba_pairs, &c->ws_lba_pairs_bytes, al((size_t)std::max(n_pairs, 1) * 2 * sizeof(int32_t))))) return rc;
    d.pairs = (int32_t*)c->ws_lba_pairs;
    { ProfScope ps(c, "lba_structure"); lba_launch_pairs(s, d); }

    const int max_trials = prm.max_trials > 0 ? prm.max_trials : 10;
    int cur = 0, iters = 0, trials = 0, rejected = 0, failed = 0, flags = 0;
    bool ended_rejected = false;
    double lambda = 0.0, ni = 2.0;
    int nbad = 0;
    memset(pin->trace, 0, sizeof pin->trace);
    for (int it = 0; it < prm.iterations; ++it) {
        if (stopped()) { flags |= RFE_LBA_FLAG_STOPPED; break; }
        ++iters;
        const bool want_max = it == 0 && !(prm.user_lambda_init > 0);
        { ProfScope ps(c, "lba_linearise"); lba_launch_errors(s, d, cur, true, want_max); }
        if ((rc = read_ctl())) return rc;
        double current = pin->ctl.d[LBA_D_CHI];
        const double ini = current;
        if (it == 0) { lambda = prm.user_lambda_init > 0 ? prm.user_lambda_init : 1e-5 * pin->ctl.d[LBA_D_MAXDIAG]; ni = 2.0; nbad = 0; }
        double rho = 0.0;
        int qmax = 0;
        bool stop_seen = false;
        do {
            ++trials;
            { ProfScope ps(c, "lba_trial"); lba_launch_trial(s, d, cur, lambda); }
            { ProfScope ps(c, "lba_errors"); lba_launch_errors(s, d, cur ^ 1, false, false); }
            if ((rc = read_ctl())) return rc;
            double temp = pin->ctl.d[LBA_D_CHI];
            if (!pin->ctl.i[LBA_I_SOLVED]) { temp = DBL_MAX; ++failed; flags |= RFE_LBA_FLAG_SOLVE_FAILED; }
            const double scale = pin->ctl.d[LBA_D_SCALE] + 1e-3;
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
            stop_seen = stopped();
        } while (rho < 0 && qmax < max_trials && !stop_seen);
        if (stop_seen) flags |= RFE_LBA_FLAG_STOPPED;
        double* tr = pin->trace + 4 * it;
        tr[0] = (double)qmax; tr[1] = lambda; tr[2] = current; tr[3] = 0.0;
        if (qmax == max_trials || rho == 0) break;
        if ((ini - current) * 1e3 < ini) ++nbad; else nbad = 0;
        if (nbad >= 3) break;
    }
    if (iters == 0) {
        flags |= RFE_LBA_FLAG_NO_ITERATION;
        ProfScope ps(c, "lba_errors");
        lba_launch_errors(s, d, cur, false, false);
    }
    if (ended_rejected) flags |= RFE_LBA_FLAG_ENDED_REJECTED;
    { ProfScope ps(c, "lba_finish"); lba_launch_finish(s, d, cur, pose, pose_f32, point, point_f32, erase, chi2); }
    if ((rc = read_ctl())) return rc;
    flags |= pin->ctl.i[LBA_I_FLAGS];
    const int erased = pin->ctl.i[LBA_I_ERASED];
    const int32_t st[8] = {iters, trials, rejected, failed, erased, flags, n_free, n_pairs};
    memcpy(pin->stats, st, sizeof st);
    RFE_HIP(c, hipMemcpyAsync(stats, pin->stats, sizeof st, hipMemcpyHostToDevice, s));
    if (trace && prm.iterations > 0)
        RFE_HIP(c, hipMemcpyAsync(trace, pin->trace, (size_t)prm.iterations * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    RFE_HIP(c, hipStreamSynchronize(s));
    RFE_HIP(c, hipGetLastError());
    return erased;
}

extern "C" int rfe_local_ba(rfe_ctx* c, rfe_local_ba_params prm, const float* kf_pose, const float* kf_cam, const int32_t* kf_nlevels,
                            const float* kf_sigma2, const int32_t* kf_feat_off, const float* kpts, const int32_t* octave, const float* uright,
                            const float* xw, const int32_t* edge_point, const int32_t* edge_kf, const int32_t* edge_feat, int P, int F, int L, int E,
                            int Nf, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* erase, double* chi2, double* trace,
                            int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = lba_check(c, prm, kf_pose, kf_cam, kf_nlevels, kf_sigma2, kf_feat_off, kpts, xw, edge_point, edge_kf, edge_feat, P, F, L, E, Nf, pose,
                       point, erase, stats);
    if (rc) return rc;
    const int K = P + F;
    for (int k = 0; k < K; ++k)
        if (kf_nlevels[k] < 1 || kf_nlevels[k] > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, "local_ba: nlevels outside 1..16");
    for (int k = 0; k <= K; ++k)
        if (kf_feat_off[k] < 0 || kf_feat_off[k] > Nf || (k < K && kf_feat_off[k + 1] < kf_feat_off[k]))
            return fail(c, RFE_ERR_INVALID, "local_ba: kf_feat_off not ascending inside 0..Nf");
    for (int e = 0; e < E; ++e) {
        const int p = edge_point[e], k = edge_kf[e], f = edge_feat[e];
        if (p < 0 || p >= L || k < 0 || k >= K || f < 0 || f >= kf_feat_off[k + 1] - kf_feat_off[k])
            return fail(c, RFE_ERR_INVALID, "local_ba: edge index out of range");
        if (e > 0 && !(edge_point[e - 1] < p || (edge_point[e - 1] == p && edge_kf[e - 1] < k)))
            return fail(c, RFE_ERR_INVALID, "local_ba: edges not strictly ascending in (point, keyframe)");
    }
    RFE_HIP(c, hipSetDevice(c->device));
    float *dkp, *dkc, *dks, *dk, *du, *dx, *dpf, *dqf; int32_t *dnl, *dfo, *doc, *dep, *dek, *def, *dst; double *dpo, *dpt, *dc, *dtr; uint8_t* der;
    HostIo io(c, HostIo::DIRECT);
    io.in(dkp, kf_pose, (size_t)K * 7); io.in(dkc, kf_cam, (size_t)K * 5); io.in(dnl, kf_nlevels, (size_t)K);
    io.in(dks, kf_sigma2, (size_t)K * RFE_MAX_LEVELS); io.in(dfo, kf_feat_off, (size_t)K + 1);
    io.in(dk, kpts, (size_t)Nf * 2); io.in_opt(doc, octave, (size_t)Nf); io.in_opt(du, uright, (size_t)Nf); io.in(dx, xw, (size_t)L * 3);
    io.in(dep, edge_point, (size_t)E); io.in(dek, edge_kf, (size_t)E); io.in(def, edge_feat, (size_t)E);
    io.out(dpo, pose, (size_t)P * 7); io.out_opt(dpf, pose_f32, (size_t)P * 7); io.out(dpt, point, (size_t)L * 3); io.out_opt(dqf, point_f32, (size_t)L * 3);
    io.out(der, erase, (size_t)E); io.out_opt(dc, chi2, (size_t)E); io.out_opt(dtr, trace, (size_t)prm.iterations * 4); io.out(dst, stats, 8);
    if ((rc = io.upload())) return rc;
    const int erased = rfe_local_ba_dev(c, prm, dkp, dkc, dnl, dks, dfo, dk, doc, du, dx, dep, dek, def, P, F, L, E, Nf, dpo, dpf, dpt, dqf, der, dc,
                                        dtr, dst);
    if (erased < 0) return erased;
    if ((rc = io.download())) return rc;
    return erased;
}
