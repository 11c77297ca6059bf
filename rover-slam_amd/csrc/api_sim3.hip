// api_sim3.hip -- C ABI of librover_fe.so: Sim3Solver's RANSAC, every hypothesis of B problems per call (sim3_solver.hip).
#include <limits.h>
#include <math.h>
#include <string.h>
#include "api_internal.h"

using namespace rfe;

// ws_s3: the per-problem records, the front's rows, and counts / hyps when the caller keeps neither
struct Sim3Buffers { Sim3Prob* prob; float *front, *hyps; int32_t* counts; };
static void sim3_layout(Bump& a, int B, int N, int H, bool own_counts, bool own_hyps, Sim3Buffers& b) {
    b.prob = a.take<Sim3Prob>(64);
    b.front = a.take<float>(std::max<size_t>((size_t)B * 12 * N, 1));
    b.counts = own_counts ? a.take<int32_t>((size_t)B * H) : nullptr;
    b.hyps = own_hyps ? a.take<float>((size_t)B * H * 32) : nullptr;
}

static int sim3_check(rfe_ctx* c, const rfe_sim3_solver_params* P, const void* xw1, const void* xw2, const void* s1, const void* s2,
                      const void* draws, int B, int N, int H, const void* T12, const void* stats) {
    if (!P || !draws || !T12 || !stats) return fail(c, RFE_ERR_INVALID, "sim3_ransac: null pointer");
    if (B < 0 || B > 64) return fail(c, RFE_ERR_INVALID, "sim3_ransac: B outside 0..64");
    if (N < 0 || N > 4096) return fail(c, RFE_ERR_INVALID, "sim3_ransac: N outside 0..4096");
    if (H < 1 || H > 1024) return fail(c, RFE_ERR_INVALID, "sim3_ransac: H outside 1..1024");
    if (B > 0 && N > 0 && (!xw1 || !xw2 || !s1 || !s2)) return fail(c, RFE_ERR_INVALID, "sim3_ransac: null pointer");
    for (int b = 0; b < B; ++b) {
        if (P[b].its < 1 || P[b].its > H) return fail(c, RFE_ERR_INVALID, "sim3_ransac: its outside 1..H");
        if (P[b].min_inliers < 0) return fail(c, RFE_ERR_INVALID, "sim3_ransac: negative min_inliers");
    }
    return RFE_OK;
}

extern "C" int rfe_sim3_ransac_dev(rfe_ctx* c, const rfe_sim3_solver_params* P, const float* xw1, const float* xw2, const float* s1,
                                   const float* s2, const int32_t* draws, int B, int N, int H, float* T12, float* R, float* t, float* s,
                                   uint8_t* inliers, uint8_t* best_inliers, int32_t* counts, float* hyps, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = sim3_check(c, P, xw1, xw2, s1, s2, draws, B, N, H, T12, stats);
    if (rc) return rc;
    if (B == 0) return RFE_OK;
    RFE_HIP(c, hipSetDevice(c->device));
    Sim3Buffers w;
    rc = ws_carve(c, &c->ws_s3, &c->ws_s3_bytes, [&](Bump& a) { sim3_layout(a, B, N, H, !counts, !hyps, w); });
    if (rc) return rc;
    int32_t* cn = counts ? counts : w.counts;
    float* hy = hyps ? hyps : w.hyps;
    { ProfScope ps(c, "sim3_front"); launch_sim3_front(c->stream, P, xw1, xw2, s1, s2, B, N, w.prob, w.front); }
    { ProfScope ps(c, "sim3_hypotheses"); launch_sim3_hypotheses(c->stream, w.prob, w.front, draws, B, N, H, cn, hy); }
    { ProfScope ps(c, "sim3_select"); launch_sim3_select(c->stream, w.prob, w.front, cn, hy, B, N, H, T12, R, t, s, inliers, best_inliers, stats); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_sim3_ransac(rfe_ctx* c, const rfe_sim3_solver_params* P, const float* xw1, const float* xw2, const float* s1, const float* s2,
                               const int32_t* draws, int B, int N, int H, float* T12, float* R, float* t, float* s, uint8_t* inliers,
                               uint8_t* best_inliers, int32_t* counts, float* hyps, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = sim3_check(c, P, xw1, xw2, s1, s2, draws, B, N, H, T12, stats);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        const rfe_sim3_solver_params& p = P[b];
        if (!(finite({p.fx1, p.fy1, p.cx1, p.cy1, p.fx2, p.fy2, p.cx2, p.cy2}) && finite(p.rcw1) && finite(p.rcw2) && finite(p.tcw1) && finite(p.tcw2)))
            return fail(c, RFE_ERR_INVALID, "sim3_ransac: non-finite pose or intrinsic");
        const int n = p.n < 0 ? 0 : (p.n > N ? N : p.n);
        for (int i = 0; i < n; ++i) {
            const float a = s1[(size_t)b * N + i], d = s2[(size_t)b * N + i];
            if (!(finite(a) && finite(d) && a >= 0.f && d >= 0.f)) return fail(c, RFE_ERR_INVALID, "sim3_ransac: negative or non-finite sigma2");
        }
    }
    if (B == 0) return 0;
    RFE_HIP(c, hipSetDevice(c->device));
    const size_t f = (size_t)B * N, g = (size_t)B * H;
    float *dx1, *dx2, *ds1, *ds2, *dT, *dR, *dt, *dsc, *dhy, *dhy_in; int32_t *ddr, *dcn, *dcn_in, *dst; uint8_t *din, *dbe, *din_in, *dbe_in;
    HostIo io(c, HostIo::DIRECT);
    io.in(dx1, xw1, f * 3); io.in(dx2, xw2, f * 3); io.in(ds1, s1, f); io.in(ds2, s2, f); io.in(ddr, draws, g * 3);
    // written in front of n and its only: what else they hold goes in
    io.in_opt(din_in, (const uint8_t*)inliers, f); io.in_opt(dbe_in, (const uint8_t*)best_inliers, f);
    io.in_opt(dcn_in, (const int32_t*)counts, g); io.in_opt(dhy_in, (const float*)hyps, g * 32);
    io.out(dT, T12, (size_t)B * 16); io.out_opt(dR, R, (size_t)B * 9); io.out_opt(dt, t, (size_t)B * 3); io.out_opt(dsc, s, (size_t)B);
    io.out_opt(din, inliers, f); io.out_opt(dbe, best_inliers, f); io.out_opt(dcn, counts, g); io.out_opt(dhy, hyps, g * 32);
    io.out(dst, stats, (size_t)B * 8);
    if ((rc = io.upload())) return rc;
    if (inliers && f) RFE_HIP(c, hipMemcpyAsync(din, din_in, f, hipMemcpyDeviceToDevice, c->stream));
    if (best_inliers && f) RFE_HIP(c, hipMemcpyAsync(dbe, dbe_in, f, hipMemcpyDeviceToDevice, c->stream));
    if (counts) RFE_HIP(c, hipMemcpyAsync(dcn, dcn_in, g * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    if (hyps) RFE_HIP(c, hipMemcpyAsync(dhy, dhy_in, g * 32 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = rfe_sim3_ransac_dev(c, P, dx1, dx2, ds1, ds2, ddr, B, N, H, dT, dR, dt, dsc, din, dbe, dcn, dhy, dst))) return rc;
    if ((rc = io.download())) return rc;                                // waits for the stream
    return stats[0];
}

extern "C" int rfe_sim3_ransac_iterations(double probability, int min_inliers, int n, int max_its) {
    int it;
    if (min_inliers == n) {
        it = 1;
    } else {
        const float epsilon = (float)min_inliers / n;
        const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        it = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT_MIN;   // NaN and out of range: what cvttsd2si leaves
    }
    return std::max(1, std::min(it, max_its));
}
