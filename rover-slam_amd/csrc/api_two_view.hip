// api_two_view.hip -- C ABI of librover_fe.so: TwoViewReconstruction, the H and F RANSAC of B frame pairs per call (two_view.hip).
#include <string.h>
#include "api_internal.h"

using namespace rfe;

// ws_tv
static void tv_layout(Bump& a, int B, int Kmax, int H, bool own_scores, TvBuffers& b) {
    const size_t Ks = tv_soa_stride(Kmax), slots = std::max<size_t>((size_t)B * 8 * Kmax, 1);
    b.prob = a.take<TvProb>(TV_MAX_B); b.sel = a.take<TvSel>(TV_MAX_B);
    b.soa = a.take<float>(std::max<size_t>((size_t)B * 4 * Ks, 1));
    b.sets = a.take<int32_t>((size_t)B * H * 8);
    b.hmodels = a.take<float>((size_t)B * H * 18);
    b.scores = own_scores ? a.take<float>((size_t)B * H * 2) : nullptr;
    b.winl = a.take<uint8_t>(std::max<size_t>((size_t)B * 2 * Kmax, 1));
    b.rcode = a.take<uint8_t>(slots); b.rcos = a.take<float>(slots); b.rp = a.take<float>(slots * 3);
}

static int tv_check_args(rfe_ctx* c, const rfe_two_view_params* P, const void* k1, const void* k2, const void* S, const void* pairs, const void* draws,
                         int B, int N1max, int N2max, int Kmax, int H, const void* R21, const void* t21, const void* stats) {
    if (!P || !draws || !S || !R21 || !t21 || !stats) return fail(c, RFE_ERR_INVALID, "two_view: null pointer");
    if (B < 0 || B > TV_MAX_B) return fail(c, RFE_ERR_INVALID, "two_view: B outside 0..16");
    if (N1max < 0 || N1max > 4096 || N2max < 0 || N2max > 4096 || Kmax < 0 || Kmax > 4096)
        return fail(c, RFE_ERR_INVALID, "two_view: N1max, N2max or Kmax outside 0..4096");
    if (H < 1 || H > 1024) return fail(c, RFE_ERR_INVALID, "two_view: H outside 1..1024");
    if (B > 0 && ((N1max > 0 && !k1) || (N2max > 0 && !k2) || (Kmax > 0 && !pairs))) return fail(c, RFE_ERR_INVALID, "two_view: null pointer");
    for (int b = 0; b < B; ++b) {
        const int its = P[b].its == 0 ? 200 : P[b].its;
        if (P[b].its < 0 || its > H) return fail(c, RFE_ERR_INVALID, "two_view: its outside 0..H");
        if (P[b].n1 < 0 || P[b].n1 > N1max || P[b].n2 < 0 || P[b].n2 > N2max) return fail(c, RFE_ERR_INVALID, "two_view: n1 or n2 outside its capacity");
        if (P[b].min_triangulated < 0) return fail(c, RFE_ERR_INVALID, "two_view: negative min_triangulated");
    }
    return RFE_OK;
}

extern "C" int rfe_two_view_dev(rfe_ctx* c, const rfe_two_view_params* P, const float* kpts1, const float* kpts2, const int32_t* S,
                                const int32_t* pairs, const int32_t* draws, int B, int N1max, int N2max, int Kmax, int H, float* R21, float* t21,
                                float* p3d, uint8_t* triangulated, uint8_t* inliers_h, uint8_t* inliers_f, float* scores, float* models,
                                float* cand, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = tv_check_args(c, P, kpts1, kpts2, S, pairs, draws, B, N1max, N2max, Kmax, H, R21, t21, stats);
    if (rc) return rc;
    if (B == 0) return RFE_OK;
    RFE_HIP(c, hipSetDevice(c->device));
    TvBuffers w;
    rc = ws_carve(c, &c->ws_tv, &c->ws_tv_bytes, [&](Bump& a) { tv_layout(a, B, Kmax, H, !scores, w); });
    if (rc) return rc;
    {
        ProfScope ps(c, "two_view");
        launch_two_view(c->stream, P, kpts1, kpts2, S, pairs, draws, B, N1max, N2max, Kmax, H, w, R21, t21, p3d, triangulated, inliers_h, inliers_f,
                        scores ? scores : w.scores, models, cand, stats);
    }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_two_view(rfe_ctx* c, const rfe_two_view_params* P, const float* kpts1, const float* kpts2, const int32_t* S, const int32_t* pairs,
                            const int32_t* draws, int B, int N1max, int N2max, int Kmax, int H, float* R21, float* t21, float* p3d,
                            uint8_t* triangulated, uint8_t* inliers_h, uint8_t* inliers_f, float* scores, float* models, float* cand,
                            int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = tv_check_args(c, P, kpts1, kpts2, S, pairs, draws, B, N1max, N2max, Kmax, H, R21, t21, stats);
    if (rc) return rc;
    for (int b = 0; b < B; ++b)
        if (!finite({P[b].fx, P[b].fy, P[b].cx, P[b].cy, P[b].sigma})) return fail(c, RFE_ERR_INVALID, "two_view: non-finite intrinsic or sigma");
    if (B == 0) return 0;
    RFE_HIP(c, hipSetDevice(c->device));
    const size_t f1 = (size_t)B * N1max, f2 = (size_t)B * N2max, fk = (size_t)B * Kmax, g = (size_t)B * H;
    float *dk1, *dk2, *dR, *dt, *dp, *dsc, *dmo, *dca, *dp_in, *dsc_in, *dca_in; int32_t *dS, *dpr, *ddr, *dst;
    uint8_t *dtr, *dih, *dif, *dtr_in, *dih_in, *dif_in;
    HostIo io(c, HostIo::DIRECT);
    io.in(dk1, kpts1, f1 * 2); io.in(dk2, kpts2, f2 * 2); io.in(dS, S, (size_t)B); io.in(dpr, pairs, fk * 2); io.in(ddr, draws, g * 8);
    // written in front of the counts only: what else they hold goes in
    io.in_opt(dp_in, (const float*)p3d, f1 * 3); io.in_opt(dtr_in, (const uint8_t*)triangulated, f1);
    io.in_opt(dih_in, (const uint8_t*)inliers_h, fk); io.in_opt(dif_in, (const uint8_t*)inliers_f, fk);
    io.in_opt(dsc_in, (const float*)scores, g * 2); io.in_opt(dca_in, (const float*)cand, (size_t)B * 128);
    io.out(dR, R21, (size_t)B * 9); io.out(dt, t21, (size_t)B * 3); io.out_opt(dp, p3d, f1 * 3); io.out_opt(dtr, triangulated, f1);
    io.out_opt(dih, inliers_h, fk); io.out_opt(dif, inliers_f, fk); io.out_opt(dsc, scores, g * 2); io.out_opt(dmo, models, (size_t)B * 18);
    io.out_opt(dca, cand, (size_t)B * 128); io.out(dst, stats, (size_t)B * 16);
    if ((rc = io.upload())) return rc;
    const struct { void* dst; const void* src; size_t bytes; } keep[] = {{dp, dp_in, f1 * 12}, {dtr, dtr_in, f1}, {dih, dih_in, fk}, {dif, dif_in, fk},
                                                                         {dsc, dsc_in, g * 8}, {dca, dca_in, (size_t)B * 512}};
    for (const auto& k : keep)
        if (k.dst && k.bytes) RFE_HIP(c, hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = rfe_two_view_dev(c, P, dk1, dk2, dS, dpr, ddr, B, N1max, N2max, Kmax, H, dR, dt, dp, dtr, dih, dif, dsc, dmo, dca, dst))) return rc;
    if ((rc = io.download())) return rc;                                // waits for the stream
    return stats[0];
}
