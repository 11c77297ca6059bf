// api_pose.hip -- C ABI of librover_fe.so: Optimizer::PoseOptimization, B problems per call (pose_opt.hip).
#include <string.h>
#include "api_internal.h"

using namespace rfe;

static int pose_check(rfe_ctx* c, const rfe_pose_params* P, const void* pose0, const void* kpts, const void* xw, const void* has_mp, int B, int N,
                      const void* pose, const void* outlier, const void* stats) {
    if (!P || !pose0 || !pose || !outlier || !stats) return fail(c, RFE_ERR_INVALID, "pose_optimization: null pointer");
    if (B < 0 || B > 64) return fail(c, RFE_ERR_INVALID, "pose_optimization: B outside 0..64");
    if (N < 0 || N > 4096) return fail(c, RFE_ERR_INVALID, "pose_optimization: N outside 0..4096");
    if (P->nlevels < 1 || P->nlevels > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, "pose_optimization: nlevels outside 1..16");
    for (int k = 0; k < 4; ++k)
        if (P->iterations[k] < 0) return fail(c, RFE_ERR_INVALID, "pose_optimization: negative iterations");
    if (P->max_trials < 0) return fail(c, RFE_ERR_INVALID, "pose_optimization: negative max_trials");
    if (B > 0 && N > 0 && (!kpts || !xw || !has_mp)) return fail(c, RFE_ERR_INVALID, "pose_optimization: null pointer");
    return RFE_OK;
}

extern "C" int rfe_pose_optimization_dev(rfe_ctx* c, const rfe_pose_params* P, const float* pose0, const float* kpts, const int32_t* octave,
                                         const float* uright, const float* xw, const uint8_t* has_mp, const int32_t* n, int B, int N,
                                         double* pose, float* pose_f32, uint8_t* outlier, float* chi2, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    const int rc = pose_check(c, P, pose0, kpts, xw, has_mp, B, N, pose, outlier, stats);
    if (rc) return rc;
    if (B == 0) return RFE_OK;
    RFE_HIP(c, hipSetDevice(c->device));
    { ProfScope ps(c, "pose_opt");
      launch_pose_opt(c->stream, *P, pose0, kpts, octave, uright, xw, has_mp, n, B, N, pose, pose_f32, outlier, chi2, trace, stats); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_pose_optimization(rfe_ctx* c, const rfe_pose_params* P, const float* pose0, const float* kpts, const int32_t* octave,
                                     const float* uright, const float* xw, const uint8_t* has_mp, const int32_t* n, int B, int N, double* pose,
                                     float* pose_f32, uint8_t* outlier, float* chi2, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = pose_check(c, P, pose0, kpts, xw, has_mp, B, N, pose, outlier, stats);
    if (rc) return rc;
    if (!(finite({P->fx, P->fy, P->cx, P->cy, P->bf}) && finite(P->inv_level_sigma2, P->nlevels) && finite(pose0, (size_t)B * 7)))
        return fail(c, RFE_ERR_INVALID, "pose_optimization: non-finite argument");
    if (B == 0) return 0;
    RFE_HIP(c, hipSetDevice(c->device));
    const size_t f = (size_t)B * N;
    float *dp0, *dk, *du, *dx, *dpf, *dc, *dc_in; int32_t *doct, *dn, *dst; uint8_t *dm, *dout, *dout_in; double *dpose, *dtr;
    HostIo io(c, HostIo::DIRECT);
    io.in(dp0, pose0, (size_t)B * 7); io.in(dk, kpts, f * 2); io.in_opt(doct, octave, f); io.in_opt(du, uright, f); io.in(dx, xw, f * 3);
    io.in(dm, has_mp, f); io.in_opt(dn, n, B);
    io.in(dout_in, (const uint8_t*)outlier, f); io.in_opt(dc_in, (const float*)chi2, f);   // written where has_mp is set only: what else they hold goes in
    io.out(dpose, pose, (size_t)B * 7); io.out_opt(dpf, pose_f32, (size_t)B * 7); io.out(dout, outlier, f); io.out_opt(dc, chi2, f);
    io.out_opt(dtr, trace, (size_t)B * 32); io.out(dst, stats, (size_t)B * 8);
    if ((rc = io.upload())) return rc;
    if (f > 0) {
        RFE_HIP(c, hipMemcpyAsync(dout, dout_in, f, hipMemcpyDeviceToDevice, c->stream));
        if (chi2) RFE_HIP(c, hipMemcpyAsync(dc, dc_in, f * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = rfe_pose_optimization_dev(c, P, dp0, dk, doct, du, dx, dm, dn, B, N, dpose, dpf, dout, dc, dtr, dst))) return rc;
    if ((rc = io.download())) return rc;                                // waits for the stream
    return stats[0];
}
