// api_pose_inertial.hip -- C ABI of librover_fe.so: Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame, B problems per call
// (pose_inertial.hip).
#include <string.h>
#include "api_internal.h"

using namespace rfe;

static int pio_check(rfe_ctx* c, const rfe_pose_inertial_params* P, const void* mode, const void* cam, const void* state, const void* prev_state,
                     const void* preint, const void* cov_rw, const void* kpts, const void* xw, const void* has_mp, const void* track_depth, int B,
                     int N, const void* state_out, const void* outlier, const void* stats) {
    if (!P || !mode || !cam || !state || !prev_state || !preint || !cov_rw || !state_out || !outlier || !stats)
        return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: null pointer");
    if (B < 0 || B > 64) return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: B outside 0..64");
    if (N < 0 || N > 4096) return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: N outside 0..4096");
    if (P->nlevels < 1 || P->nlevels > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: nlevels outside 1..16");
    if (B > 0 && N > 0 && (!kpts || !xw || !has_mp || !track_depth)) return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: null pointer");
    return RFE_OK;
}

extern "C" int rfe_pose_inertial_optimization_dev(rfe_ctx* c, const rfe_pose_inertial_params* P, const int32_t* mode, const int32_t* rec_init,
                                                  const float* cam, const float* state, const float* prev_state, const float* preint,
                                                  const float* cov_rw, const double* prior_in, const float* kpts, const int32_t* octave,
                                                  const float* uright, const float* xw, const uint8_t* has_mp, const float* track_depth,
                                                  const int32_t* n, int B, int N, double* state_out, float* state_f32, uint8_t* outlier,
                                                  float* chi2, double* prior_out, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    const int rc = pio_check(c, P, mode, cam, state, prev_state, preint, cov_rw, kpts, xw, has_mp, track_depth, B, N, state_out, outlier, stats);
    if (rc) return rc;
    if (B == 0) return RFE_OK;
    RFE_HIP(c, hipSetDevice(c->device));
    PioArgs a;
    a.mode = mode; a.rec_init = rec_init; a.octave = octave; a.n = n; a.cam = cam; a.state = state; a.prev_state = prev_state; a.preint = preint;
    a.cov_rw = cov_rw; a.kpts = kpts; a.uright = uright; a.xw = xw; a.track_depth = track_depth; a.prior_in = prior_in; a.has_mp = has_mp;
    a.state_out = state_out; a.prior_out = prior_out; a.trace = trace; a.state_f32 = state_f32; a.chi2 = chi2; a.outlier = outlier; a.stats = stats;
    a.N = N;
    { ProfScope ps(c, "pose_inertial");
      launch_pose_inertial(c->stream, *P, a, B); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_pose_inertial_optimization(rfe_ctx* c, const rfe_pose_inertial_params* P, const int32_t* mode, const int32_t* rec_init,
                                              const float* cam, const float* state, const float* prev_state, const float* preint,
                                              const float* cov_rw, const double* prior_in, const float* kpts, const int32_t* octave,
                                              const float* uright, const float* xw, const uint8_t* has_mp, const float* track_depth,
                                              const int32_t* n, int B, int N, double* state_out, float* state_f32, uint8_t* outlier, float* chi2,
                                              double* prior_out, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = pio_check(c, P, mode, cam, state, prev_state, preint, cov_rw, kpts, xw, has_mp, track_depth, B, N, state_out, outlier, stats);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (mode[b] != RFE_PIO_LAST_KEYFRAME && mode[b] != RFE_PIO_LAST_FRAME)
            return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: mode is neither RFE_PIO_LAST_KEYFRAME nor RFE_PIO_LAST_FRAME");
        if (mode[b] == RFE_PIO_LAST_FRAME && !prior_in) return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: LastFrame mode without prior_in");
        if (!(preint[(size_t)b * RFE_PIO_PREINT_FLOATS] > 0.f)) return fail(c, RFE_ERR_INVALID, "pose_inertial_optimization: dT is not positive");
    }
    if (B == 0) return 0;
    RFE_HIP(c, hipSetDevice(c->device));
    const size_t f = (size_t)B * N;
    float *dcam, *dst, *dpst, *dpre, *dcov, *dk, *du, *dx, *dtd, *dsf, *dc, *dc_in; int32_t *dmode, *drec, *doct, *dn, *dstats;
    uint8_t *dm, *dout, *dout_in; double *dpin, *dso, *dpo, *dtr;
    HostIo io(c, HostIo::DIRECT);
    io.in(dmode, mode, (size_t)B); io.in_opt(drec, rec_init, (size_t)B); io.in(dcam, cam, (size_t)B * RFE_PIO_CAM_FLOATS);
    io.in(dst, state, (size_t)B * RFE_PIO_STATE_FLOATS); io.in(dpst, prev_state, (size_t)B * RFE_PIO_STATE_FLOATS);
    io.in(dpre, preint, (size_t)B * RFE_PIO_PREINT_FLOATS); io.in(dcov, cov_rw, (size_t)B * RFE_PIO_COV_RW_FLOATS);
    io.in_opt(dpin, prior_in, (size_t)B * RFE_PIO_PRIOR_DOUBLES);
    io.in(dk, kpts, f * 2); io.in_opt(doct, octave, f); io.in_opt(du, uright, f); io.in(dx, xw, f * 3); io.in(dm, has_mp, f);
    io.in(dtd, track_depth, f); io.in_opt(dn, n, (size_t)B);
    io.in(dout_in, (const uint8_t*)outlier, f); io.in_opt(dc_in, (const float*)chi2, f);   // written where has_mp is set only: what else they hold goes in
    io.out(dso, state_out, (size_t)B * RFE_PIO_STATE_FLOATS); io.out_opt(dsf, state_f32, (size_t)B * RFE_PIO_STATE_FLOATS); io.out(dout, outlier, f);
    io.out_opt(dc, chi2, f); io.out_opt(dpo, prior_out, (size_t)B * RFE_PIO_PRIOR_DOUBLES); io.out_opt(dtr, trace, (size_t)B * 32);
    io.out(dstats, stats, (size_t)B * 16);
    if ((rc = io.upload())) return rc;
    if (f > 0) {
        RFE_HIP(c, hipMemcpyAsync(dout, dout_in, f, hipMemcpyDeviceToDevice, c->stream));
        if (chi2) RFE_HIP(c, hipMemcpyAsync(dc, dc_in, f * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = rfe_pose_inertial_optimization_dev(c, P, dmode, drec, dcam, dst, dpst, dpre, dcov, dpin, dk, doct, du, dx, dm, dtd, dn, B, N, dso, dsf,
                                                 dout, dc, dpo, dtr, dstats)))
        return rc;
    if ((rc = io.download())) return rc;                                // waits for the stream
    return stats[0];
}
