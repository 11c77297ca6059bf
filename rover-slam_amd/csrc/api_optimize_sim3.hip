// api_optimize_sim3.hip -- C ABI of librover_fe.so: Optimizer::OptimizeSim3, B problems per call (optimize_sim3.hip).
#include <string.h>
#include "api_internal.h"

using namespace rfe;

static int osim3_check(rfe_ctx* c, const rfe_optimize_sim3_params* P, const void* s12_0, const void* xw1, const void* xw2, const void* valid,
                       const void* kpts1, const void* idx2, const void* kpts2, int B, int N, int N2, const void* s12, const void* keep,
                       const void* stats) {
    if (!P || !s12_0 || !s12 || !keep || !stats) return fail(c, RFE_ERR_INVALID, "optimize_sim3: null pointer");
    if (B < 0 || B > 64) return fail(c, RFE_ERR_INVALID, "optimize_sim3: B outside 0..64");
    if (N < 0 || N > 4096) return fail(c, RFE_ERR_INVALID, "optimize_sim3: N outside 0..4096");
    if (N2 < 0 || N2 > 4096) return fail(c, RFE_ERR_INVALID, "optimize_sim3: N2 outside 0..4096");
    for (int b = 0; b < B; ++b) {
        if (P[b].nlevels1 < 1 || P[b].nlevels1 > RFE_MAX_LEVELS || P[b].nlevels2 < 1 || P[b].nlevels2 > RFE_MAX_LEVELS)
            return fail(c, RFE_ERR_INVALID, "optimize_sim3: nlevels outside 1..16");
        for (int k = 0; k < 3; ++k)
            if (P[b].iterations[k] < 0) return fail(c, RFE_ERR_INVALID, "optimize_sim3: negative iterations");
        if (P[b].max_trials < 0) return fail(c, RFE_ERR_INVALID, "optimize_sim3: negative max_trials");
    }
    if (B > 0 && N > 0 && (!xw1 || !xw2 || !valid || !kpts1 || !idx2)) return fail(c, RFE_ERR_INVALID, "optimize_sim3: null pointer");
    if (B > 0 && N2 > 0 && !kpts2) return fail(c, RFE_ERR_INVALID, "optimize_sim3: null pointer");
    return RFE_OK;
}

extern "C" int rfe_optimize_sim3_dev(rfe_ctx* c, const rfe_optimize_sim3_params* P, const double* s12_0, const float* xw1, const float* xw2,
                                     const uint8_t* valid, const float* kpts1, const int32_t* octave1, const int32_t* idx2,
                                     const float* kpts2, const int32_t* octave2, int B, int N, int N2, double* s12, float* s12_f32,
                                     uint8_t* keep, double* chi2, double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    const int rc = osim3_check(c, P, s12_0, xw1, xw2, valid, kpts1, idx2, kpts2, B, N, N2, s12, keep, stats);
    if (rc) return rc;
    if (B == 0) return RFE_OK;
    RFE_HIP(c, hipSetDevice(c->device));
    { ProfScope ps(c, "optimize_sim3");
      launch_optimize_sim3(c->stream, P, s12_0, xw1, xw2, valid, kpts1, octave1, idx2, kpts2, octave2, B, N, N2, s12, s12_f32, keep, chi2, trace,
                           stats); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_optimize_sim3(rfe_ctx* c, const rfe_optimize_sim3_params* P, const double* s12_0, const float* xw1, const float* xw2,
                                 const uint8_t* valid, const float* kpts1, const int32_t* octave1, const int32_t* idx2, const float* kpts2,
                                 const int32_t* octave2, int B, int N, int N2, double* s12, float* s12_f32, uint8_t* keep, double* chi2,
                                 double* trace, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = osim3_check(c, P, s12_0, xw1, xw2, valid, kpts1, idx2, kpts2, B, N, N2, s12, keep, stats);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        const rfe_optimize_sim3_params& p = P[b];
        if (!(finite({p.fx1, p.fy1, p.cx1, p.cy1, p.fx2, p.fy2, p.cx2, p.cy2, p.th2}) && finite(p.rcw1, 9) && finite(p.rcw2, 9) &&
              finite(p.tcw1, 3) && finite(p.tcw2, 3) && finite(p.inv_level_sigma2_1, p.nlevels1) && finite(p.inv_level_sigma2_2, p.nlevels2)))
            return fail(c, RFE_ERR_INVALID, "optimize_sim3: non-finite argument");
    }
    if (B == 0) return 0;
    RFE_HIP(c, hipSetDevice(c->device));
    const size_t f = (size_t)B * N, g = (size_t)B * N2;
    double *ds0, *ds, *dc, *dc_in, *dtr; float *dx1, *dx2, *dk1, *dk2, *dsf; uint8_t *dv, *dkeep, *dkeep_in; int32_t *do1, *di2, *do2, *dst;
    HostIo io(c, HostIo::DIRECT);
    io.in(ds0, s12_0, (size_t)B * 8); io.in(dx1, xw1, f * 3); io.in(dx2, xw2, f * 3); io.in(dv, valid, f); io.in(dk1, kpts1, f * 2);
    io.in_opt(do1, octave1, f); io.in(di2, idx2, f); io.in_opt(dk2, kpts2, g * 2); io.in_opt(do2, octave2, g);
    io.in(dkeep_in, (const uint8_t*)keep, f); io.in_opt(dc_in, (const double*)chi2, f * 2);   // cleared / written per row: what else they hold goes in
    io.out(ds, s12, (size_t)B * 8); io.out_opt(dsf, s12_f32, (size_t)B * 8); io.out(dkeep, keep, f); io.out_opt(dc, chi2, f * 2);
    io.out_opt(dtr, trace, (size_t)B * 16); io.out(dst, stats, (size_t)B * 8);
    if ((rc = io.upload())) return rc;
    if (f > 0) {
        RFE_HIP(c, hipMemcpyAsync(dkeep, dkeep_in, f, hipMemcpyDeviceToDevice, c->stream));
        if (chi2) RFE_HIP(c, hipMemcpyAsync(dc, dc_in, f * 2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = rfe_optimize_sim3_dev(c, P, ds0, dx1, dx2, dv, dk1, do1, di2, dk2, do2, B, N, N2, ds, dsf, dkeep, dc, dtr, dst))) return rc;
    if ((rc = io.download())) return rc;                                // waits for the stream
    return stats[0];
}
