// proj_frustum.hip -- steps 2 and 3 of Tracking::SearchLocalPoints up to the search (reference src/Tracking.cc:4124-4147): Frame::isInFrustum
// (src/Frame.cc:711-794, one camera) and the head of SPmatcher::SearchByProjection1 (src/Matchers/SPmatcher.cc:1184-1206) for all local map
// points of a frame at once:
//   * frustum_project_kernel: Pc = mRcw * P + mtcw, Pinhole::project, the depth, image, distance and viewing-angle gates in the reference's
//                             order, MapPoint::PredictScale (src/MapPoint.cc:716-732: the bare mfMaxDistance = scale_dist), the far-point gate
//                             and radius = (RadiusByViewingCos * th) * mvScaleFactors[L].  One thread per map point; fp32, one rounding per
//                             written operation (-ffp-contract=off, plain / and sqrtf).  proj / radius / level are what proj_count_kernel
//                             (proj_search.hip) reads; the rest is what isInFrustum leaves in the map point.
#include "rfe_internal.h"

namespace rfe {

// RadiusByViewingCos compares the float with the DOUBLE literal 0.998 (SPmatcher.cc:1359).  fl32(0.998) = 0x1.fef9dcp-1 = 0.99800002574...
// lies above that literal and its lower neighbour 0x1.fef9dap-1 = 0.99799996614... below it, so `(double)viewCos > 0.998` is
// `viewCos >= fl32(0.998)` for every float (and false for NaN in both forms).
constexpr float FR_VIEWCOS_NEAR = 0x1.fef9dcp-1f;
static_assert(FR_VIEWCOS_NEAR == 0.998f && (double)FR_VIEWCOS_NEAR > 0.998 && (double)0x1.fef9dap-1f < 0.998, "threshold of RadiusByViewingCos");

__global__ __launch_bounds__(256) void frustum_project_kernel(const rfe_frustum_params P, const float* __restrict__ pw,
                                                              const float* __restrict__ normal, const float* __restrict__ min_dist,
                                                              const float* __restrict__ max_dist, const float* __restrict__ scale_dist,
                                                              const uint8_t* __restrict__ valid, int Np, float* __restrict__ proj,
                                                              float* __restrict__ radius, int32_t* __restrict__ level,
                                                              float* __restrict__ proj_xr, float* __restrict__ depth,
                                                              float* __restrict__ view_cos, int32_t* __restrict__ reject,
                                                              int32_t* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int rej = 1, lv = -1;
    float u = 0.f, v = 0.f, r = 0.f, xr = 0.f, dep = 0.f, vc = 0.f;
    if (i < Np && (!valid || valid[i])) {
        const float px = pw[3 * i], py = pw[3 * i + 1], pz = pw[3 * i + 2];
        const float x = ((P.rcw[0] * px + P.rcw[1] * py) + P.rcw[2] * pz) + P.tcw[0];
        const float y = ((P.rcw[3] * px + P.rcw[4] * py) + P.rcw[5] * pz) + P.tcw[1];
        const float z = ((P.rcw[6] * px + P.rcw[7] * py) + P.rcw[8] * pz) + P.tcw[2];
        const float pc_dist = sqrtf((x * x + y * y) + z * z);             // Pc.norm()
        const float invz = 1.f / z;
        rej = 2; u = -1.f; v = -1.f;                                      // Frame.cc:712-713
        if (!(z < 0.f)) {                                                 // z == +-0 and NaN go on
            const float pu = (P.fx * x) / z + P.cx, pv = (P.fy * y) / z + P.cy;   // Pinhole::project
            rej = 3;
            if (!(pu < P.min_x || pu > P.max_x || pv < P.min_y || pv > P.max_y)) {   // closed, and NaN passes: every comparison is false
                u = pu; v = pv;                                           // :740-741
                const float ox = px - P.ow[0], oy = py - P.ow[1], oz = pz - P.ow[2];
                const float dist = sqrtf((ox * ox + oy * oy) + oz * oz);
                rej = 4;
                if (!(dist < min_dist[i] || dist > max_dist[i])) {
                    const float cosv = ((ox * normal[3 * i] + oy * normal[3 * i + 1]) + oz * normal[3 * i + 2]) / dist;
                    rej = 5;
                    if (!(cosv < P.view_cos_limit)) {
                        lv = predict_scale_level(scale_dist[i], dist, P.log_scale_factor, P.nlevels);
                        xr = u - P.mbf * invz; dep = pc_dist; vc = cosv;
                        rej = (P.far_points && pc_dist > P.th_far) ? 6 : 0;                       // SPmatcher.cc:1184
                        if (rej == 0) {
                            const int L = P.level_mode == RFE_LEVEL_PREDICTED ? lv : 0;           // :1193 as written: nPredictedLevel = 0
                            r = ((cosv >= FR_VIEWCOS_NEAR ? 2.5f : 4.0f) * P.th) * level_table(P.scale_factors, L);
                        }
                    }
                }
            }
        }
    }
    if (i < Np) {
        proj[2 * i] = u; proj[2 * i + 1] = v; radius[i] = r; level[i] = lv;
        if (proj_xr) proj_xr[i] = xr;
        if (depth) depth[i] = dep;
        if (view_cos) view_cos[i] = vc;
        if (reject) reject[i] = rej;
    }
    const unsigned long long seen = __ballot(i < Np && (rej == 0 || rej == 6));
    const unsigned long long searched = __ballot(i < Np && rej == 0);
    if ((threadIdx.x & 63) == 0) {
        if (seen) atomicAdd(&stats[4], (int)__popcll(seen));
        if (searched) atomicAdd(&stats[5], (int)__popcll(searched));
    }
}

void launch_frustum_project(hipStream_t s, const rfe_frustum_params& P, const float* pw, const float* normal, const float* min_dist,
                            const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np, float* proj, float* radius,
                            int32_t* level, float* proj_xr, float* depth, float* view_cos, int32_t* reject, int32_t* stats) {
    if (Np <= 0) return;
    hipLaunchKernelGGL(frustum_project_kernel, dim3((Np + 255) / 256), dim3(256), 0, s, P, pw, normal, min_dist, max_dist, scale_dist, valid, Np,
                       proj, radius, level, proj_xr, depth, view_cos, reject, stats);
}

}  // namespace rfe
