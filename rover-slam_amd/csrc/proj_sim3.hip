// proj_sim3.hip -- the front of the Sim3 SearchByProjection loops of loop closing (reference src/Matchers/SPmatcher.cc:1576-1625 and
// :2094-2139; the same lines open Fuse's Sim3 overload, :230-300) for all map points of a call at once:
//   * sim3_project_kernel: Tcw * p3Dw as Sophus writes it (Thirdparty/Sophus/sophus/so3.hpp:358-367 plus the translation), the projection
//                          in the form the overload uses, the gates in the reference's order, MapPoint::PredictScale (src/MapPoint.cc:689-707;
//                          it divides the bare mfMaxDistance = scale_dist, not the 1.2f * mfMaxDistance the distance gate compares with)
//                          and radius = th * mvScaleFactors[level].  One thread per map point; fp32, one rounding per written operation
//                          (-ffp-contract=off, plain / and sqrtf).  What it writes is what proj_count_kernel (proj_search.hip) reads.
#include "rfe_internal.h"

namespace rfe {

// Eigen's cross product component order (Eigen/src/Geometry/OrthoMethods.h)
#define S3_CROSS(ox, oy, oz, ax, ay, az, bx, by, bz) \
    const float ox = ay * bz - az * by, oy = az * bx - ax * bz, oz = ax * by - ay * bx

__global__ __launch_bounds__(256) void sim3_project_kernel(const rfe_sim3_params P, const float* __restrict__ pw,
                                                           const float* __restrict__ normal, const float* __restrict__ min_dist,
                                                           const float* __restrict__ max_dist, const float* __restrict__ scale_dist,
                                                           const uint8_t* __restrict__ valid, int Np,
                                                           float* __restrict__ proj, float* __restrict__ radius,
                                                           int32_t* __restrict__ level, int32_t* __restrict__ reject,
                                                           int32_t* __restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int rej = 1, lv = -1;
    float u = 0.f, v = 0.f, r = 0.f;
    if (i < Np && (!valid || valid[i])) {
        const float px = pw[3 * i], py = pw[3 * i + 1], pz = pw[3 * i + 2];
        const float qx = P.quat[0], qy = P.quat[1], qz = P.quat[2], qw = P.quat[3];
        S3_CROSS(ax, ay, az, qx, qy, qz, px, py, pz);                 // uv = q.vec().cross(p)
        const float ux = ax + ax, uy = ay + ay, uz = az + az;         // uv += uv
        S3_CROSS(wx, wy, wz, qx, qy, qz, ux, uy, uz);                 // q.vec().cross(uv)
        const float x = ((px + qw * ux) + wx) + P.t[0], y = ((py + qw * uy) + wy) + P.t[1], z = ((pz + qw * uz) + wz) + P.t[2];
        rej = 2;
        if (!(z < 0.f)) {                                             // z == 0 (and NaN) goes on and fails IsInImage through inf / NaN
            if (P.proj_mode == RFE_PROJ_INVZ) {
                const float invz = 1.f / z;
                u = P.fx * (x * invz) + P.cx; v = P.fy * (y * invz) + P.cy;
            } else {
                u = (P.fx * x) / z + P.cx; v = (P.fy * y) / z + P.cy;
            }
            rej = 3;
            if (u >= P.min_x && u < P.max_x && v >= P.min_y && v < P.max_y) {      // KeyFrame::IsInImage: half open, NaN fails
                const float ox = px - P.ow[0], oy = py - P.ow[1], oz = pz - P.ow[2];
                const float dist = sqrtf((ox * ox + oy * oy) + oz * oz);
                rej = 4;
                if (!(dist < min_dist[i] || dist > max_dist[i])) {
                    rej = 5;
                    if (!((ox * normal[3 * i] + oy * normal[3 * i + 1]) + oz * normal[3 * i + 2] < 0.5f * dist)) {
                        rej = 0;
                        lv = predict_scale_level(scale_dist[i], dist, P.log_scale_factor, P.nlevels);
                        r = (float)P.th * level_table(P.scale_factors, lv);
                    }
                }
            }
        }
    }
    if (rej != 0) { u = 0.f; v = 0.f; }
    if (i < Np) {
        proj[2 * i] = u; proj[2 * i + 1] = v; radius[i] = r; level[i] = lv;
        if (reject) reject[i] = rej;
    }
    const unsigned long long searched = __ballot(i < Np && rej == 0);
    if ((threadIdx.x & 63) == 0 && searched) atomicAdd(&stats[4], (int)__popcll(searched));
}

void launch_sim3_project(hipStream_t s, const rfe_sim3_params& P, const float* pw, const float* normal, const float* min_dist,
                         const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np, float* proj, float* radius,
                         int32_t* level, int32_t* reject, int32_t* stats) {
    if (Np <= 0) return;
    hipLaunchKernelGGL(sim3_project_kernel, dim3((Np + 255) / 256), dim3(256), 0, s, P, pw, normal, min_dist, max_dist, scale_dist, valid, Np,
                       proj, radius, level, reject, stats);
}

}  // namespace rfe
