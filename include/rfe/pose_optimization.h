// rfe/pose_optimization.h -- drop-in for Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:55-401) on top of
// rfe_pose_optimization: the four rounds of motion-only Levenberg-Marquardt and the chi2 classification between them run in
// one kernel; what comes back is the pose and mvbOutlier.
// Works on any Frame-like class with the reference's member names:
//   N, mvKeysUn, mvuRight, mvpMapPoints (entries with GetWorldPos(), indexable with (i)), mvInvLevelSigma2, fx, fy, cx, cy, mbf, mpCamera2,
//   mvbOutlier, GetPose() (unit_quaternion() with x() y() z() w(), translation() indexable with (i)) and SetPose(pose), where the pose type is
//   constructible from (quaternion(w, x, y, z), vector(x, y, z)) as Sophus::SE3f is from Eigen's -- that constructor normalises the cast
//   quaternion, as at :394-397.
// Returns the reference's value, nInitialCorrespondences - nBad (0 below three correspondences, with mvbOutlier cleared and the pose
// untouched, :270); -1 and nothing touched for a frame with a second camera (mpCamera2: EdgeSE3ProjectXYZOnlyPoseToBody is out of scope --
// such a caller keeps the reference's function); a negative rfe_status when the library refuses or fails.
// A caller whose frame is resident on the device calls rfe_pose_optimization_dev itself, between rfe_match_dev and
// rfe_search_local_points_dev.
#pragma once
#include <cstdint>
#include <type_traits>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

template <class FrameT>
int PoseOptimization_rfe(rfe_ctx* ctx, FrameT* pFrame, int32_t* stats_out = nullptr /*[8], as rfe_pose_optimization*/) {
    if (pFrame->mpCamera2) return -1;
    const int N = pFrame->N;
    const size_t n = (size_t)(N > 0 ? N : 0);
    if (N < 0 || N > 4096 || pFrame->mvInvLevelSigma2.empty() || pFrame->mvInvLevelSigma2.size() > RFE_MAX_LEVELS) return RFE_ERR_INVALID;
    rfe_pose_params P = rfe_pose_params();
    P.fx = pFrame->fx; P.fy = pFrame->fy; P.cx = pFrame->cx; P.cy = pFrame->cy; P.bf = pFrame->mbf;
    P.nlevels = (int32_t)pFrame->mvInvLevelSigma2.size();
    rfe_detail::copy_levels(pFrame->mvInvLevelSigma2, P.nlevels, P.inv_level_sigma2);
    const auto Tcw = pFrame->GetPose();
    const auto q0 = Tcw.unit_quaternion();
    const auto t0 = Tcw.translation();
    const float pose0[7] = {q0.x(), q0.y(), q0.z(), q0.w(), t0(0), t0(1), t0(2)};
    std::vector<float> kpts(n * 2), uright(n), xw(n * 3, 0.f);
    std::vector<int32_t> octave(n);
    std::vector<uint8_t> has_mp(n), outlier(n);
    for (size_t i = 0; i < n; ++i) {
        kpts[2 * i] = pFrame->mvKeysUn[i].pt.x; kpts[2 * i + 1] = pFrame->mvKeysUn[i].pt.y; octave[i] = pFrame->mvKeysUn[i].octave;
        uright[i] = pFrame->mvuRight[i];
        outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
        if (pFrame->mvpMapPoints[i]) {
            has_mp[i] = 1;
            rfe_detail::copy_vec3(pFrame->mvpMapPoints[i]->GetWorldPos(), &xw[3 * i]);
        }
    }
    double pose[7]; float pose_f32[7]; int32_t stats[8];
    const int rc = rfe_pose_optimization(ctx, &P, pose0, kpts.data(), octave.data(), uright.data(), xw.data(), has_mp.data(), nullptr, 1, N, pose,
                                         pose_f32, outlier.data(), nullptr, nullptr, stats);
    if (rc < 0) return rc;
    if (stats_out) for (int k = 0; k < 8; ++k) stats_out[k] = stats[k];
    for (size_t i = 0; i < n; ++i) if (has_mp[i]) pFrame->mvbOutlier[i] = outlier[i] != 0;
    if (stats[1] < 3) return 0;
    using PoseT = typename std::decay<decltype(Tcw)>::type;
    using QuatT = typename std::decay<decltype(q0)>::type;
    using VecT = typename std::decay<decltype(t0)>::type;
    pFrame->SetPose(PoseT(QuatT(pose_f32[3], pose_f32[0], pose_f32[1], pose_f32[2]), VecT(pose_f32[4], pose_f32[5], pose_f32[6])));
    return stats[0];
}

}  // namespace ORB_SLAM3
