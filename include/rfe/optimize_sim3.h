// rfe/optimize_sim3.h -- drop-in for Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4195-4494) on top of rfe_optimize_sim3
// (DESIGN.md 6k): the gather of the reference's first loop on the host, both Levenberg-Marquardt rounds and the two chi2 checks in one
// device call.
// Works on any KeyFrame / MapPoint / Sim3 / 7x7-matrix classes with the reference's member names:
//   KeyFrame: GetRotation() (indexable with (r, c)), GetTranslation() (with (i)), GetMapPointMatches(), mvKeysUn, mvInvLevelSigma2, fx, fy,
//             cx, cy, mpCamera->GetType();  MapPoint: isBad(), GetIndexInKeyFrame(pKF) (std::get<0> is the index), GetWorldPos() (with (i));
//   Sim3 (g2o::Sim3): rotation() with x() y() z() w() and a (w, x, y, z) constructor, translation() (with (i)) and an (x, y, z)
//             constructor, scale(), and the (quaternion, vector, double) constructor;  the matrix (Eigen::Matrix<double, 7, 7>): setZero().
// Effects, as the reference's: vpMatches1[i] is nulled exactly where a chi2 check removes the pair, g2oS12 is written only when the
// second round ran (not on `return 0` at :4457), mAcumHessian is zeroed only on that path (:4465 -- the reference never fills it), and
// the return value is nIn.
// Stated differences: a KannalaBrandt8 camera on either keyframe, more than 4096 matches or more than 4096 keypoints in pKF2, or an empty
// mvInvLevelSigma2 are refused: RFE_OPTIMIZE_SIM3_NOT_SERVED (-100) comes back and nothing is touched (keep the reference's function for
// those).  Any other negative value is the library's rfe_status (-1 RFE_ERR_INVALID, ...).  stats, when given, receives
// rfe_optimize_sim3's stats [8].
#pragma once
#include <algorithm>
#include <cstdint>
#include <tuple>
#include <type_traits>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

enum { RFE_OPTIMIZE_SIM3_NOT_SERVED = -100 };    // apart from every rfe_status

template <class KeyFrameT, class MapPointT, class Sim3T, class HessianT>
int OptimizeSim3_rfe(rfe_ctx* ctx, KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, const float th2,
                     const bool bFixScale, HessianT& mAcumHessian, const bool bAllPoints = false, int32_t* stats = nullptr) {
    const size_t N = vpMatches1.size(), N2 = pKF2->mvKeysUn.size();
    const size_t L1 = pKF1->mvInvLevelSigma2.size(), L2 = pKF2->mvInvLevelSigma2.size();
    if (pKF1->mpCamera->GetType() != 0 || pKF2->mpCamera->GetType() != 0 /*GeometricCamera::CAM_PINHOLE*/) return RFE_OPTIMIZE_SIM3_NOT_SERVED;
    if (N > 4096 || N2 > 4096 || L1 == 0 || L2 == 0 || pKF1->mvKeysUn.size() < N) return RFE_OPTIMIZE_SIM3_NOT_SERVED;
    rfe_optimize_sim3_params P = rfe_optimize_sim3_params();
    rfe_detail::copy_rotation(pKF1->GetRotation(), P.rcw1); rfe_detail::copy_vec3(pKF1->GetTranslation(), P.tcw1);
    rfe_detail::copy_rotation(pKF2->GetRotation(), P.rcw2); rfe_detail::copy_vec3(pKF2->GetTranslation(), P.tcw2);
    P.fx1 = pKF1->fx; P.fy1 = pKF1->fy; P.cx1 = pKF1->cx; P.cy1 = pKF1->cy;
    P.fx2 = pKF2->fx; P.fy2 = pKF2->fy; P.cx2 = pKF2->cx; P.cy2 = pKF2->cy;
    P.nlevels1 = (int32_t)std::min<size_t>(L1, RFE_MAX_LEVELS); rfe_detail::copy_levels(pKF1->mvInvLevelSigma2, P.nlevels1, P.inv_level_sigma2_1);
    P.nlevels2 = (int32_t)std::min<size_t>(L2, RFE_MAX_LEVELS); rfe_detail::copy_levels(pKF2->mvInvLevelSigma2, P.nlevels2, P.inv_level_sigma2_2);
    P.th2 = th2; P.fix_scale = bFixScale ? 1 : 0; P.all_points = bAllPoints ? 1 : 0; P.n = (int32_t)N; P.n2 = (int32_t)N2;

    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<float> xw1(3 * N + 1, 0.f), xw2(3 * N + 1, 0.f), kpts1(2 * N + 1), kpts2(2 * N2 + 1);
    std::vector<int32_t> octave1(N + 1), octave2(N2 + 1), idx2(N + 1, -1);
    std::vector<uint8_t> valid(N + 1, 0), keep(N + 1, 1);
    rfe_detail::gather_keypoints(pKF1->mvKeysUn, N, kpts1.data(), octave1.data());
    rfe_detail::gather_keypoints(pKF2->mvKeysUn, N2, kpts2.data(), octave2.data());
    for (size_t i = 0; i < N; ++i) {                                   // :4254-4319: which rows hold two good map points
        MapPointT* pMP2 = vpMatches1[i];
        if (!pMP2) continue;
        MapPointT* pMP1 = i < vpMapPoints1.size() ? vpMapPoints1[i] : nullptr;
        idx2[i] = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
        if (!pMP1 || pMP1->isBad() || pMP2->isBad()) continue;
        valid[i] = 1;
        rfe_detail::copy_vec3(pMP1->GetWorldPos(), &xw1[3 * i]);
        rfe_detail::copy_vec3(pMP2->GetWorldPos(), &xw2[3 * i]);
    }
    const auto q = g2oS12.rotation();
    const auto t = g2oS12.translation();
    const double s12_0[8] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2), g2oS12.scale()};
    double s12[8];
    int32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = rfe_optimize_sim3(ctx, &P, s12_0, xw1.data(), xw2.data(), valid.data(), kpts1.data(), octave1.data(), idx2.data(),
                                     kpts2.data(), octave2.data(), 1, (int)N, (int)N2, s12, nullptr, keep.data(), nullptr, nullptr, st);
    if (rc < 0) return rc;
    if (stats) for (int k = 0; k < 8; ++k) stats[k] = st[k];
    for (size_t i = 0; i < N; ++i)
        if (!keep[i]) vpMatches1[i] = static_cast<MapPointT*>(nullptr);
    if (st[7] & 16) return 0;                                          // :4456-4457: before mAcumHessian and g2oS12 are written
    mAcumHessian.setZero();
    typedef typename std::decay<decltype(g2oS12.rotation())>::type QuatT;
    typedef typename std::decay<decltype(g2oS12.translation())>::type VecT;
    g2oS12 = Sim3T(QuatT(s12[3], s12[0], s12[1], s12[2]), VecT(s12[4], s12[5], s12[6]), s12[7]);
    return st[0];
}

}  // namespace ORB_SLAM3
