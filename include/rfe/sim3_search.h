// rfe/sim3_search.h -- drop-in bodies for the two Sim3 SearchByProjection overloads of loop closing on top of
// rfe_search_by_projection_sim3:
//   SPmatcher::SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming)
//       (reference src/Matchers/SPmatcher.cc:1558-1669, called from src/LoopClosing.cc:1477)
//   SPmatcher::SearchByProjection(KeyFrame*, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)
//       (:2076-2182, called from LoopClosing.cc:1508 and :1774)
// The transform, projection, gates, PredictScale, the candidate lists, the scan and the loop's sequential assignment run on the device in
// one call.  Works on any KeyFrame-like / MapPoint-like / Sim3-like triple with the reference's member names:
//   KeyFrame: NLeft, fx, fy, cx, cy, mnMinX, mnMinY, mnMaxX, mnMaxY, mnScaleLevels, mfLogScaleFactor, mvScaleFactors, mvKeysUn, mDescriptors
//   MapPoint: isBad(), GetWorldPos(), GetNormal() (indexable with (i)), GetMinDistanceInvariance(), GetMaxDistanceInvariance(),
//             GetDescriptor(), and GetMaxDistance() -- see below
//   Sim3:     rotationMatrix(), translation(), scale()
// MapPoint::PredictScale (src/MapPoint.cc:689-707) divides the BARE mfMaxDistance by the distance, while the distance gate compares with
// GetMaxDistanceInvariance() = 1.2f * mfMaxDistance (:668-672); with the usual scale factor 1.2 the two are one level apart.  mfMaxDistance
// is protected and PredictScale is its only reader, so the reference's MapPoint needs ONE added public member for this header:
//     float GetMaxDistance() { unique_lock<mutex> lock(mMutexPos); return mfMaxDistance; }        // include/MapPoint.h
// (dividing GetMaxDistanceInvariance() by 1.2f is not the same float.)
// SE3T is the caller's Sophus::SE3f, named at the call site: SearchByProjectionSim3_rfe<Sophus::SE3f>(ctx, pKF, Scw, ...).  The pose is
// built exactly as :1566 builds it -- SE3T(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) -- and the device gets its
// unit_quaternion(), translation() and inverse().translation(); it derives nothing itself.
// Pinhole, one camera: a two-camera keyframe (pKF->NLeft != -1) is refused with -1 and nothing is touched -- such a caller, and one with a
// KannalaBrandt8 camera, keeps the reference's loop.
// `ctx` can be the session of the extractor: mpSPextractorLeft->featureExtractor->ExtractorSession.
#pragma once
#include <algorithm>
#include <cstdint>
#include <set>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {
namespace rfe_detail {

// what both overloads share; on success `accepted[f]` is the index into vpPoints of the map point feature f got, or -1
template <class SE3T, class KeyFrameT, class Sim3T, class MapPointT>
int SearchSim3(rfe_ctx* ctx, KeyFrameT* pKF, Sim3T& Scw, const std::vector<MapPointT*>& vpPoints, const std::vector<MapPointT*>& vpMatched,
               int th, float th_accept, int proj_mode, int dist_mode, std::vector<int32_t>& accepted) {
    const int Np = (int)vpPoints.size(), Nf = (int)pKF->mvKeysUn.size();
    accepted.assign((size_t)Nf, -1);
    if (Np == 0 || Nf == 0) return 0;
    if ((int)vpMatched.size() < Nf || (int)pKF->mvScaleFactors.size() < pKF->mnScaleLevels) return RFE_ERR_INVALID;
    const SE3T Tcw(Scw.rotationMatrix(), Scw.translation() / Scw.scale());
    const auto quat = Tcw.unit_quaternion();
    rfe_sim3_params P = rfe_sim3_params();
    P.quat[0] = quat.x(); P.quat[1] = quat.y(); P.quat[2] = quat.z(); P.quat[3] = quat.w();
    copy_vec3(Tcw.translation(), P.t); copy_vec3(Tcw.inverse().translation(), P.ow);
    P.fx = pKF->fx; P.fy = pKF->fy; P.cx = pKF->cx; P.cy = pKF->cy;
    P.min_x = pKF->mnMinX; P.min_y = pKF->mnMinY; P.max_x = pKF->mnMaxX; P.max_y = pKF->mnMaxY;
    P.th = th; P.nlevels = pKF->mnScaleLevels; P.log_scale_factor = pKF->mfLogScaleFactor;
    copy_levels(pKF->mvScaleFactors, P.nlevels, P.scale_factors);
    P.proj_mode = proj_mode; P.dist_mode = dist_mode;

    std::set<MapPointT*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPointT*>(nullptr));
    std::vector<float> q((size_t)Np * 256), pw((size_t)Np * 3), normal((size_t)Np * 3), min_dist((size_t)Np), max_dist((size_t)Np),
        scale_dist((size_t)Np);
    std::vector<uint8_t> valid((size_t)Np), matched_in((size_t)Nf);
    gather_map_points(vpPoints, q.data(), pw.data(), normal.data(), min_dist.data(), max_dist.data(), scale_dist.data(),
                      [&](size_t i, MapPointT* pMP) { valid[i] = !pMP->isBad() && !spAlreadyFound.count(pMP); });
    std::vector<float> f((size_t)Nf * 256), kpts((size_t)Nf * 2);
    gather_features(pKF->mvKeysUn, pKF->mDescriptors, (size_t)Nf, kpts.data(), nullptr, f.data());
    for (int j = 0; j < Nf; ++j) matched_in[j] = vpMatched[j] != nullptr;
    return rfe_search_by_projection_sim3(ctx, &P, q.data(), pw.data(), normal.data(), min_dist.data(), max_dist.data(), scale_dist.data(),
                                         valid.data(), Np, f.data(), kpts.data(), nullptr, matched_in.data(), Nf, th_accept, accepted.data(),
                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

}  // namespace rfe_detail

// Both return nmatches like the reference (>= 0); -1 for a refused keyframe, a negative rfe_status when the library refuses or fails
// (vpMatched / vpMatchedKF untouched).  th_low is SPmatcher::TH_LOW.

// :1558-1669: float distances, u = fx * (x * (1 / z)) + cx, accepted when bestDist <= TH_LOW (ratioHamming is unused there)
template <class SE3T, class KeyFrameT, class Sim3T, class MapPointT>
int SearchByProjectionSim3_rfe(rfe_ctx* ctx, KeyFrameT* pKF, Sim3T& Scw, const std::vector<MapPointT*>& vpPoints,
                               const std::vector<KeyFrameT*>& vpPointsKFs, std::vector<MapPointT*>& vpMatched,
                               std::vector<KeyFrameT*>& vpMatchedKF, int th, float /*ratioHamming*/, const float th_low = 1.2f) {
    if (pKF->NLeft != -1) return -1;
    if (vpPointsKFs.size() < vpPoints.size() || vpMatchedKF.size() < vpMatched.size()) return RFE_ERR_INVALID;
    std::vector<int32_t> accepted;
    const int n = rfe_detail::SearchSim3<SE3T>(ctx, pKF, Scw, vpPoints, vpMatched, th, th_low, RFE_PROJ_INVZ, RFE_DIST_FLOAT, accepted);
    if (n < 0) return n;
    for (size_t j = 0; j < accepted.size(); ++j)
        if (accepted[j] >= 0) { vpMatched[j] = vpPoints[accepted[j]]; vpMatchedKF[j] = vpPointsKFs[accepted[j]]; }
    return n;
}

// :2076-2182: Pinhole::project, `int dist`, accepted when bestDist <= TH_LOW * ratioHamming
template <class SE3T, class KeyFrameT, class Sim3T, class MapPointT>
int SearchByProjectionSim3_rfe(rfe_ctx* ctx, KeyFrameT* pKF, Sim3T& Scw, const std::vector<MapPointT*>& vpPoints,
                               std::vector<MapPointT*>& vpMatched, int th, float ratioHamming, const float th_low = 1.2f) {
    if (pKF->NLeft != -1) return -1;
    std::vector<int32_t> accepted;
    const int n = rfe_detail::SearchSim3<SE3T>(ctx, pKF, Scw, vpPoints, vpMatched, th, th_low * ratioHamming, RFE_PROJ_DIV, RFE_DIST_TRUNC,
                                               accepted);
    if (n < 0) return n;
    for (size_t j = 0; j < accepted.size(); ++j)
        if (accepted[j] >= 0) vpMatched[j] = vpPoints[accepted[j]];
    return n;
}

}  // namespace ORB_SLAM3
