// rfe/local_points_search.h -- drop-in body for steps 2 and 3 of Tracking::SearchLocalPoints (reference src/Tracking.cc:4119-4180), which run
// on every tracked frame: Frame::isInFrustum(pMP, 0.5) for every local map point (src/Frame.cc:703-795) and SPmatcher::SearchByProjection1
// over the points that passed (src/Matchers/SPmatcher.cc:1170-1283), on top of rfe_search_local_points.  The transform,
// projection, gates, PredictScale, the radius, the candidate lists, the scan and the loop's sequential assignment run on the device in one
// call; this header builds its arrays and writes back, per map point, exactly what isInFrustum leaves there.
// Works on any Frame-like / MapPoint-like pair with the reference's member names:
//   Frame:    Nleft, mnId, GetPose() (rotationMatrix() indexable with (r, c), translation() with (i): what UpdatePoseMatrices copies into
//             mRcw / mtcw), GetOw(), mpCamera->GetType(), fx, fy, cx, cy, mbf, mnMinX, mnMinY, mnMaxX, mnMaxY, mnScaleLevels,
//             mfLogScaleFactor, mvScaleFactors, mvKeysUn, mDescriptors, mvpMapPoints, mmProjectPoints
//   MapPoint: mnId, mnLastFrameSeen, isBad(), Observations(), IncreaseVisible(), GetWorldPos(), GetNormal() (indexable with (i)),
//             GetMinDistanceInvariance(), GetMaxDistanceInvariance(), GetDescriptor(), mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR,
//             mTrackDepth, mnTrackScaleLevel, mTrackViewCos, and GetMaxDistance(), the one accessor rfe/sim3_search.h already asks the
//             reference to add (MapPoint::PredictScale divides the bare mfMaxDistance, which no getter returns).
// One pinhole camera: a two-camera frame (F.Nleft != -1: isInFrustumChecks and the right-camera branch) and a KannalaBrandt8 camera are
// refused with -1 and nothing is touched -- such a caller keeps the reference's loops.
// RFE_SP_PYRAMID: built with -DRFE_SP_PYRAMID=1 the search runs at the predicted level (RFE_LEVEL_PREDICTED, ORB-SLAM3's form) instead of
// level 0 as SPmatcher.cc:1193 is written.
// `ctx` can be the session of the extractor: mpSPextractorLeft->featureExtractor->ExtractorSession.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

// returns nmatches like SearchByProjection1 (>= 0; 0 without a search when no point is in the frustum, as :4150); -1 for a refused frame, a
// negative rfe_status when the library refuses or fails (F and the map points untouched).  nToMatch, when given, receives the reference's
// count of points in the frustum.
template <class FrameT, class MapPointT>
int SearchLocalPoints_rfe(rfe_ctx* ctx, FrameT& F, const std::vector<MapPointT*>& vpLocalMapPoints, const float th, const bool bFarPoints,
                          const float thFarPoints, int* nToMatch = nullptr, const float th_high = 1.4f /*SPmatcher::TH_HIGH*/) {
    if (nToMatch) *nToMatch = 0;
    if (F.Nleft != -1 || F.mpCamera->GetType() != 0 /*GeometricCamera::CAM_PINHOLE*/) return -1;
    const int Np = (int)vpLocalMapPoints.size(), Nf = (int)F.mvKeysUn.size();
    if (Np == 0) return 0;
    if ((int)F.mvScaleFactors.size() < F.mnScaleLevels || (int)F.mvpMapPoints.size() < Nf) return RFE_ERR_INVALID;
    rfe_frustum_params P = rfe_frustum_params();
    const auto Tcw = F.GetPose();
    rfe_detail::copy_rotation(Tcw.rotationMatrix(), P.rcw); rfe_detail::copy_vec3(Tcw.translation(), P.tcw); rfe_detail::copy_vec3(F.GetOw(), P.ow);
    P.fx = F.fx; P.fy = F.fy; P.cx = F.cx; P.cy = F.cy; P.mbf = F.mbf;
    P.min_x = F.mnMinX; P.min_y = F.mnMinY; P.max_x = F.mnMaxX; P.max_y = F.mnMaxY;
    P.view_cos_limit = 0.5f;                                         // Tracking.cc:4136
    P.th = th; P.far_points = bFarPoints ? 1 : 0; P.th_far = thFarPoints;
    P.nlevels = F.mnScaleLevels; P.log_scale_factor = F.mfLogScaleFactor;
    rfe_detail::copy_levels(F.mvScaleFactors, P.nlevels, P.scale_factors);
#if defined(RFE_SP_PYRAMID) && RFE_SP_PYRAMID
    P.level_mode = RFE_LEVEL_PREDICTED;
#else
    P.level_mode = RFE_LEVEL_ZERO;
#endif

    const size_t np = (size_t)Np, nf = (size_t)Nf;
    std::vector<float> q(np * 256), pw(np * 3), normal(np * 3), min_dist(np), max_dist(np), scale_dist(np);
    std::vector<uint8_t> valid(np), observed(np), skip(nf);
    const auto flags = [&](size_t i, MapPointT* pMP) {                // :4129-4133
        valid[i] = pMP->mnLastFrameSeen != F.mnId && !pMP->isBad(); observed[i] = pMP->Observations() > 0;
    };
    rfe_detail::gather_map_points(vpLocalMapPoints, q.data(), pw.data(), normal.data(), min_dist.data(), max_dist.data(), scale_dist.data(), flags);
    std::vector<float> f(nf * 256), kpts(std::max<size_t>(nf, 1) * 2);   // a frame without features still passes "one of kpts and kxy"
    std::vector<int32_t> octave(nf), assign(nf, -1);
    rfe_detail::gather_features(F.mvKeysUn, F.mDescriptors, nf, kpts.data(), octave.data(), f.data());
    rfe_detail::gather_skip(F.mvpMapPoints, nf, skip.data());
    std::vector<float> proj(np * 2), proj_xr(np), depth(np), view_cos(np);
    std::vector<int32_t> level(np), reject(np), stats(8);
    const int n = rfe_search_local_points(ctx, &P, q.data(), pw.data(), normal.data(), min_dist.data(), max_dist.data(), scale_dist.data(),
                                          valid.data(), observed.data(), Np, f.data(), kpts.data(), nullptr, octave.data(), skip.data(), Nf,
                                          th_high, assign.data(), nullptr, nullptr, nullptr, proj.data(), proj_xr.data(), depth.data(),
                                          view_cos.data(), level.data(), reject.data(), stats.data());
    if (n < 0) return n;
    for (int i = 0; i < Np; ++i) {
        MapPointT* pMP = vpLocalMapPoints[i];
        const int rej = reject[i];
        if (rej == 1) continue;                                       // isInFrustum was not called
        pMP->mbTrackInView = false;                                   // Frame.cc:711-713, and what :740-741 overwrite behind the image gate
        pMP->mTrackProjX = proj[2 * (size_t)i];
        pMP->mTrackProjY = proj[2 * (size_t)i + 1];
        if (rej != 0 && rej != 6) continue;
        pMP->mbTrackInView = true;                                    // :778-791
        pMP->mTrackProjXR = proj_xr[i];
        pMP->mTrackDepth = depth[i];
        pMP->mnTrackScaleLevel = level[i];
        pMP->mTrackViewCos = view_cos[i];
        pMP->IncreaseVisible();                                       // Tracking.cc:4139
        F.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);   // :4143-4146
    }
    for (int j = 0; j < Nf; ++j)
        if (assign[j] >= 0) F.mvpMapPoints[j] = vpLocalMapPoints[assign[j]];
    if (nToMatch) *nToMatch = stats[4];
    return n;
}

}  // namespace ORB_SLAM3
