// rfe/projection_search.h -- drop-in body for SPmatcher::SearchByProjection1 (reference src/Matchers/SPmatcher.cc:1170-1354, called from
// Tracking::SearchLocalPoints at src/Tracking.cc:4178 on every tracked frame) on top of rfe_search_by_projection: the feature grid, the
// candidate lists, the scan and the loop's sequential assignment run on the device in one call.
// Works on any Frame-like / MapPoint-like pair with the reference's member names:
//   Frame:    Nleft, mvKeysUn, mDescriptors, mvpMapPoints, mvScaleFactors, mnMinX, mnMinY, mnMaxX, mnMaxY
//   MapPoint: mbTrackInView, mTrackDepth, mTrackViewCos, mTrackProjX, mTrackProjY, isBad(), Observations(), GetDescriptor()
// Left-camera branch only: a two-camera rig (F.Nleft != -1, right-camera branch :1285-1351) is refused with -1 and nothing is touched --
// such a caller keeps SPmatcher::SearchByProjection1.
// `ctx` can be the session of the extractor: mpSPextractorLeft->featureExtractor->ExtractorSession.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

// SPmatcher::RadiusByViewingCos (src/Matchers/SPmatcher.cc:1357-1364)
inline float RadiusByViewingCos_rfe(float viewCos) { return viewCos > 0.998f ? 2.5f : 4.0f; }

// returns nmatches like the reference (>= 0); -1 for a refused frame, a negative rfe_status when the library refuses or fails (F untouched)
template <class FrameT, class MapPointT>
int SearchByProjection1_rfe(rfe_ctx* ctx, FrameT& F, const std::vector<MapPointT*>& vpMapPoints, const float th, const bool bFarPoints,
                            const float thFarPoints, const float th_high = 1.4f /*SPmatcher::TH_HIGH*/) {
    if (F.Nleft != -1) return -1;
    const bool bFactor = th != 1.0f;
    std::vector<int> sel;                          // vpMapPoints indices that reach the search, in the loop's order (:1178-1190)
    sel.reserve(vpMapPoints.size());
    for (size_t i = 0; i < vpMapPoints.size(); ++i) {
        MapPointT* pMP = vpMapPoints[i];
        if (!pMP->mbTrackInView) continue;
        if (bFarPoints && pMP->mTrackDepth > thFarPoints) continue;
        if (pMP->isBad()) continue;
        sel.push_back((int)i);
    }
    const int Nq = (int)sel.size(), Nf = (int)F.mvKeysUn.size();
    if (Nq == 0 || Nf == 0) return 0;
    std::vector<float> q((size_t)Nq * 256), proj((size_t)Nq * 2), radius((size_t)Nq);
    std::vector<uint8_t> observed((size_t)Nq), skip((size_t)Nf);
    for (int k = 0; k < Nq; ++k) {
        MapPointT* pMP = vpMapPoints[sel[k]];
        float r = RadiusByViewingCos_rfe(pMP->mTrackViewCos);
        if (bFactor) r *= th;
        radius[k] = r * F.mvScaleFactors[0];        // nPredictedLevel is 0 as the reference is written (:1193)
        proj[2 * k] = pMP->mTrackProjX; proj[2 * k + 1] = pMP->mTrackProjY;
        observed[k] = pMP->Observations() > 0;
        rfe_detail::copy_descriptor(pMP->GetDescriptor(), 0, &q[(size_t)k * 256]);
    }
    std::vector<float> f((size_t)Nf * 256), kpts((size_t)Nf * 2);
    std::vector<int32_t> octave((size_t)Nf), assign((size_t)Nf, -1);
    rfe_detail::gather_features(F.mvKeysUn, F.mDescriptors, (size_t)Nf, kpts.data(), octave.data(), f.data());
    rfe_detail::gather_skip(F.mvpMapPoints, (size_t)Nf, skip.data());
    const int n = rfe_search_by_projection(ctx, q.data(), proj.data(), radius.data(), nullptr, observed.data(), Nq, f.data(), kpts.data(),
                                           nullptr, octave.data(), skip.data(), Nf, F.mnMinX, F.mnMinY, F.mnMaxX, F.mnMaxY, th_high,
                                           assign.data(), nullptr, nullptr, nullptr, nullptr);
    if (n < 0) return n;
    for (int j = 0; j < Nf; ++j)
        if (assign[j] >= 0) F.mvpMapPoints[j] = vpMapPoints[sel[assign[j]]];
    return n;
}

}  // namespace ORB_SLAM3
