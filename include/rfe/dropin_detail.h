// rfe/dropin_detail.h -- the host gathers the drop-in headers of this directory share: the reference's poses, level tables, descriptor rows,
// keypoints and map points into the flat arrays the C ABI takes.  Templates and inline functions only; every helper makes one pass and
// writes into memory the caller owns.  Travels with the headers that include it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../rover_fe.h"
#include "cv_compat.h"

namespace ORB_SLAM3 {
namespace rfe_detail {

// a rotation indexable with (r, c) into float[9], row-major; a vector indexable with (i) into float[3]
template <class RotT> inline void copy_rotation(const RotT& R, float* dst) { for (int k = 0; k < 9; ++k) dst[k] = R(k / 3, k % 3); }
template <class VecT> inline void copy_vec3(const VecT& v, float* dst) { for (int k = 0; k < 3; ++k) dst[k] = v(k); }
// the first min(nlevels, RFE_MAX_LEVELS) entries of a per-level vector (mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2)
template <class LevelsT> inline void copy_levels(const LevelsT& v, int nlevels, float* dst) { for (int l = 0; l < nlevels && l < RFE_MAX_LEVELS; ++l) dst[l] = v[l]; }
// one 256-float descriptor row
inline void copy_descriptor(const cv::Mat& m, int row, float* dst) { const float* s = m.ptr<float>(row); std::copy(s, s + 256, dst); }

// mvKeysUn / mvKeys -> kpts [n,2] and, when asked for, octave [n]
template <class KeysT>
inline void gather_keypoints(const KeysT& keys, size_t n, float* kpts, int32_t* octave = nullptr) {
    for (size_t j = 0; j < n; ++j) {
        kpts[2 * j] = keys[j].pt.x; kpts[2 * j + 1] = keys[j].pt.y;
        if (octave) octave[j] = keys[j].octave;
    }
}
// the same, and mDescriptors -> f [n,256]
template <class KeysT>
inline void gather_features(const KeysT& keys, const cv::Mat& desc, size_t n, float* kpts, int32_t* octave, float* f) {
    gather_keypoints(keys, n, kpts, octave);
    for (size_t j = 0; j < n; ++j) copy_descriptor(desc, (int)j, f + j * 256);
}
// mvpMapPoints -> skip [n]: the feature holds a map point somebody observes
template <class MapPointT>
inline void gather_skip(const std::vector<MapPointT*>& mps, size_t n, uint8_t* skip) {
    for (size_t j = 0; j < n; ++j) skip[j] = mps[j] && mps[j]->Observations() > 0;
}
// map points -> q [N,256], pw [N,3], normal [N,3], min_dist, max_dist, scale_dist [N].  flags(i, pMP) runs first for every point: the valid /
// observed predicates differ between the searches and stay with the caller.  Every accessor is called once per point, in this order.
template <class MapPointT, class FlagsT>
inline void gather_map_points(const std::vector<MapPointT*>& vp, float* q, float* pw, float* normal, float* min_dist, float* max_dist,
                              float* scale_dist, FlagsT flags) {
    for (size_t i = 0; i < vp.size(); ++i) {
        MapPointT* pMP = vp[i];
        flags(i, pMP);
        copy_vec3(pMP->GetWorldPos(), pw + 3 * i);
        copy_vec3(pMP->GetNormal(), normal + 3 * i);
        min_dist[i] = pMP->GetMinDistanceInvariance(); max_dist[i] = pMP->GetMaxDistanceInvariance();
        scale_dist[i] = pMP->GetMaxDistance();                        // what PredictScale divides, not the gate's 1.2f * mfMaxDistance
        copy_descriptor(pMP->GetDescriptor(), 0, q + 256 * i);
    }
}

}  // namespace rfe_detail
}  // namespace ORB_SLAM3
