// rfe/global_ba.h -- drop-ins for Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) and
// Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag, nLoopKF, bRobust) (reference src/Optimizer.cc:2813-3220) on top of
// rfe_global_ba: the vertices and edges are gathered on the host as the reference writes them, sorted and packed;
// optimize(nIterations) runs on the device; poses and positions are written back as :3106-3219.
// Works on any KeyFrame / MapPoint / Map-like classes with the reference's member names:
//   KeyFrame: mnId, isBad(), GetMap(), GetPose() / SetPose() as rfe/pose_optimization.h, mTcwGBA (assignable from GetPose()'s type),
//     mnBAGlobalForKF, mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf, mpCamera (GetType()), mpCamera2
//   MapPoint: mnId, isBad(), GetObservations() (a map KeyFrame* -> tuple<int, int>), GetWorldPos() / SetWorldPos() (a vector indexable
//     with (i) and constructible from (x, y, z)), mPosGBA, mnBAGlobalForKF, UpdateNormalAndDepth()
//   Map: GetInitKFid(), GetOriginKF() (-> mnId), GetAllKeyFrames(), GetAllMapPoints()
// Order handed to the library: the keyframes that are not bad in ascending mnId (g2o's Hessian order is the ascending vertex id), the one
// with mnId == GetInitKFid() fixed; the points that are not bad in ascending mnId; the edges by (point, keyframe), the packing and sort
// of rfe/local_ba.h.  The reference adds a point's edges in the pointer order of its observation map; the sorted order is this entry's
// canonical replacement (6l, departure (a)).  An observation on a keyframe that is bad, has no vertex or has mnId > maxKFid is skipped
// (:2953-2956); one without a left index counts for vbNotIncludedMP (:2957) and adds no edge.
// Write-back as written: when nLoopKF == pMap->GetOriginKF()->mnId, SetPose and SetWorldPos + UpdateNormalAndDepth; otherwise mTcwGBA,
// mPosGBA and mnBAGlobalForKF on both.  A point no observation counted for (vbNotIncludedMP), or whose observations all lack a left
// index (included == 0: the reference would hand it back its own position), is left alone.  The pose handed over is
// PoseT(QuatT(w, x, y, z) of the float casts, VecT): the Sophus constructors normalise on the caller's side (6m's float-pose note).
// Returns the number of LM iterations run (>= 0).  RFE_GBA_NOT_SERVED and nothing touched (the caller keeps the reference's function): no
// keyframe that is not bad, a keyframe with mpCamera2 (EdgeSE3ProjectXYZToBody), a KannalaBrandt8 camera, a level table that is empty or
// longer than RFE_MAX_LEVELS, a problem over RFE_GBA_MAX_KF, RFE_GBA_MAX_POINTS, RFE_GBA_MAX_EDGES or RFE_GBA_MAX_PAIRS.  A negative
// rfe_status when the library refuses or fails.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <tuple>
#include <type_traits>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

enum { RFE_GBA_NOT_SERVED = -12 };

template <class KeyFrameT, class MapPointT>
int BundleAdjustment_rfe(rfe_ctx* ctx, const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP, int nIterations,
                         bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust, int32_t* stats_out = nullptr /*[8], as rfe_global_ba*/) {
    // the vertices, :2894-2912 and :2921-2939, in the order the library takes them
    std::vector<KeyFrameT*> kfs;
    for (KeyFrameT* pKF : vpKFs)
        if (!pKF->isBad()) kfs.push_back(pKF);
    if (kfs.empty()) return RFE_GBA_NOT_SERVED;
    auto* pMap = vpKFs[0]->GetMap();
    std::sort(kfs.begin(), kfs.end(), [](const KeyFrameT* a, const KeyFrameT* b) { return a->mnId < b->mnId; });
    const long unsigned int maxKFid = kfs.back()->mnId;
    std::vector<MapPointT*> mps;
    for (MapPointT* pMP : vpMP)
        if (!pMP->isBad()) mps.push_back(pMP);
    std::sort(mps.begin(), mps.end(), [](const MapPointT* a, const MapPointT* b) { return a->mnId < b->mnId; });
    const int K = (int)kfs.size(), L = (int)mps.size();
    for (KeyFrameT* pKF : kfs)
        if (pKF->mpCamera2 || (pKF->mpCamera && pKF->mpCamera->GetType() != 0 /*CAM_PINHOLE*/) || pKF->mvInvLevelSigma2.empty() ||
            pKF->mvInvLevelSigma2.size() > RFE_MAX_LEVELS)
            return RFE_GBA_NOT_SERVED;
    if (K > RFE_GBA_MAX_KF || L > RFE_GBA_MAX_POINTS) return RFE_GBA_NOT_SERVED;
    std::map<KeyFrameT*, int> kf_index;
    for (int k = 0; k < K; ++k) kf_index[kfs[k]] = k;
    std::vector<uint8_t> fixed(K);
    for (int k = 0; k < K; ++k) fixed[k] = kfs[k]->mnId == pMap->GetInitKFid() ? 1 : 0;
    // the edges, :2942-3080, by (point, keyframe)
    struct EdgeRec { int p, k, feat; };
    std::vector<EdgeRec> edges;
    std::vector<uint8_t> counted(std::max(L, 1), 0);         // !vbNotIncludedMP
    long long pairs = 0;
    for (int p = 0; p < L; ++p) {
        const auto observations = mps[p]->GetObservations();
        const size_t first = edges.size();
        long long nfree = 0;
        for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrameT* pKF = mit->first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;
            const auto at = kf_index.find(pKF);
            if (at == kf_index.end()) continue;
            counted[p] = 1;
            const int leftIndex = std::get<0>(mit->second);
            if (leftIndex == -1) continue;
            edges.push_back(EdgeRec{p, at->second, leftIndex});
            if (!fixed[at->second]) ++nfree;
        }
        std::sort(edges.begin() + first, edges.end(), [](const EdgeRec& a, const EdgeRec& b) { return a.k < b.k; });
        pairs += nfree * (nfree + 1) / 2;
        if (edges.size() > (size_t)RFE_GBA_MAX_EDGES || pairs > RFE_GBA_MAX_PAIRS) return RFE_GBA_NOT_SERVED;
    }
    const int E = (int)edges.size();

    // pack: per keyframe its pose, camera and level table, and the features its edges observe, in edge order
    std::vector<float> kf_pose((size_t)K * 7), kf_cam((size_t)K * 5), kf_sigma2((size_t)K * RFE_MAX_LEVELS, 0.f), xw((size_t)std::max(L, 1) * 3);
    std::vector<int32_t> kf_nlevels(K), kf_feat_off(K + 1, 0), edge_point(std::max(E, 1)), edge_kf(std::max(E, 1)), edge_feat(std::max(E, 1));
    for (int k = 0; k < K; ++k) {
        const auto Tcw = kfs[k]->GetPose();
        const auto q = Tcw.unit_quaternion();
        const auto t = Tcw.translation();
        const float pose[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
        std::copy(pose, pose + 7, &kf_pose[(size_t)k * 7]);
        const float cam[5] = {kfs[k]->fx, kfs[k]->fy, kfs[k]->cx, kfs[k]->cy, kfs[k]->mbf};
        std::copy(cam, cam + 5, &kf_cam[(size_t)k * 5]);
        kf_nlevels[k] = (int32_t)kfs[k]->mvInvLevelSigma2.size();
        rfe_detail::copy_levels(kfs[k]->mvInvLevelSigma2, kf_nlevels[k], &kf_sigma2[(size_t)k * RFE_MAX_LEVELS]);
    }
    for (int p = 0; p < L; ++p) rfe_detail::copy_vec3(mps[p]->GetWorldPos(), &xw[(size_t)p * 3]);
    for (const EdgeRec& e : edges) ++kf_feat_off[e.k + 1];
    for (int k = 0; k < K; ++k) kf_feat_off[k + 1] += kf_feat_off[k];
    const int Nf = kf_feat_off[K];
    std::vector<float> kpts((size_t)std::max(Nf, 1) * 2), uright(std::max(Nf, 1));
    std::vector<int32_t> octave(std::max(Nf, 1)), next(kf_feat_off.begin(), kf_feat_off.end() - 1);
    for (int e = 0; e < E; ++e) {
        const EdgeRec& r = edges[e];
        const int f = next[r.k]++;
        edge_point[e] = r.p; edge_kf[e] = r.k; edge_feat[e] = f - kf_feat_off[r.k];
        const auto& kp = kfs[r.k]->mvKeysUn[r.feat];
        kpts[2 * (size_t)f] = kp.pt.x; kpts[2 * (size_t)f + 1] = kp.pt.y; octave[f] = kp.octave;
        uright[f] = kfs[r.k]->mvuRight[r.feat];
    }
    rfe_global_ba_params prm = rfe_global_ba_params();
    prm.iterations = nIterations; prm.max_trials = 10;
    prm.user_lambda_init = 0.0;
    prm.robust = bRobust ? 1 : 0;
    prm.huber2_mono = 5.99; prm.huber2_stereo = 7.815;       // `sqrt(5.99)`, `sqrt(7.815)`, :2915-2916
    prm.stop = reinterpret_cast<const volatile uint8_t*>(pbStopFlag);
    std::vector<double> pose((size_t)K * 7), point((size_t)std::max(L, 1) * 3);
    std::vector<float> pose_f32(pose.size()), point_f32(point.size());
    std::vector<uint8_t> included(std::max(L, 1));
    int32_t stats[8];
    const int rc = rfe_global_ba(ctx, prm, kf_pose.data(), kf_cam.data(), kf_nlevels.data(), kf_sigma2.data(), kf_feat_off.data(), fixed.data(),
                                 kpts.data(), octave.data(), uright.data(), xw.data(), edge_point.data(), edge_kf.data(), edge_feat.data(), K, L, E,
                                 Nf, pose.data(), pose_f32.data(), point.data(), point_f32.data(), included.data(), nullptr, nullptr, stats);
    if (rc < 0) return rc;
    if (stats_out) for (int k = 0; k < 8; ++k) stats_out[k] = stats[k];
    // :3106-3219
    const bool direct = nLoopKF == pMap->GetOriginKF()->mnId;
    for (int k = 0; k < K; ++k) {
        const auto Tcw = kfs[k]->GetPose();
        using PoseT = typename std::decay<decltype(Tcw)>::type;
        using QuatT = typename std::decay<decltype(Tcw.unit_quaternion())>::type;
        using VecT = typename std::decay<decltype(Tcw.translation())>::type;
        const float* o = &pose_f32[(size_t)k * 7];
        const PoseT T(QuatT(o[3], o[0], o[1], o[2]), VecT(o[4], o[5], o[6]));
        if (direct) {
            kfs[k]->SetPose(T);
        } else {
            kfs[k]->mTcwGBA = T;
            kfs[k]->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (int p = 0; p < L; ++p) {
        if (!counted[p] || !included[p]) continue;
        using PosT = typename std::decay<decltype(mps[p]->GetWorldPos())>::type;
        const float* o = &point_f32[(size_t)p * 3];
        if (direct) {
            mps[p]->SetWorldPos(PosT(o[0], o[1], o[2]));
            mps[p]->UpdateNormalAndDepth();
        } else {
            mps[p]->mPosGBA = PosT(o[0], o[1], o[2]);
            mps[p]->mnBAGlobalForKF = nLoopKF;
        }
    }
    return rc;
}

template <class MapT>
int GlobalBundleAdjustemnt_rfe(rfe_ctx* ctx, MapT* pMap, int nIterations = 5, bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0,
                               const bool bRobust = true, int32_t* stats_out = nullptr) {
    const auto vpKFs = pMap->GetAllKeyFrames();
    const auto vpMP = pMap->GetAllMapPoints();
    return BundleAdjustment_rfe(ctx, vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, stats_out);
}

}  // namespace ORB_SLAM3
