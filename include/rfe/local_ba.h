// rfe/local_ba.h -- drop-in for Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges)
// (reference src/Optimizer.cc:1740-2188) on top of rfe_local_ba: steps 1-4 (the local keyframes, the local map points, the
// fixed keyframes) run on the host as the reference writes them; vertices and edges are sorted and packed; the robust optimize(10) and
// the classification run on the device; observations are erased and poses and positions written back under mMutexMapUpdate as :2153-2187.
// Works on any KeyFrame / MapPoint / Map-like classes with the reference's member names:
//   KeyFrame: mnId, mnBALocalForKF, mnBAFixedForKF, GetMap(), isBad(), GetVectorCovisibleKeyFrames(), GetMapPointMatches(), mvKeysUn,
//     mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf, mpCamera (GetType()), mpCamera2, GetPose() / SetPose() as rfe/pose_optimization.h,
//     EraseMapPointMatch(MapPoint*)
//   MapPoint: mnId, mnBALocalForKF, isBad(), GetMap(), GetObservations() (a map KeyFrame* -> tuple<int, int>), GetWorldPos() /
//     SetWorldPos() (a vector indexable with (i) and constructible from (x, y, z)), UpdateNormalAndDepth(), EraseObservation(KeyFrame*)
//   Map: GetInitKFid(), IsInertial(), mMutexMapUpdate, IncreaseChangeIndex(), msOptKFs, msFixedKFs
// Order handed to the library: the free keyframes in ascending mnId (g2o's Hessian order), then the fixed ones in ascending mnId -- a local
// keyframe that is the map's init keyframe goes with the fixed ones, setFixed(true) is all the reference does with it -- the points in
// ascending mnId, the edges by (point, keyframe).  The reference adds a point's edges in the pointer order of its observation map, which
// differs from run to run; the sorted order is this entry's canonical replacement (6l, departure (a)).
// Returns the number of erased observations (>= 0) after a run.  RFE_LBA_NO_FIXED_KF: num_fixedKF == 0 (:1851), RFE_LBA_STOPPED:
// *pbStopFlag was set (:2094); both return as the reference does, with the counters written (and, for RFE_LBA_STOPPED, msOptKFs / msFixedKFs refilled, :1879-1914) and nothing else touched.
// RFE_LBA_NOT_SERVED and no pose, position or observation touched (the caller keeps the reference's function): a keyframe with mpCamera2
// (EdgeSE3ProjectXYZToBody), a KannalaBrandt8 camera, more than RFE_LBA_MAX_FREE free keyframes, RFE_LBA_MAX_KF keyframes,
// RFE_LBA_MAX_POINTS points or RFE_LBA_MAX_EDGES edges.  A negative rfe_status when the library refuses or fails.
// A local keyframe that is the init keyframe keeps its pose (the reference hands it back the value it read).
// num_MPs receives the number of point vertices (the reference leaves it as it was).  The marks mnBALocalForKF / mnBAFixedForKF are
// written in every case, as by the reference.
#pragma once
#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

enum { RFE_LBA_NO_FIXED_KF = -10, RFE_LBA_STOPPED = -11, RFE_LBA_NOT_SERVED = -12 };

template <class KeyFrameT, class MapT>
int LocalBundleAdjustment_rfe(rfe_ctx* ctx, KeyFrameT* pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs,
                              int& num_edges, int32_t* stats_out = nullptr /*[8], as rfe_local_ba*/) {
    using MapPointT = typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type;
    // steps 1-4, :1744-1810
    std::list<KeyFrameT*> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    auto* pCurrentMap = pKF->GetMap();
    const std::vector<KeyFrameT*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = (int)vNeighKFs.size(); i < iend; i++) {
        KeyFrameT* pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lLocalKeyFrames.push_back(pKFi);
    }
    num_fixedKF = 0;
    std::list<MapPointT*> lLocalMapPoints;
    for (KeyFrameT* pKFi : lLocalKeyFrames) {
        if (pKFi->mnId == pMap->GetInitKFid()) num_fixedKF = 1;
        std::vector<MapPointT*> vpMPs = pKFi->GetMapPointMatches();
        for (MapPointT* pMP : vpMPs)
            if (pMP)
                if (!pMP->isBad() && pMP->GetMap() == pCurrentMap)
                    if (pMP->mnBALocalForKF != pKF->mnId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = pKF->mnId;
                    }
    }
    std::list<KeyFrameT*> lFixedCameras;
    for (MapPointT* pMP : lLocalMapPoints) {
        auto observations = pMP->GetObservations();
        for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrameT* pKFi = mit->first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
            }
        }
    }
    num_fixedKF = (int)lFixedCameras.size() + num_fixedKF;
    if (num_fixedKF == 0) return RFE_LBA_NO_FIXED_KF;

    // the vertices in the order the library takes them
    const auto by_id = [](const KeyFrameT* a, const KeyFrameT* b) { return a->mnId < b->mnId; };
    std::vector<KeyFrameT*> free_kf, fixed_kf(lFixedCameras.begin(), lFixedCameras.end());
    for (KeyFrameT* pKFi : lLocalKeyFrames) (pKFi->mnId == pMap->GetInitKFid() ? fixed_kf : free_kf).push_back(pKFi);
    std::sort(free_kf.begin(), free_kf.end(), by_id);
    std::sort(fixed_kf.begin(), fixed_kf.end(), by_id);
    std::vector<KeyFrameT*> kfs(free_kf);
    kfs.insert(kfs.end(), fixed_kf.begin(), fixed_kf.end());
    std::vector<MapPointT*> mps(lLocalMapPoints.begin(), lLocalMapPoints.end());
    std::sort(mps.begin(), mps.end(), [](const MapPointT* a, const MapPointT* b) { return a->mnId < b->mnId; });
    const int P = (int)free_kf.size(), K = (int)kfs.size(), L = (int)mps.size();
    num_OptKF = (int)lLocalKeyFrames.size();
    num_MPs = L;
    std::map<KeyFrameT*, int> kf_index;
    for (int k = 0; k < K; ++k) kf_index[kfs[k]] = k;
    for (KeyFrameT* pKFi : kfs)
        if (pKFi->mpCamera2 || (pKFi->mpCamera && pKFi->mpCamera->GetType() != 0 /*CAM_PINHOLE*/) || pKFi->mvInvLevelSigma2.empty() ||
            pKFi->mvInvLevelSigma2.size() > RFE_MAX_LEVELS)
            return RFE_LBA_NOT_SERVED;
    // the edges, :1965-2091, by (point, keyframe)
    struct EdgeRec { int p, k, feat; };
    std::vector<EdgeRec> edges;
    for (int p = 0; p < L; ++p) {
        const auto observations = mps[p]->GetObservations();
        const size_t first = edges.size();
        for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
            KeyFrameT* pKFi = mit->first;
            if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) {
                const int leftIndex = std::get<0>(mit->second);
                const auto at = kf_index.find(pKFi);
                if (leftIndex != -1 && at != kf_index.end()) edges.push_back(EdgeRec{p, at->second, leftIndex});
            }
        }
        std::sort(edges.begin() + first, edges.end(), [](const EdgeRec& a, const EdgeRec& b) { return a.k < b.k; });
    }
    const int E = (int)edges.size();
    num_edges = E;
    if (P > RFE_LBA_MAX_FREE || K > RFE_LBA_MAX_KF || L > RFE_LBA_MAX_POINTS || E > RFE_LBA_MAX_EDGES) return RFE_LBA_NOT_SERVED;
    // DEBUG LBA, :1879-1914: filled in front of the stop check, as the reference does
    pCurrentMap->msOptKFs.clear();
    pCurrentMap->msFixedKFs.clear();
    for (KeyFrameT* pKFi : lLocalKeyFrames) pCurrentMap->msOptKFs.insert(pKFi->mnId);
    for (KeyFrameT* pKFi : lFixedCameras) pCurrentMap->msFixedKFs.insert(pKFi->mnId);
    if (pbStopFlag)
        if (*pbStopFlag) return RFE_LBA_STOPPED;

    // pack: per keyframe its pose, camera and level table, and the features its edges observe, in edge order
    std::vector<float> kf_pose((size_t)K * 7), kf_cam((size_t)K * 5), kf_sigma2((size_t)K * RFE_MAX_LEVELS, 0.f), xw((size_t)L * 3);
    std::vector<int32_t> kf_nlevels(K), kf_feat_off(K + 1, 0), edge_point(E), edge_kf(E), edge_feat(E);
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
    std::vector<float> kpts((size_t)Nf * 2), uright(Nf);
    std::vector<int32_t> octave(Nf), next(kf_feat_off.begin(), kf_feat_off.end() - 1);
    for (int e = 0; e < E; ++e) {
        const EdgeRec& r = edges[e];
        const int f = next[r.k]++;
        edge_point[e] = r.p; edge_kf[e] = r.k; edge_feat[e] = f - kf_feat_off[r.k];
        const auto& kp = kfs[r.k]->mvKeysUn[r.feat];
        kpts[2 * (size_t)f] = kp.pt.x; kpts[2 * (size_t)f + 1] = kp.pt.y; octave[f] = kp.octave;
        uright[f] = kfs[r.k]->mvuRight[r.feat];
    }
    rfe_local_ba_params prm = rfe_local_ba_params();
    prm.iterations = 10; prm.max_trials = 10;
    prm.user_lambda_init = pMap->IsInertial() ? 100.0 : 0.0;
    prm.th2_mono = 5.991; prm.th2_stereo = 7.815;
    prm.stop = reinterpret_cast<const volatile uint8_t*>(pbStopFlag);
    std::vector<double> pose((size_t)std::max(P, 1) * 7), point((size_t)std::max(L, 1) * 3);
    std::vector<float> pose_f32(pose.size()), point_f32(point.size());
    std::vector<uint8_t> erase(std::max(E, 1));
    int32_t stats[8];
    const int rc = rfe_local_ba(ctx, prm, kf_pose.data(), kf_cam.data(), kf_nlevels.data(), kf_sigma2.data(), kf_feat_off.data(), kpts.data(),
                                octave.data(), uright.data(), xw.data(), edge_point.data(), edge_kf.data(), edge_feat.data(), P, K - P, L, E, Nf,
                                pose.data(), pose_f32.data(), point.data(), point_f32.data(), erase.data(), nullptr, nullptr, stats);
    if (rc < 0) return rc;
    if (stats_out) for (int k = 0; k < 8; ++k) stats_out[k] = stats[k];
    // :2107-2187
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    int erased = 0;
    for (int e = 0; e < E; ++e) {
        MapPointT* pMP = mps[edges[e].p];
        if (pMP->isBad()) continue;
        if (erase[e]) {
            KeyFrameT* pKFi = kfs[edges[e].k];
            pKFi->EraseMapPointMatch(pMP);
            pMP->EraseObservation(pKFi);
            ++erased;
        }
    }
    for (int k = 0; k < P; ++k) {
        const auto Tcw = free_kf[k]->GetPose();
        using PoseT = typename std::decay<decltype(Tcw)>::type;
        using QuatT = typename std::decay<decltype(Tcw.unit_quaternion())>::type;
        using VecT = typename std::decay<decltype(Tcw.translation())>::type;
        const float* o = &pose_f32[(size_t)k * 7];
        free_kf[k]->SetPose(PoseT(QuatT(o[3], o[0], o[1], o[2]), VecT(o[4], o[5], o[6])));
    }
    for (int p = 0; p < L; ++p) {
        using PosT = typename std::decay<decltype(mps[p]->GetWorldPos())>::type;
        const float* o = &point_f32[(size_t)p * 3];
        mps[p]->SetWorldPos(PosT(o[0], o[1], o[2]));
        mps[p]->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();
    return erased;
}

}  // namespace ORB_SLAM3
