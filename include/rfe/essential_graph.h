// rfe/essential_graph.h -- drop-in for Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
// LoopConnections, bFixScale) (reference src/Optimizer.cc:4509-4840) on top of rfe_essential_graph: steps 2-4 (the
// vertices, the loop-connection edges, the spanning-tree, loop and covisibility edges) run on the host as the reference writes them; the
// two Sim3 tables and the sorted edge list are packed; optimize(20) and the map points' correction run on the device; poses and positions
// are written back under mMutexMapUpdate as :4787-4836.
// Works on any KeyFrame / MapPoint / Map-like classes with the reference's member names:
//   KeyFrame: mnId, isBad(), GetPose() / SetPose() as rfe/pose_optimization.h, GetParent(), GetLoopEdges(), GetCovisiblesByWeight(int),
//     hasChild(KeyFrame*), GetWeight(KeyFrame*), bImu, mPrevKF
//   MapPoint: isBad(), mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame(), GetWorldPos() / SetWorldPos() (a vector indexable
//     with (i) and constructible from (x, y, z)), UpdateNormalAndDepth()
//   Map: GetAllKeyFrames(), GetAllMapPoints(), GetInitKFid(), mMutexMapUpdate, IncreaseChangeIndex()
//   the Sim3 of KeyFrameAndPose: rotation() (x(), y(), z(), w()), translation() (indexable with (i)), scale()
// Order handed to the library: the keyframes that are not bad in ascending mnId (g2o's Hessian order is the ascending vertex id); the
// edges in the order the reference creates them -- step 3, then step 4 keyframe by keyframe -- stably sorted by (vertex 0, vertex 1), which
// keeps duplicates apart and replaces the pointer order of g2o's edge set (6m, departure (b)).
// A keyframe that is bad gets no vertex, as in the reference; the reference then hands optimizer.vertex() == NULL to addEdge for its
// step-4 edges, which g2o dereferences.  Here a bad keyframe adds no edge, no edge is added to a keyframe without a vertex, and its pose
// is not written (6m, departure (h)).  A point whose reference keyframe has no vertex keeps its position (SetWorldPos receives what
// GetWorldPos returned).  A pose that is not in CorrectedSim3 enters as (double) unit_quaternion normalised by sqrt(((x x + y y) + z z) +
// w w), (double) translation, scale 1.
// Returns the number of LM iterations run (>= 0).  RFE_EG_NOT_SERVED and nothing touched (the caller keeps the reference's function): a
// keyframe with bImu and mPrevKF (the inertial edge), more than RFE_EG_MAX_KF keyframes, RFE_EG_MAX_EDGES edges or RFE_EG_MAX_POINTS
// points, no keyframe at all.  A negative rfe_status when the library refuses or fails.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

enum { RFE_EG_NOT_SERVED = -12 };

namespace rfe_detail {
// a g2o::Sim3-like value -> qx qy qz qw tx ty tz s
template <class Sim3T> inline void copy_sim3(const Sim3T& S, double* dst) {
    const auto q = S.rotation();
    const auto t = S.translation();
    dst[0] = q.x(); dst[1] = q.y(); dst[2] = q.z(); dst[3] = q.w();
    for (int k = 0; k < 3; ++k) dst[4 + k] = t(k);
    dst[7] = S.scale();
}
}  // namespace rfe_detail

template <class MapT, class KeyFrameT, class PoseMapT, class ConnectionsT>
int OptimizeEssentialGraph_rfe(rfe_ctx* ctx, MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF, const PoseMapT& NonCorrectedSim3,
                               const PoseMapT& CorrectedSim3, const ConnectionsT& LoopConnections, const bool& bFixScale,
                               int32_t* stats_out = nullptr /*[8], as rfe_essential_graph*/) {
    const std::vector<KeyFrameT*> vpKFs = pMap->GetAllKeyFrames();
    const auto vpMPs = pMap->GetAllMapPoints();
    using MapPointT = typename std::remove_pointer<typename std::decay<decltype(vpMPs[0])>::type>::type;
    const int minFeat = 100;
    // step 2, :4553-4593: one vertex per keyframe that is not bad, in ascending mnId
    std::vector<KeyFrameT*> kfs;
    for (KeyFrameT* pKF : vpKFs)
        if (!pKF->isBad()) kfs.push_back(pKF);
    std::sort(kfs.begin(), kfs.end(), [](const KeyFrameT* a, const KeyFrameT* b) { return a->mnId < b->mnId; });
    const int N = (int)kfs.size();
    if (N < 1 || N > RFE_EG_MAX_KF) return RFE_EG_NOT_SERVED;
    for (KeyFrameT* pKF : kfs)
        if (pKF->bImu && pKF->mPrevKF) return RFE_EG_NOT_SERVED;
    std::map<long unsigned int, int> index;
    for (int k = 0; k < N; ++k) index[kfs[k]->mnId] = k;
    const auto vertex = [&](const KeyFrameT* pKF) {
        const auto at = index.find(pKF->mnId);
        return at == index.end() ? -1 : at->second;
    };
    std::vector<double> s_est((size_t)N * 8), s_meas((size_t)N * 8);
    std::vector<uint8_t> fixed(N);
    for (int k = 0; k < N; ++k) {
        KeyFrameT* pKF = kfs[k];
        double* e = &s_est[(size_t)k * 8];
        const auto it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {
            rfe_detail::copy_sim3(it->second, e);
        } else {
            const auto Tcw = pKF->GetPose();
            const auto q = Tcw.unit_quaternion();
            const auto t = Tcw.translation();
            const double x = (double)q.x(), y = (double)q.y(), z = (double)q.z(), w = (double)q.w();
            const double n = std::sqrt(((x * x + y * y) + z * z) + w * w);
            e[0] = x / n; e[1] = y / n; e[2] = z / n; e[3] = w / n;
            for (int c = 0; c < 3; ++c) e[4 + c] = (double)t(c);
            e[7] = 1.0;
        }
        const auto itn = NonCorrectedSim3.find(pKF);
        if (itn != NonCorrectedSim3.end()) rfe_detail::copy_sim3(itn->second, &s_meas[(size_t)k * 8]);
        else std::copy(e, e + 8, &s_meas[(size_t)k * 8]);
        fixed[k] = pKF->mnId == pMap->GetInitKFid();
    }
    struct EdgeRec { int i, j, from_est; };
    std::vector<EdgeRec> edges;
    std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
    // step 3, :4605-4645
    for (auto mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrameT* pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const int vi = vertex(pKF);
        for (auto sit = mit->second.begin(), send = mit->second.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const int vj = vertex(*sit);
            if (vi < 0 || vj < 0 || vi == vj) continue;
            edges.push_back(EdgeRec{vi, vj, 1});
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    // step 4, :4649-4780
    for (int k = 0; k < N; ++k) {
        KeyFrameT* pKF = kfs[k];
        KeyFrameT* pParentKF = pKF->GetParent();
        if (pParentKF) {
            const int vj = vertex(pParentKF);
            if (vj >= 0 && vj != k) edges.push_back(EdgeRec{k, vj, 0});
        }
        const auto sLoopEdges = pKF->GetLoopEdges();
        for (auto sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrameT* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) {
                const int vj = vertex(pLKF);
                if (vj >= 0) edges.push_back(EdgeRec{k, vj, 0});
            }
        }
        const std::vector<KeyFrameT*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (KeyFrameT* pKFn : vpConnectedKFs)
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn))
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    const int vj = vertex(pKFn);
                    if (vj >= 0) edges.push_back(EdgeRec{k, vj, 0});
                }
    }
    std::stable_sort(edges.begin(), edges.end(), [](const EdgeRec& a, const EdgeRec& b) { return a.i < b.i || (a.i == b.i && a.j < b.j); });
    const int E = (int)edges.size();
    // the points, :4806-4833
    std::vector<MapPointT*> mps;
    for (MapPointT* pMP : vpMPs)
        if (!pMP->isBad()) mps.push_back(pMP);
    if (E > RFE_EG_MAX_EDGES || mps.size() > (size_t)RFE_EG_MAX_POINTS) return RFE_EG_NOT_SERVED;
    const int L = (int)mps.size();
    std::vector<int32_t> edge_i(E), edge_j(E), point_ref(L);
    std::vector<uint8_t> edge_from_est(E);
    for (int e = 0; e < E; ++e) { edge_i[e] = edges[e].i; edge_j[e] = edges[e].j; edge_from_est[e] = (uint8_t)edges[e].from_est; }
    std::vector<float> xw((size_t)L * 3), xw_out((size_t)std::max(L, 1) * 3);
    for (int l = 0; l < L; ++l) {
        MapPointT* pMP = mps[l];
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const auto at = index.find(nIDr);
        point_ref[l] = at == index.end() ? -1 : at->second;
        rfe_detail::copy_vec3(pMP->GetWorldPos(), &xw[(size_t)l * 3]);
    }
    rfe_essential_graph_params prm = rfe_essential_graph_params();
    prm.iterations = 20; prm.max_trials = 10; prm.user_lambda_init = 1e-16; prm.fix_scale = bFixScale ? 1 : 0;
    std::vector<double> siw((size_t)N * 8);
    std::vector<float> tiw((size_t)N * 7);
    int32_t stats[8];
    const int rc = rfe_essential_graph(ctx, prm, s_est.data(), s_meas.data(), fixed.data(), edge_i.data(), edge_j.data(), edge_from_est.data(),
                                       xw.data(), point_ref.data(), N, E, L, siw.data(), tiw.data(), nullptr, xw_out.data(), nullptr, nullptr,
                                       stats);
    if (rc < 0) return rc;
    if (stats_out) for (int k = 0; k < 8; ++k) stats_out[k] = stats[k];
    // :4787-4836
    std::unique_lock<typename std::decay<decltype(pMap->mMutexMapUpdate)>::type> lock(pMap->mMutexMapUpdate);
    for (int k = 0; k < N; ++k) {
        const auto Tcw = kfs[k]->GetPose();
        using PoseT = typename std::decay<decltype(Tcw)>::type;
        using QuatT = typename std::decay<decltype(Tcw.unit_quaternion())>::type;
        using VecT = typename std::decay<decltype(Tcw.translation())>::type;
        const float* o = &tiw[(size_t)k * 7];
        kfs[k]->SetPose(PoseT(QuatT(o[3], o[0], o[1], o[2]), VecT(o[4], o[5], o[6])));
    }
    for (int l = 0; l < L; ++l) {
        using PosT = typename std::decay<decltype(mps[l]->GetWorldPos())>::type;
        const float* o = &xw_out[(size_t)l * 3];
        mps[l]->SetWorldPos(PosT(o[0], o[1], o[2]));
        mps[l]->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();
    return rc;
}

}  // namespace ORB_SLAM3
