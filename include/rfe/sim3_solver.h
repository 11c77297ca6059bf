// rfe/sim3_solver.h -- drop-in for Sim3Solver (reference src/Sim3Solver.cc, include/Sim3Solver.h) on top of rfe_sim3_ransac:
// every RANSAC hypothesis of the candidate is evaluated in ONE device call, made by the first iterate() / find(); every iterate(n, ..) then
// replays the reference's chunk semantics (mnIterations, mnBestInliers carried across chunks, bNoMore, bConverge, vbInliers scattered
// through mvnIndices1, the returned matrix) from the per-hypothesis counts and transforms on the host.
// Works on any KeyFrame / MapPoint-like classes with the reference's member names:
//   KeyFrame: GetMapPointMatches(), GetRotation() (indexable with (r, c)), GetTranslation() (with (i)), mvKeysUn, mvLevelSigma2, fx, fy, cx,
//             cy, mpCamera->GetType();  MapPoint: isBad(), GetIndexInKeyFrame(pKF) (std::get<0> is the index), GetWorldPos() (with (i)).
// Matrices come back as row-major std::array (Eigen::Map<const Eigen::Matrix<float, 4, 4, Eigen::RowMajor>>(T.data()) in Rover-SLAM).
// The random numbers come from the functor handed to the constructor -- DUtils::Random::RandomInt in Rover-SLAM -- called as
// randomInt(0, size - 1) three times per iteration, for ALL mRansacMaxIts iterations up front: after an early convergence the caller's
// stream is further along than the reference's (departure (d)).
// Stated differences:
//   * the five-argument overload returns an uninitialised bestSim3 in the reference when a chunk improves nothing (:242, :301): here it
//     returns the best transform so far (the identity before any hypothesis);
//   * iterate() after a convergence: the reference goes on drawing; here nothing is left to run, so it answers bNoMore with the best so far;
//   * fewer than three correspondences that still satisfy N >= mRansacMinInliers: the reference draws from an empty list; here bNoMore;
//   * a KannalaBrandt8 camera on either keyframe, more than 4096 correspondences or more than 1024 iterations are refused: status() is -1
//     (keep the reference's class) and every iterate() answers bNoMore with the identity.
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <tuple>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

template <class KeyFrameT, class MapPointT>
class Sim3Solver_rfe {
public:
    typedef std::array<float, 16> Mat4;
    typedef std::array<float, 9> Mat3;
    typedef std::array<float, 3> Vec3;

    Sim3Solver_rfe(rfe_ctx* ctx, std::function<int(int, int)> randomInt, KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12,
                   const bool bFixScale = true, std::vector<KeyFrameT*> vpKeyFrameMatchedMP = std::vector<KeyFrameT*>())
        : ctx_(ctx), rand_(randomInt) {
        bool bDifferentKFs = false;                                    // :40-45, as written
        if (vpKeyFrameMatchedMP.empty()) {
            bDifferentKFs = true;
            vpKeyFrameMatchedMP = std::vector<KeyFrameT*>(vpMatched12.size(), pKF2);
        }
        if (pKF1->mpCamera->GetType() != 0 || pKF2->mpCamera->GetType() != 0 /*GeometricCamera::CAM_PINHOLE*/) status_ = -1;
        const std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        rfe_detail::copy_rotation(pKF1->GetRotation(), P_.rcw1); rfe_detail::copy_vec3(pKF1->GetTranslation(), P_.tcw1);
        rfe_detail::copy_rotation(pKF2->GetRotation(), P_.rcw2); rfe_detail::copy_vec3(pKF2->GetTranslation(), P_.tcw2);
        P_.fx1 = pKF1->fx; P_.fy1 = pKF1->fy; P_.cx1 = pKF1->cx; P_.cy1 = pKF1->cy;
        P_.fx2 = pKF2->fx; P_.fy2 = pKF2->fy; P_.cx2 = pKF2->cx; P_.cy2 = pKF2->cy;
        P_.fix_scale = bFixScale ? 1 : 0;
        KeyFrameT* pKFm = pKF2;
        for (int i1 = 0; i1 < mN1; i1++) {                            // :71-118
            if (!vpMatched12[i1]) continue;
            MapPointT* pMP1 = vpKeyFrameMP1[i1];
            MapPointT* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
            const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
            const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            sigma2_1_.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]);
            sigma2_2_.push_back(pKFm->mvLevelSigma2[pKFm->mvKeysUn[indexKF2].octave]);
            mvnIndices1.push_back((size_t)i1);
            const auto X1 = pMP1->GetWorldPos(); const auto X2 = pMP2->GetWorldPos();
            for (int k = 0; k < 3; ++k) { xw1_.push_back(X1(k)); xw2_.push_back(X2(k)); }
        }
        best_.fill(0.f); best_[0] = best_[5] = best_[10] = best_[15] = 1.f;
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        N = (int)mvnIndices1.size();
        mRansacMinInliers = minInliers;
        mRansacMaxIts = rfe_sim3_ransac_iterations(probability, minInliers, N, maxIterations);
        mnIterations = 0;
        ran_ = ok_ = converged_ = false;                               // the next iterate() draws and evaluates under these parameters
    }

    // the five-argument overload (:221-302)
    Mat4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
        bNoMore = false; bConverge = false;
        vbInliers = std::vector<bool>(mN1 > 0 ? mN1 : 0, false);
        nInliers = 0;
        if (N < mRansacMinInliers || status_ < 0 || !run()) { bNoMore = true; return identity(); }
        if (converged_) { bNoMore = true; return best_; }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int h = mnIterations++;
            if (counts_[h] >= mnBestInliers) {
                mnBestInliers = counts_[h];
                best_h_ = h;
                for (int k = 0; k < 16; ++k) best_[k] = hyps_[(size_t)h * 32 + k];
                if (counts_[h] > mRansacMinInliers) {
                    nInliers = counts_[h];
                    for (int i = 0; i < N; i++) if (inliers_[i]) vbInliers[mvnIndices1[i]] = true;
                    bConverge = true; converged_ = true;
                    return best_;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return best_;
    }
    // the four-argument overload (:152-219): the identity unless the chunk converged
    Mat4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bool bConverge = false;
        const Mat4 T = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
        return bConverge ? T : identity();
    }
    Mat4 find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    Mat4 GetEstimatedTransformation() const { return best_; }
    Mat3 GetEstimatedRotation() const { Mat3 R; for (int k = 0; k < 9; ++k) R[k] = best_h_ < 0 ? (k % 4 == 0 ? 1.f : 0.f) : hyps_[(size_t)best_h_ * 32 + 16 + k]; return R; }
    Vec3 GetEstimatedTranslation() const { Vec3 t; for (int k = 0; k < 3; ++k) t[k] = best_h_ < 0 ? 0.f : hyps_[(size_t)best_h_ * 32 + 25 + k]; return t; }
    float GetEstimatedScale() const { return best_h_ < 0 ? 1.f : hyps_[(size_t)best_h_ * 32 + 28]; }

    int status() const { return status_; }                           // 0; -1 not served; another negative rfe_status: refused or failed
    const int32_t* stats() const { return stats_; }                  // rfe_sim3_ransac's, once the device call has been made
    int correspondences() const { return N; }
    int iterations() const { return mRansacMaxIts; }

private:
    static Mat4 identity() { Mat4 I; I.fill(0.f); I[0] = I[5] = I[10] = I[15] = 1.f; return I; }
    // the one device call; false: nothing can run (fewer than three correspondences, or the library refused)
    bool run() {
        if (ran_) return ok_;
        ran_ = true;
        if (N < 3) return ok_ = false;
        if (N > 4096 || mRansacMaxIts > 1024) { status_ = -1; return ok_ = false; }
        const int H = mRansacMaxIts;
        std::vector<int32_t> draws((size_t)H * 3);
        for (int h = 0; h < H; ++h)
            for (int k = 0; k < 3; ++k) draws[(size_t)h * 3 + k] = rand_(0, N - 1 - k);
        P_.min_inliers = mRansacMinInliers; P_.its = H; P_.n = N;
        counts_.assign(H, 0); hyps_.assign((size_t)H * 32, 0.f); inliers_.assign(N, 0);
        float T12[16];
        const int rc = rfe_sim3_ransac(ctx_, &P_, xw1_.data(), xw2_.data(), sigma2_1_.data(), sigma2_2_.data(), draws.data(), 1, N, H, T12, nullptr,
                                       nullptr, nullptr, inliers_.data(), nullptr, counts_.data(), hyps_.data(), stats_);
        if (rc < 0) { status_ = rc; return ok_ = false; }
        return ok_ = true;
    }

    rfe_ctx* ctx_;
    std::function<int(int, int)> rand_;
    rfe_sim3_solver_params P_ = rfe_sim3_solver_params();
    std::vector<float> xw1_, xw2_, sigma2_1_, sigma2_2_, hyps_;
    std::vector<int32_t> counts_;
    std::vector<uint8_t> inliers_;
    std::vector<size_t> mvnIndices1;
    int32_t stats_[8] = {0, 0, 0, -1, 0, 0, 0, 0};
    int N = 0, mN1 = 0, mnIterations = 0, mnBestInliers = 0, mRansacMinInliers = 6, mRansacMaxIts = 300, best_h_ = -1, status_ = 0;
    bool ran_ = false, ok_ = false, converged_ = false;
    Mat4 best_;
};

}  // namespace ORB_SLAM3
