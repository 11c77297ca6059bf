// rfe/two_view_reconstruction.h -- drop-in for TwoViewReconstruction (reference src/TwoViewReconstruction.cc, include/TwoViewReconstruction.h)
// on top of rfe_two_view: Reconstruct() packs vMatches12 into the match list, draws the 8 x iterations random numbers the
// reference draws, and makes ONE device call for both models, their 200 hypotheses each, the decomposition and every CheckRT pass.
// Works on any KeyPoint-like type with `.pt.x`, `.pt.y` and any Point3f-like type constructible from (x, y, z).
// R21 and t21 come back as row-major std::array (Sophus::SE3f(Eigen::Map<const Eigen::Matrix<float, 3, 3, Eigen::RowMajor>>(R.data()),
// Eigen::Map<const Eigen::Vector3f>(t.data())) in Rover-SLAM).
// The random numbers come from the functor handed to the constructor -- in Rover-SLAM `[]{ DUtils::Random::SeedRandOnce(0); return rand(); }`
// -- called exactly 8 x iterations times per Reconstruct(), as DUtils::Random::RandomInt calls rand(): the caller's stream stands where the
// reference's would.
// Stated differences:
//   * vP3D is assigned on the homography branch too; the reference forgets `vP3D = bestP3D` there (:932-938) and leaves the caller's
//     stale vector.  model() tells which branch ran (0 none, 1 H, 2 F);
//   * vP3D and vbTriangulated are sized vKeys1.size() and zero / false when Reconstruct() answers false (the reference leaves them alone);
//   * fewer than 8 matches answer false (the reference indexes an empty vector);
//   * more than 4096 keypoints in a frame or more than 1024 iterations are not served: status() is -1, nothing is drawn and nothing is
//     touched (keep the reference's class).
#pragma once
#include <array>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

static_assert(RAND_MAX == 2147483647, "rfe_two_view resolves a draw as (int)(((double)r / 2147483648.0) * size): rand() must span 31 bits");

class TwoViewReconstruction_rfe {
public:
    typedef std::array<float, 9> Mat3;
    typedef std::array<float, 3> Vec3;

    TwoViewReconstruction_rfe(rfe_ctx* ctx, std::function<int()> rand31, float fx, float fy, float cx, float cy, float sigma = 1.0, int iterations = 200)
        : ctx_(ctx), rand_(rand31), its_(iterations) {
        P_.fx = fx; P_.fy = fy; P_.cx = cx; P_.cy = cy; P_.sigma = sigma;
    }
    // 0 = the reference's 0.50 (ORB-SLAM2 used 0.40)
    void SetHomographyRatio(float rh_threshold) { P_.rh_threshold = rh_threshold; }

    template <class KeysT, class Point3T>
    bool Reconstruct(const KeysT& vKeys1, const KeysT& vKeys2, const std::vector<int>& vMatches12, Mat3& R21, Vec3& t21, std::vector<Point3T>& vP3D,
                     std::vector<bool>& vbTriangulated) {
        const size_t n1 = vKeys1.size(), n2 = vKeys2.size();
        for (int k = 0; k < 16; ++k) stats_[k] = 0;
        if (n1 > 4096 || n2 > 4096 || its_ < 1 || its_ > 1024) { status_ = -1; return false; }
        status_ = 0;
        std::vector<float> k1(2 * n1 + 2), k2(2 * n2 + 2);
        rfe_detail::gather_keypoints(vKeys1, n1, k1.data());
        rfe_detail::gather_keypoints(vKeys2, n2, k2.data());
        std::vector<int32_t> pairs;                                     // mvMatches12 (:64-77)
        pairs.reserve(2 * n1 + 2);
        for (size_t i = 0, iend = vMatches12.size(); i < iend && i < n1; i++)
            if (vMatches12[i] >= 0) { pairs.push_back((int32_t)i); pairs.push_back(vMatches12[i]); }
        const int32_t S = (int32_t)(pairs.size() / 2);
        pairs.resize(pairs.size() + 2);
        std::vector<int32_t> draws((size_t)its_ * 8);
        for (size_t k = 0; k < draws.size(); ++k) draws[k] = rand_();    // :99-115: 8 per iteration, whatever comes of them
        P_.its = its_; P_.n1 = (int32_t)n1; P_.n2 = (int32_t)n2;
        std::vector<float> p3d(3 * n1 + 3);
        std::vector<uint8_t> tri(n1 + 1);
        Mat3 R; Vec3 t;
        const int rc = rfe_two_view(ctx_, &P_, k1.data(), k2.data(), &S, pairs.data(), draws.data(), 1, (int)n1, (int)n2, S, its_, R.data(), t.data(),
                                    p3d.data(), tri.data(), nullptr, nullptr, nullptr, nullptr, nullptr, stats_);
        if (rc < 0) { status_ = rc; return false; }
        vP3D.assign(n1, Point3T(0.f, 0.f, 0.f));
        vbTriangulated.assign(n1, false);
        for (size_t i = 0; i < n1; ++i) {
            vP3D[i] = Point3T(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
            vbTriangulated[i] = tri[i] != 0;
        }
        if (rc == 1) { R21 = R; t21 = t; }
        return rc == 1;
    }

    int status() const { return status_; }                           // 0; -1 not served; another negative rfe_status: refused or failed
    int model() const { return stats_[1]; }                          // 0 none, 1 the homography branch, 2 the fundamental-matrix branch
    const int32_t* stats() const { return stats_; }                  // rfe_two_view's

private:
    rfe_ctx* ctx_;
    std::function<int()> rand_;
    rfe_two_view_params P_ = rfe_two_view_params();
    int its_, status_ = 0;
    int32_t stats_[16] = {0};
};

}  // namespace ORB_SLAM3
