// rfe/pose_inertial_optimization.h -- drop-ins for Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool) and
// Optimizer::PoseInertialOptimizationLastFrame(Frame*, bool) (reference src/Optimizer.cc:416-968, :983-1623) on top of
// rfe_pose_inertial_optimization: the four rounds of Gauss-Newton, the chi2 classification between them, the recovery pass,
// the final Hessian, its marginalisation and ConstraintPoseImu's clipping run in one kernel; what comes back is mvbOutlier, the values for
// SetImuPoseVelocity and mImuBias, and the constraint the next frame's call takes as its prior.
// Works on any Frame-like class with the reference's member names:
//   N, mvKeysUn, mvuRight, mvpMapPoints (entries with GetWorldPos() indexable with (i), and mTrackDepth), mvInvLevelSigma2, fx, fy, cx, cy, mbf,
//   mpCamera2, mvbOutlier, GetPose() (rotationMatrix() indexable with (r, c), translation() with (i)), GetImuRotation(), GetImuPosition(),
//   GetVelocity(), mImuBias (bax bay baz bwx bwy bwz, constructible from those six), mImuCalib.mTcb / mTbc (as GetPose()),
//   SetImuPoseVelocity(Rwb, twb, v) taking what GetImuRotation() / GetImuPosition() / GetVelocity() return (writable with (r, c) / (i), as
//   Eigen's are), mpImuPreintegrated / mpImuPreintegratedFrame (dT, dR, dV, dP, JRg, JVg, JVa, JPg, JPa, b, C), and
//   mpLastKeyFrame (GetImuRotation(), GetImuPosition(), GetVelocity(), GetGyroBias(), GetAccBias()) or mpPrevFrame (a Frame).
// The prior travels as a plain PoseImuConstraint_rfe, in rfe_pose_inertial_optimization's prior layout.  The integrator adds
//   PoseImuConstraint_rfe* mpcpi_rfe = nullptr;   (owned: deleted with the frame)
// to Frame, next to the reference's mpcpi.  Both drop-ins set the current frame's; the LastFrame one reads the previous frame's and frees
// it where the reference deletes pFp->mpcpi (:1618).  ToConstraintPoseImu<ConstraintPoseImu>(c) builds the reference's object for a caller
// that falls back to the reference's function on a later frame; that constructor symmetrises and clips a second time, which changes the
// already clipped H by rounding only.
// Both return the reference's value, nInitialCorrespondences - nBad; -1 and nothing touched for a frame with a second camera (mpCamera2)
// and, in LastFrame mode, for a previous frame without mpcpi_rfe (the reference dereferences a NULL there) -- such a caller keeps the
// reference's function.  -1 means that and nothing else: when the library refuses or fails, the drop-ins return RFE_PIO_DROPIN_ERROR +
// rfe_status (-101 for RFE_ERR_INVALID: N > 4096, no or too many levels, a dT that is not positive), and nothing has been touched either.
// A caller whose frame is resident on the device calls rfe_pose_inertial_optimization_dev itself, behind rfe_search_local_points_dev, and
// hands prior_out_dev / state_f32_dev of frame k to frame k + 1 as prior_in_dev / prev_state_dev.
#pragma once
#include <cstdint>
#include <type_traits>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

enum { RFE_PIO_DROPIN_ERROR = -100 };          // a library status s < 0 comes back as RFE_PIO_DROPIN_ERROR + s, so that -1 stays "not served"

struct PoseImuConstraint_rfe {                 // RFE_PIO_PRIOR_DOUBLES doubles, row-major
    double Rwb[9], twb[3], vwb[3], bg[3], ba[3], H[225];
};
static_assert(sizeof(PoseImuConstraint_rfe) == RFE_PIO_PRIOR_DOUBLES * sizeof(double), "PoseImuConstraint_rfe is the prior layout");

// the reference's ConstraintPoseImu (or any class with its six public members and its constructor) from a stored constraint
template <class ConstraintT>
ConstraintT* ToConstraintPoseImu(const PoseImuConstraint_rfe& c) {
    typename std::decay<decltype(ConstraintT::Rwb)>::type R;
    typename std::decay<decltype(ConstraintT::twb)>::type t, v, bg, ba;
    typename std::decay<decltype(ConstraintT::H)>::type H;
    for (int k = 0; k < 9; ++k) R(k / 3, k % 3) = c.Rwb[k];
    for (int k = 0; k < 3; ++k) { t(k) = c.twb[k]; v(k) = c.vwb[k]; bg(k) = c.bg[k]; ba(k) = c.ba[k]; }
    for (int k = 0; k < 225; ++k) H(k / 15, k % 15) = c.H[k];
    return new ConstraintT(R, t, v, bg, ba, H);
}

namespace rfe_detail {

template <class PoseT> inline void copy_se3(const PoseT& T, float* dst) { copy_rotation(T.rotationMatrix(), dst); copy_vec3(T.translation(), dst + 9); }
// Rwb 9, twb 3, velocity 3 of a Frame or KeyFrame
template <class BodyT> inline void copy_body(BodyT* p, float* dst) {
    copy_rotation(p->GetImuRotation(), dst); copy_vec3(p->GetImuPosition(), dst + 9); copy_vec3(p->GetVelocity(), dst + 12);
}
template <class BiasT> inline void copy_bias(const BiasT& b, float* bg, float* ba) {
    bg[0] = b.bwx; bg[1] = b.bwy; bg[2] = b.bwz; ba[0] = b.bax; ba[1] = b.bay; ba[2] = b.baz;
}
// IMU::Preintegrated -> preint [RFE_PIO_PREINT_FLOATS]
template <class PreintT> inline void copy_preintegration(PreintT* p, float* dst) {
    dst[0] = p->dT;
    copy_rotation(p->dR, dst + 1); copy_vec3(p->dV, dst + 10); copy_vec3(p->dP, dst + 13);
    copy_rotation(p->JRg, dst + 16); copy_rotation(p->JVg, dst + 25); copy_rotation(p->JVa, dst + 34); copy_rotation(p->JPg, dst + 43);
    copy_rotation(p->JPa, dst + 52);
    copy_bias(p->b, dst + 64, dst + 61);
    for (int k = 0; k < 81; ++k) dst[67 + k] = p->C(k / 9, k % 9);
}

// what the two entries share behind their gathers of the previous state
template <class FrameT, class PreintT>
int pose_inertial(rfe_ctx* ctx, FrameT* pFrame, int32_t mode, bool bRecInit, const float* prev_state, PreintT* edge_preint, const double* prior_in,
                  int32_t* stats_out) {
    const int N = pFrame->N;
    const size_t n = (size_t)(N > 0 ? N : 0);
    if (N < 0 || N > 4096 || pFrame->mvInvLevelSigma2.empty() || pFrame->mvInvLevelSigma2.size() > RFE_MAX_LEVELS) return RFE_PIO_DROPIN_ERROR + RFE_ERR_INVALID;
    rfe_pose_inertial_params P = rfe_pose_inertial_params();
    P.fx = pFrame->fx; P.fy = pFrame->fy; P.cx = pFrame->cx; P.cy = pFrame->cy; P.bf = pFrame->mbf;
    P.nlevels = (int32_t)pFrame->mvInvLevelSigma2.size();
    copy_levels(pFrame->mvInvLevelSigma2, P.nlevels, P.inv_level_sigma2);
    float cam[RFE_PIO_CAM_FLOATS], state[RFE_PIO_STATE_FLOATS], preint[RFE_PIO_PREINT_FLOATS], cov_rw[RFE_PIO_COV_RW_FLOATS];
    copy_se3(pFrame->GetPose(), cam); copy_se3(pFrame->mImuCalib.mTcb, cam + 12); copy_se3(pFrame->mImuCalib.mTbc, cam + 24);
    copy_body(pFrame, state);
    copy_bias(pFrame->mImuBias, state + 15, state + 18);
    copy_preintegration(edge_preint, preint);
    for (int k = 0; k < 9; ++k) {                                   // InfoG / InfoA read mpImuPreintegrated in both modes (:669, :1233)
        cov_rw[k] = pFrame->mpImuPreintegrated->C(9 + k / 3, 9 + k % 3);
        cov_rw[9 + k] = pFrame->mpImuPreintegrated->C(12 + k / 3, 12 + k % 3);
    }
    std::vector<float> kpts(n * 2), uright(n), xw(n * 3, 0.f), depth(n, 0.f);
    std::vector<int32_t> octave(n);
    std::vector<uint8_t> has_mp(n), outlier(n);
    gather_keypoints(pFrame->mvKeysUn, n, kpts.data(), octave.data());
    for (size_t i = 0; i < n; ++i) {
        uright[i] = pFrame->mvuRight[i];
        outlier[i] = pFrame->mvbOutlier[i] ? 1 : 0;
        if (pFrame->mvpMapPoints[i]) {
            has_mp[i] = 1;
            copy_vec3(pFrame->mvpMapPoints[i]->GetWorldPos(), &xw[3 * i]);
            depth[i] = pFrame->mvpMapPoints[i]->mTrackDepth;
        }
    }
    const int32_t rec = bRecInit ? 1 : 0;
    double state_out[RFE_PIO_STATE_FLOATS]; float sf[RFE_PIO_STATE_FLOATS]; int32_t stats[16];
    PoseImuConstraint_rfe* out = new PoseImuConstraint_rfe();
    const int rc = rfe_pose_inertial_optimization(ctx, &P, &mode, &rec, cam, state, prev_state, preint, cov_rw, prior_in, kpts.data(), octave.data(),
                                                  uright.data(), xw.data(), has_mp.data(), depth.data(), nullptr, 1, N, state_out, sf, outlier.data(),
                                                  nullptr, reinterpret_cast<double*>(out), nullptr, stats);
    if (rc < 0) { delete out; return RFE_PIO_DROPIN_ERROR + rc; }
    if (stats_out) for (int k = 0; k < 16; ++k) stats_out[k] = stats[k];
    for (size_t i = 0; i < n; ++i) if (has_mp[i]) pFrame->mvbOutlier[i] = outlier[i] != 0;
    typename std::decay<decltype(pFrame->GetImuRotation())>::type R = pFrame->GetImuRotation();
    typename std::decay<decltype(pFrame->GetImuPosition())>::type t = pFrame->GetImuPosition();
    typename std::decay<decltype(pFrame->GetVelocity())>::type v = pFrame->GetVelocity();
    for (int k = 0; k < 9; ++k) R(k / 3, k % 3) = sf[k];
    for (int k = 0; k < 3; ++k) { t(k) = sf[9 + k]; v(k) = sf[12 + k]; }
    pFrame->SetImuPoseVelocity(R, t, v);
    using BiasT = typename std::decay<decltype(pFrame->mImuBias)>::type;
    pFrame->mImuBias = BiasT(sf[18], sf[19], sf[20], sf[15], sf[16], sf[17]);
    delete pFrame->mpcpi_rfe;
    pFrame->mpcpi_rfe = out;
    return stats[0];
}

}  // namespace rfe_detail

template <class FrameT>
int PoseInertialOptimizationLastKeyFrame_rfe(rfe_ctx* ctx, FrameT* pFrame, bool bRecInit = false,
                                             int32_t* stats_out = nullptr /*[16], as rfe_pose_inertial_optimization*/) {
    if (pFrame->mpCamera2) return -1;
    auto* pKF = pFrame->mpLastKeyFrame;
    float prev[RFE_PIO_STATE_FLOATS];
    rfe_detail::copy_body(pKF, prev);
    rfe_detail::copy_vec3(pKF->GetGyroBias(), prev + 15); rfe_detail::copy_vec3(pKF->GetAccBias(), prev + 18);
    return rfe_detail::pose_inertial(ctx, pFrame, (int32_t)RFE_PIO_LAST_KEYFRAME, bRecInit, prev, pFrame->mpImuPreintegrated, nullptr, stats_out);
}

template <class FrameT>
int PoseInertialOptimizationLastFrame_rfe(rfe_ctx* ctx, FrameT* pFrame, bool bRecInit = false,
                                          int32_t* stats_out = nullptr /*[16], as rfe_pose_inertial_optimization*/) {
    if (pFrame->mpCamera2) return -1;
    auto* pFp = pFrame->mpPrevFrame;
    if (!pFp->mpcpi_rfe) return -1;
    float prev[RFE_PIO_STATE_FLOATS];
    rfe_detail::copy_body(pFp, prev);
    rfe_detail::copy_bias(pFp->mImuBias, prev + 15, prev + 18);
    const int rc = rfe_detail::pose_inertial(ctx, pFrame, (int32_t)RFE_PIO_LAST_FRAME, bRecInit, prev, pFrame->mpImuPreintegratedFrame,
                                             reinterpret_cast<const double*>(pFp->mpcpi_rfe), stats_out);
    if (rc < 0) return rc;
    delete pFp->mpcpi_rfe;
    pFp->mpcpi_rfe = nullptr;
    return rc;
}

}  // namespace ORB_SLAM3
