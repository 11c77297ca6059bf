// rfe/stereo_match.h -- drop-in body for Frame::ComputeStereoMatches (reference src/Frame.cc:1159-1446,
// called from the stereo Frame constructor at src/Frame.cc:171) on top of rfe_stereo_match.
// Works on any Frame-like type with the reference's member names: N, mvKeys, mvKeysRight, mDescriptors,
// mDescriptorsRight, imgLeft, imgRight, mb, mbf, mvuRight, mvDepth.  nLevels must be 1: a frame holding a keypoint with octave != 0
// (RFE_SP_PYRAMID extraction) is refused with RFE_ERR_INVALID, every mvuRight / mvDepth -1.
// `ctx` can be the session of either extractor: mpSPextractorLeft->featureExtractor->ExtractorSession.
// Frames of an RFE_SP_PYRAMID extraction (nLevels > 1): ComputeStereoMatchesPyramid_rfe below.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "../rover_fe.h"
#include "cv_compat.h"

namespace ORB_SLAM3 {

template <class FrameT>
int ComputeStereoMatches_rfe(rfe_ctx* ctx, FrameT& F) {
    const int N = (int)F.mvKeys.size(), Nr = (int)F.mvKeysRight.size();
    F.mvuRight = std::vector<float>(N, -1.0f);
    F.mvDepth = std::vector<float>(N, -1.0f);
    if (N == 0) return 0;
    // nLevels == 1 geometry only: keypoints of a pyramid level (octave > 0) would need the level image at pt * mvInvScaleFactors[octave]
    // (src/Frame.cc:1305-1318) -- refused rather than matched as if they were level-0 pixels
    for (int i = 0; i < N; ++i) if (F.mvKeys[i].octave != 0) return RFE_ERR_INVALID;
    for (int i = 0; i < Nr; ++i) if (F.mvKeysRight[i].octave != 0) return RFE_ERR_INVALID;
    std::vector<float> kl((size_t)N * 2), kr((size_t)(Nr > 0 ? Nr : 1) * 2), dl((size_t)N * 256), dr((size_t)(Nr > 0 ? Nr : 1) * 256);
    for (int i = 0; i < N; ++i) {
        kl[2 * i] = F.mvKeys[i].pt.x; kl[2 * i + 1] = F.mvKeys[i].pt.y;
        const float* s = F.mDescriptors.template ptr<float>(i);
        std::copy(s, s + 256, dl.begin() + (size_t)i * 256);
    }
    for (int i = 0; i < Nr; ++i) {
        kr[2 * i] = F.mvKeysRight[i].pt.x; kr[2 * i + 1] = F.mvKeysRight[i].pt.y;
        const float* s = F.mDescriptorsRight.template ptr<float>(i);
        std::copy(s, s + 256, dr.begin() + (size_t)i * 256);
    }
    return rfe_stereo_match(ctx, F.imgLeft.template ptr<unsigned char>(0), F.imgRight.template ptr<unsigned char>(0), F.imgLeft.rows,
                            F.imgLeft.cols, (int)F.imgLeft.step, kl.data(), N, kr.data(), Nr, dl.data(), dr.data(), F.mb, F.mbf,
                            F.mvuRight.data(), F.mvDepth.data());
}

// Frame::ComputeStereoMatches for frames whose keypoints came from SPextractor built with -DRFE_SP_PYRAMID=1 (any nLevels >= 1), on
// top of rfe_stereo_match_pyramid: additionally reads mvKeys[i].octave and, from the two extractors, mvImagePyramid, GetLevels(),
// GetScaleFactor().  Level 0 is F.imgLeft / F.imgRight (the single-level extractor path leaves mvImagePyramid[0] empty); levels >= 1
// are packed from mvImagePyramid into the library's tight layout.  RFE_ERR_INVALID, every mvuRight / mvDepth -1, when the two
// extractors disagree on levels / scale factor or a level Mat's size differs from rfe_pyramid_geometry's.
// sad_source: RFE_STEREO_SAD_LEVEL (patches from the pyramid level) or RFE_STEREO_SAD_LEVEL0 (the reference as written).
template <class FrameT, class ExtractorT>
int ComputeStereoMatchesPyramid_rfe(rfe_ctx* ctx, FrameT& F, ExtractorT& left, ExtractorT& right, int sad_source = RFE_STEREO_SAD_LEVEL) {
    const int N = (int)F.mvKeys.size(), Nr = (int)F.mvKeysRight.size();
    F.mvuRight = std::vector<float>(N, -1.0f);
    F.mvDepth = std::vector<float>(N, -1.0f);
    const int L = left.GetLevels();
    const float sf = left.GetScaleFactor();
    if (L != right.GetLevels() || sf != right.GetScaleFactor() || L < 1 || L > RFE_MAX_LEVELS) return RFE_ERR_INVALID;
    const int H = F.imgLeft.rows, W = F.imgLeft.cols;
    if (F.imgRight.rows != H || F.imgRight.cols != W) return RFE_ERR_INVALID;
    int32_t lh[RFE_MAX_LEVELS], lw[RFE_MAX_LEVELS]; float ls[RFE_MAX_LEVELS];
    if (rfe_pyramid_geometry(H, W, L, sf, lh, lw, ls) != RFE_OK) return RFE_ERR_INVALID;
    if ((int)left.mvImagePyramid.size() < L || (int)right.mvImagePyramid.size() < L) return RFE_ERR_INVALID;
    size_t frame = 0;
    for (int l = 0; l < L; ++l) frame += (size_t)lh[l] * lw[l];
    std::vector<unsigned char> lv[2] = {std::vector<unsigned char>(frame), std::vector<unsigned char>(frame)};
    for (int v = 0; v < 2; ++v) {
        ExtractorT& e = v ? right : left;
        size_t off = 0;
        for (int l = 0; l < L; ++l) {
            const bool own = l > 0 || !e.mvImagePyramid[0].empty();
            if (own && (e.mvImagePyramid[l].rows != lh[l] || e.mvImagePyramid[l].cols != lw[l])) return RFE_ERR_INVALID;
            const auto& m = own ? e.mvImagePyramid[l] : (v ? F.imgRight : F.imgLeft);
            for (int r = 0; r < lh[l]; ++r) std::memcpy(lv[v].data() + off + (size_t)r * lw[l], m.template ptr<unsigned char>(r), (size_t)lw[l]);
            off += (size_t)lh[l] * lw[l];
        }
    }
    if (N == 0) return 0;
    std::vector<float> kl((size_t)N * 2), kr((size_t)(Nr > 0 ? Nr : 1) * 2), dl((size_t)N * 256), dr((size_t)(Nr > 0 ? Nr : 1) * 256);
    std::vector<int32_t> ol((size_t)N), orr((size_t)(Nr > 0 ? Nr : 1));
    for (int i = 0; i < N; ++i) {
        kl[2 * i] = F.mvKeys[i].pt.x; kl[2 * i + 1] = F.mvKeys[i].pt.y; ol[i] = F.mvKeys[i].octave;
        const float* s = F.mDescriptors.template ptr<float>(i);
        std::copy(s, s + 256, dl.begin() + (size_t)i * 256);
    }
    for (int i = 0; i < Nr; ++i) {
        kr[2 * i] = F.mvKeysRight[i].pt.x; kr[2 * i + 1] = F.mvKeysRight[i].pt.y; orr[i] = F.mvKeysRight[i].octave;
        const float* s = F.mDescriptorsRight.template ptr<float>(i);
        std::copy(s, s + 256, dr.begin() + (size_t)i * 256);
    }
    const int rc = rfe_stereo_match_pyramid(ctx, lv[0].data(), lv[1].data(), H, W, L, sf, kl.data(), ol.data(), N, kr.data(), orr.data(), Nr,
                                            dl.data(), dr.data(), F.mb, F.mbf, sad_source, F.mvuRight.data(), F.mvDepth.data());
    if (rc != RFE_OK) { std::fill(F.mvuRight.begin(), F.mvuRight.end(), -1.0f); std::fill(F.mvDepth.begin(), F.mvDepth.end(), -1.0f); }
    return rc;
}

}  // namespace ORB_SLAM3
