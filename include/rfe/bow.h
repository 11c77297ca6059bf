// rfe/bow.h -- drop-in bodies for the place-recognition side of the reference:
//   ComputeBoW3_rfe     Frame::ComputeBoW3 / KeyFrame::ComputeBoW3 (src/Frame.cc:1044-1054, src/KeyFrame.cc:123-...): binarize_descriptors +
//                       mpSPvocabulary->transform(vCurrentDesc, mBow3Vec, mFeat3Vec, 0), on rfe_bow_transform
//   AddKeyFrame_rfe     KeyFrameDatabase::add: the keyframe's BoW vector into an rfe_bow_db; the entry id is what the caller keeps per keyframe
//   ScoreKeyFrames_rfe  the front of KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:660-740,
//                       :1045-1100): common-word counts, the 0.8 max gate and mpVoc->score, on rfe_bow_db_query.  The list comes back in
//                       entry order (the reference's list follows its inverted file: first shared word, then insertion); the covisibility
//                       accumulation behind it stays the caller's.
// The two map types are template parameters: DBoW3::BowVector / DBoW3::FeatureVector and plain std::map<unsigned, double> /
// std::map<unsigned, std::vector<unsigned>> both work.  mDescriptors is the frame's N x 256 CV_32F descriptor matrix (binarised by the call,
// as Frame::binarize_descriptors does) or an N x D CV_8U one taken as it is.  More than 4096 features are refused (RFE_ERR_INVALID): such a
// caller keeps the reference's transform.
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "../rover_fe.h"
#include "cv_compat.h"

namespace ORB_SLAM3 {

// returns the number of words (>= 0) or an rfe_status (< 0; rfe_last_error(ctx)); the maps are cleared first, as transform() clears them
template <class BowVecT, class FeatVecT>
inline int ComputeBoW3_rfe(rfe_ctx* ctx, const rfe_bow_vocab* vocab, const cv::Mat& mDescriptors, BowVecT& bow, FeatVecT& fv, int levelsup = 0) {
    bow.clear();
    fv.clear();
    const int N = mDescriptors.rows;
    if (N <= 0) return 0;
    const bool f32 = mDescriptors.type() == CV_32F;
    if (!f32 && mDescriptors.type() != CV_8U) return RFE_ERR_INVALID;
    const size_t row = (size_t)mDescriptors.cols * (f32 ? 4 : 1);
    std::vector<unsigned char> packed;                  // a matrix whose rows are not back to back is copied once
    const unsigned char* data = mDescriptors.template ptr<unsigned char>(0);
    if (!mDescriptors.isContinuous()) {
        packed.resize(row * (size_t)N);
        for (int r = 0; r < N; ++r) std::memcpy(packed.data() + row * (size_t)r, mDescriptors.template ptr<unsigned char>(r), row);
        data = packed.data();
    }
    if (f32 && mDescriptors.cols != RFE_DESC_DIM) return RFE_ERR_INVALID;
    std::vector<int32_t> bow_word((size_t)N), fv_node((size_t)N), fv_offsets((size_t)N + 1), fv_feat((size_t)N);
    std::vector<double> bow_value((size_t)N);
    int32_t bow_n = 0, fv_n = 0;
    const int rc = rfe_bow_transform(ctx, vocab, f32 ? (const float*)data : nullptr, f32 ? nullptr : data, N, levelsup, nullptr, nullptr, nullptr,
                                     &bow_n, bow_word.data(), bow_value.data(), &fv_n, fv_node.data(), fv_offsets.data(), fv_feat.data());
    if (rc < 0) return rc;
    for (int i = 0; i < bow_n; ++i)
        bow.insert(bow.end(), typename BowVecT::value_type((typename BowVecT::key_type)bow_word[i], (typename BowVecT::mapped_type)bow_value[i]));
    for (int i = 0; i < fv_n; ++i) {
        typename FeatVecT::mapped_type& list = fv[(typename FeatVecT::key_type)fv_node[i]];
        list.reserve((size_t)(fv_offsets[i + 1] - fv_offsets[i]));
        for (int j = fv_offsets[i]; j < fv_offsets[i + 1]; ++j) list.push_back((typename FeatVecT::mapped_type::value_type)fv_feat[j]);
    }
    return bow_n;
}

namespace rfe_bow_detail {
template <class BowVecT>
inline void flatten(const BowVecT& bow, std::vector<int32_t>& word, std::vector<double>& value) {
    word.clear(); value.clear();
    word.reserve(bow.size()); value.reserve(bow.size());
    for (typename BowVecT::const_iterator it = bow.begin(); it != bow.end(); ++it) { word.push_back((int32_t)it->first); value.push_back((double)it->second); }
}
}  // namespace rfe_bow_detail

// returns RFE_OK or an rfe_status; *entry_id is the id the database's per-entry arrays are indexed with
template <class BowVecT>
inline int AddKeyFrame_rfe(rfe_bow_db* db, const BowVecT& bow, int32_t* entry_id) {
    std::vector<int32_t> word; std::vector<double> value;
    rfe_bow_detail::flatten(bow, word, value);
    return rfe_bow_db_add(db, word.data(), value.data(), (int)word.size(), entry_id);
}

struct ScoreKeyFramesStats_rfe { int maxCommonWords = 0, minCommonWords = 0, nSharing = 0, nScored = 0; };

// exclude: one byte per entry id (the connected keyframes of DetectNBestCandidates, the other maps' keyframes of
// DetectRelocalizationCandidates), or empty.  lScoreAndMatch: (entry id, (float)score) of every entry that shares more than minCommonWords
// words with bow, ascending entry ids.  Returns their number or an rfe_status (< 0).
template <class BowVecT>
inline int ScoreKeyFrames_rfe(rfe_bow_db* db, const BowVecT& bow, const std::vector<uint8_t>& exclude,
                              std::vector<std::pair<int32_t, float> >& lScoreAndMatch, ScoreKeyFramesStats_rfe* stats_out = nullptr) {
    lScoreAndMatch.clear();
    const int E = rfe_bow_db_size(db);
    if (E < 0) return E;
    if (!exclude.empty() && (int)exclude.size() != E) return RFE_ERR_INVALID;
    std::vector<int32_t> word; std::vector<double> value;
    rfe_bow_detail::flatten(bow, word, value);
    std::vector<int32_t> common((size_t)E + 1);
    std::vector<uint8_t> scored((size_t)E + 1);
    std::vector<double> score((size_t)E + 1);
    int32_t stats[4] = {0, 0, 0, 0};
    const int rc = rfe_bow_db_query(db, word.data(), value.data(), (int)word.size(), exclude.empty() ? nullptr : exclude.data(), common.data(),
                                    scored.data(), score.data(), stats);
    if (rc < 0) return rc;
    for (int e = 0; e < E; ++e)
        if (scored[e]) lScoreAndMatch.push_back(std::make_pair((int32_t)e, (float)score[e]));   // float si = mpVoc->score(...)
    if (stats_out) { stats_out->maxCommonWords = stats[0]; stats_out->minCommonWords = stats[1]; stats_out->nSharing = stats[2]; stats_out->nScored = stats[3]; }
    return (int)lScoreAndMatch.size();
}

}  // namespace ORB_SLAM3
