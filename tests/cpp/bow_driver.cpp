// bow_driver.cpp -- test driver for include/rfe/bow.h (tests/test_gpu_bow_dropin.py): ComputeBoW3_rfe, AddKeyFrame_rfe and ScoreKeyFrames_rfe
// over mock DBoW3 vector classes of its own and over plain std::map, the way a SLAM host would call them.
//   bow_driver case.bin out.bin [vocabulary stream file]           (without arguments: compile / link check only, exit 0)
// case.bin: i32 k, L, weighting, scoring, n_nodes, D, is_f32, levelsup, F (frames); the vocabulary arrays (parent, child_offsets, children,
// desc, weight, word_id); per frame i32 N and its descriptors (N x 256 f32 or N x D u8); i32 count and u8 exclude [count] (0 or F - 1).  Frame 0 is the query, frames
// 1.. are the keyframes of the database.  With a stream file the vocabulary is loaded from it instead.
// out.bin: i32 status, bow_n, words, f64 values; i32 fv_n, per node i32 id, count, features; i32 both map types agree; i32 n_scored, per score
// i32 entry, f32 score; i32 stats [4].
#include <map>
#include "driver_common.h"
#include "rfe/bow.h"

namespace DBoW3 {   // the two classes as the reference's Thirdparty/DBoW3 declares them: maps with a few members on top
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
class BowVector : public std::map<WordId, WordValue> {
public:
    void addWeight(WordId id, WordValue v) { (*this)[id] += v; }
};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int> > {
public:
    void addFeature(NodeId id, unsigned int i) { (*this)[id].push_back(i); }
};
}  // namespace DBoW3

template <class T> static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v;
    if (!get(f, v, n)) exit(short_case());
    return v;
}
template <class T> static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
static void put_i(FILE* f, int32_t v) { fwrite(&v, 4, 1, f); }

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* f = open_case(argv[1]);
    if (!f) return EXIT_BAD_CASE;
    const std::vector<int32_t> h = take<int32_t>(f, 9);
    const int n = h[4], D = h[5], is_f32 = h[6], levelsup = h[7], F = h[8];
    const std::vector<int32_t> parent = take<int32_t>(f, n), child_off = take<int32_t>(f, n + 1), children = take<int32_t>(f, n - 1);
    const std::vector<uint8_t> desc = take<uint8_t>(f, (size_t)n * D);
    const std::vector<double> weight = take<double>(f, n);
    const std::vector<int32_t> word_id = take<int32_t>(f, n);
    std::vector<cv::Mat> frames;
    for (int i = 0; i < F; ++i) {
        const int N = take<int32_t>(f, 1)[0];
        cv::Mat m(N, is_f32 ? 256 : D, is_f32 ? CV_32F : CV_8U);
        const std::vector<uint8_t> raw = take<uint8_t>(f, (size_t)N * (is_f32 ? 1024 : D));
        if (!raw.empty()) memcpy(m.ptr<unsigned char>(0), raw.data(), raw.size());
        frames.push_back(m);
    }
    const std::vector<uint8_t> exclude = take<uint8_t>(f, (size_t)take<int32_t>(f, 1)[0]);
    fclose(f);

    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    rfe_bow_vocab* vocab = nullptr;
    int rc;
    if (argc > 3) rc = rfe_bow_vocab_load(ctx, argv[3], &vocab);
    else {
        const rfe_bow_vocab_desc d = {h[0], h[1], h[2], h[3], n, D, parent.data(), child_off.data(), children.data(), desc.data(), weight.data(),
                                      word_id.data()};
        rc = rfe_bow_vocab_create(ctx, &d, &vocab);
    }
    if (rc != RFE_OK) { fprintf(stderr, "vocabulary: %s\n", rfe_last_error(ctx)); return EXIT_LIBRARY; }
    rfe_bow_db* db = nullptr;
    if (rfe_bow_db_create(ctx, &db) != RFE_OK) return EXIT_LIBRARY;

    // the keyframes: KeyFrame::ComputeBoW3 then KeyFrameDatabase::add
    for (int i = 1; i < F; ++i) {
        DBoW3::BowVector bow; DBoW3::FeatureVector fv;
        int32_t id = -1;
        if (ORB_SLAM3::ComputeBoW3_rfe(ctx, vocab, frames[i], bow, fv, levelsup) < 0 || ORB_SLAM3::AddKeyFrame_rfe(db, bow, &id) != RFE_OK || id != i - 1) {
            fprintf(stderr, "keyframe %d: %s\n", i, rfe_last_error(ctx));
            return EXIT_LIBRARY;
        }
    }
    // the query frame, in the reference's classes and in plain maps
    DBoW3::BowVector bow; DBoW3::FeatureVector fv;
    bow.addWeight(7, 1.0); fv.addFeature(3, 9);          // stale content: the call clears both
    const int status = ORB_SLAM3::ComputeBoW3_rfe(ctx, vocab, frames[0], bow, fv, levelsup);
    std::map<unsigned, double> bow2; std::map<unsigned, std::vector<unsigned> > fv2;
    const int status2 = ORB_SLAM3::ComputeBoW3_rfe(ctx, vocab, frames[0], bow2, fv2, levelsup);
    const bool agree = status == status2 && bow2 == static_cast<const std::map<unsigned, double>&>(bow) &&
                       fv2 == static_cast<const std::map<unsigned, std::vector<unsigned> >&>(fv);
    std::vector<std::pair<int32_t, float> > scores;
    ORB_SLAM3::ScoreKeyFramesStats_rfe st;
    const int ns = ORB_SLAM3::ScoreKeyFrames_rfe(db, bow, exclude, scores, &st);
    if (status < 0 || ns < 0) fprintf(stderr, "query: %s\n", rfe_last_error(ctx));

    FILE* o = fopen(argv[2], "wb");
    if (!o) return EXIT_OUTPUT;
    put_i(o, status); put_i(o, (int32_t)bow.size());
    for (DBoW3::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) put_i(o, (int32_t)it->first);
    for (DBoW3::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) put(o, &it->second, 1);
    put_i(o, (int32_t)fv.size());
    for (DBoW3::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        put_i(o, (int32_t)it->first); put_i(o, (int32_t)it->second.size());
        put(o, it->second.data(), it->second.size());
    }
    put_i(o, agree ? 1 : 0);
    put_i(o, ns);
    for (size_t i = 0; i < scores.size(); ++i) { put_i(o, scores[i].first); put(o, &scores[i].second, 1); }
    const int32_t s4[4] = {st.maxCommonWords, st.minCommonWords, st.nSharing, st.nScored};
    put(o, s4, 4);
    fclose(o);
    rfe_bow_db_destroy(db);
    rfe_bow_vocab_destroy(vocab);
    rfe_destroy(ctx);
    return 0;
}
