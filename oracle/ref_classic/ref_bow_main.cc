// Command-line harness around DBoW3's and KeyFrameDatabase's OWN function bodies.  The *.inc files are cut by build_ref.py out of the
// Rover-SLAM checkout (Thirdparty/DBoW3/src/Vocabulary.cpp, DescManip.cpp; src/KeyFrameDatabase.cc); BowVector.cpp, FeatureVector.cpp,
// ScoringObject.cpp and quicklz.c are compiled from the checkout as they are, and DBoW3's own headers come from its include path.  All
// of that is a build product under oracle/_ref/ and never committed.  Everything in THIS file is the project's: argument plumbing, and
// stubs for the Vocabulary members the harness does not compile (k-means training, the YAML loader, the bow-only transforms).
//   ref_bow <op> <in> <out>       op: voc_dump | voc_write | transform | score | kfdb        <in> / <out>: the array files of ref_io.h
// No Python in the process.  A case outside the reference's defined behaviour ends THIS process, not the caller.
#define RFE_REF_BOW
#include <cassert>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <sstream>
#include "ref_classes.h"
#include "DescManip.h"
#include "quicklz.h"
#include "ref_io.h"

// ---- the reference's text ---------------------------------------------------------------------------------------------------
namespace DBoW3 {
#include "voc_ctor.inc"
#include "voc_dtor.inc"
#include "voc_scoring.inc"
#include "voc_transform.inc"
#include "voc_transform1.inc"
#include "voc_tostream.inc"
#include "voc_fromstream.inc"
#include "descmanip_distance.inc"
#include "descmanip_tostream.inc"
#include "descmanip_fromstream.inc"

// The rest of Vocabulary's virtual table: not compiled from the reference, never called here.
#define RFE_UNPINNED { throw std::logic_error("ref_bow: a DBoW3 function the harness does not compile was called"); }
void Vocabulary::create(const std::vector<std::vector<cv::Mat> >&) RFE_UNPINNED
void Vocabulary::create(const std::vector<cv::Mat>&) RFE_UNPINNED
void Vocabulary::create(const std::vector<std::vector<cv::Mat> >&, int, int) RFE_UNPINNED
void Vocabulary::create(const std::vector<std::vector<cv::Mat> >&, int, int, WeightingType, ScoringType) RFE_UNPINNED
void Vocabulary::transform(const std::vector<cv::Mat>&, BowVector&) const RFE_UNPINNED
void Vocabulary::transform(const cv::Mat&, BowVector&) const RFE_UNPINNED
WordId Vocabulary::transform(const cv::Mat&) const RFE_UNPINNED
void Vocabulary::transform(const cv::Mat&, WordId&, WordValue&) const RFE_UNPINNED
void Vocabulary::transform(const cv::Mat&, WordId&) const RFE_UNPINNED
NodeId Vocabulary::getParentNode(WordId, int) const RFE_UNPINNED
cv::Mat Vocabulary::getWord(WordId) const RFE_UNPINNED
WordValue Vocabulary::getWordWeight(WordId) const RFE_UNPINNED
void Vocabulary::save(cv::FileStorage&, const std::string&) const RFE_UNPINNED
void Vocabulary::load(const cv::FileStorage&, const std::string&) RFE_UNPINNED
int Vocabulary::stopWords(double) RFE_UNPINNED
void Vocabulary::initiateClusters(const std::vector<cv::Mat>&, std::vector<cv::Mat>&) const RFE_UNPINNED
}  // namespace DBoW3

namespace ORB_SLAM3 {
#include "kfdb_add.inc"
#include "kfdb_erase.inc"
void KeyFrameDatabase::FrontNBest_sp(KeyFrame* pKF, Front& front) {
#include "kfdb_nbest_sp.inc"
    front.early = false; front.maxCommonWords = maxCommonWords; front.minCommonWords = minCommonWords;
    front.sharing = lKFsSharingWords; front.scored = lScoreAndMatch;
}
std::vector<KeyFrame*> KeyFrameDatabase::FrontReloc(Frame* F, Front& front) {
#include "kfdb_reloc.inc"
    front.early = false; front.maxCommonWords = maxCommonWords; front.minCommonWords = minCommonWords;
    front.sharing = lKFsSharingWords; front.scored = lScoreAndMatch;
    return std::vector<KeyFrame*>();
}
}  // namespace ORB_SLAM3

// ---- plumbing ---------------------------------------------------------------------------------------------------------------
namespace {
// the protected tree and the protected per-feature overload, opened for the dump and the per-feature record
struct OpenVoc : DBoW3::Vocabulary {
    OpenVoc() : DBoW3::Vocabulary(10, 5, DBoW3::TF_IDF, DBoW3::L1_NORM) {}
    using DBoW3::Vocabulary::transform;
    typedef Node node_type;
    const std::vector<Node>& nodes() const { return m_nodes; }
    const std::vector<Node*>& words() const { return m_words; }
};

void load(OpenVoc& v, const Arr& stream) {
    std::istringstream is(std::string((const char*)stream.u8(), stream.n()), std::ios::binary);
    v.fromStream(is);
    want(!is.fail(), "fromStream: the stream ended early");
}

// in: stream u8.  out: hdr i32 [k, L, scoring, weighting, n_nodes, n_words], parent i32 [n] (root -1), child_offsets i32 [n + 1],
// children i32 IN THE ORDER m_nodes[i].children HOLDS THEM, desc_cols i32 [n], desc u8 (rows one after the other), weight f64 [n],
// word_id i32 [n] (-1 for a node with children), words i32 [n_words] = m_words[w]->id
void op_voc_dump(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 1, "voc_dump: arguments");
    OpenVoc v; load(v, in[0]);
    const auto& nodes = v.nodes();
    const int n = (int)nodes.size();
    std::vector<int32_t> hdr = {v.getBranchingFactor(), v.getDepthLevels(), (int)v.getScoringType(), (int)v.getWeightingType(), n, (int)v.size()};
    std::vector<int32_t> parent, off(1, 0), children, cols, word_id, words;
    std::vector<uint8_t> desc; std::vector<double> weight;
    for (int i = 0; i < n; ++i) {
        const OpenVoc::node_type& nd = nodes[i];
        want((int)nd.id == i, "voc_dump: a node's id is not its index");
        parent.push_back(i == 0 ? -1 : (int32_t)nd.parent);
        for (DBoW3::NodeId c : nd.children) children.push_back((int32_t)c);
        off.push_back((int32_t)children.size());
        want(nd.descriptor.empty() || (nd.descriptor.rows == 1 && nd.descriptor.type() == CV_8U), "voc_dump: descriptor shape");
        cols.push_back(nd.descriptor.cols);
        if (!nd.descriptor.empty()) desc.insert(desc.end(), nd.descriptor.ptr(0), nd.descriptor.ptr(0) + nd.descriptor.cols);
        weight.push_back(nd.weight);
        word_id.push_back(nd.isLeaf() ? (int32_t)nd.word_id : -1);
    }
    for (const OpenVoc::node_type* w : v.words()) { want(w != nullptr, "voc_dump: a word without node"); words.push_back((int32_t)w->id); }
    out.add(1, hdr); out.add(1, parent); out.add(1, off); out.add(1, children); out.add(1, cols); out.add(0, desc); out.add(3, weight);
    out.add(1, word_id); out.add(1, words);
}

// in: stream u8, pi i32 [compressed].  out: u8 = what Vocabulary::toStream wrote
void op_voc_write(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 2 && in[1].n() == 1, "voc_write: arguments");
    OpenVoc v; load(v, in[0]);
    std::ostringstream os(std::ios::binary);
    v.toStream(os, in[1].i32()[0] != 0);
    const std::string s = os.str();
    out.add(0, (const uint8_t*)s.data(), s.size());
}

// in: stream u8, feats u8 [N * D], pi i32 [N, D, levelsup].  out: per feature word i32, nid i32 (-1: the descent never wrote *nid),
// weight f64 (the protected per-feature overload, called once more with *nid preset); then of the vector overload bow_word i32, bow_value
// f64 in map order, fv_node i32, fv_offsets i32 [fv_n + 1], fv_feat i32.  Where some nid is -1 the vector overload's FeatureVector was filed
// under an uninitialised node id: the caller must not use fv_* of such a case.
void op_transform(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 3 && in[2].n() == 3, "transform: arguments");
    const int N = in[2].i32()[0], D = in[2].i32()[1], levelsup = in[2].i32()[2];
    want(N >= 0 && D > 0 && D % 8 == 0 && in[1].n() == (size_t)N * D, "transform: sizes");
    OpenVoc v; load(v, in[0]);
    want(!v.empty() && v.words()[0]->descriptor.cols == D, "transform: descriptor width");
    std::vector<uint64_t> aligned(((size_t)N * D + 7) / 8 + 1);            // DescManip::distance reads the rows as uint64_t
    if (N) std::memcpy(aligned.data(), in[1].u8(), (size_t)N * D);
    std::vector<cv::Mat> feats;
    for (int i = 0; i < N; ++i) feats.push_back(cv::Mat(1, D, CV_8U, (uint8_t*)aligned.data() + (size_t)i * D));
    std::vector<int32_t> word, nid; std::vector<double> weight;
    for (int i = 0; i < N; ++i) {
        DBoW3::WordId id = 0; DBoW3::WordValue w = 0; DBoW3::NodeId n = 0xFFFFFFFFu;
        v.transform(feats[i], id, w, &n, levelsup);
        word.push_back((int32_t)id); nid.push_back(n == 0xFFFFFFFFu ? -1 : (int32_t)n); weight.push_back(w);
    }
    DBoW3::BowVector bv; DBoW3::FeatureVector fv;
    v.transform(feats, bv, fv, levelsup);
    std::vector<int32_t> bw, fn, fo(1, 0), ff; std::vector<double> bx;
    for (const auto& e : bv) { bw.push_back((int32_t)e.first); bx.push_back(e.second); }
    for (const auto& e : fv) {
        fn.push_back((int32_t)e.first);
        for (unsigned int f : e.second) ff.push_back((int32_t)f);
        fo.push_back((int32_t)ff.size());
    }
    out.add(1, word); out.add(1, nid); out.add(3, weight); out.add(1, bw); out.add(3, bx); out.add(1, fn); out.add(1, fo); out.add(1, ff);
}

DBoW3::BowVector bow_of(const int32_t* w, const double* x, size_t n) {
    DBoW3::BowVector b;
    for (size_t i = 0; i < n; ++i) {
        want(w[i] >= 0 && (i == 0 || w[i] > w[i - 1]), "a BowVector's words must ascend");
        b.insert(b.end(), std::make_pair((DBoW3::WordId)w[i], x[i]));
    }
    return b;
}

// in: w1 i32, v1 f64, w2 i32, v2 f64.  out: f64 [1] = L1Scoring::score, reached through Vocabulary::score as the callers reach it
void op_score(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 4 && in[0].n() == in[1].n() && in[2].n() == in[3].n(), "score: arguments");
    OpenVoc v;
    const double s = v.score(bow_of(in[0].i32(), in[1].f64(), in[0].n()), bow_of(in[2].i32(), in[3].f64(), in[2].n()));
    out.add(3, &s, 1);
}

// in: pi i32 [n_words], ops i32 [n_ops * 2] = (op, arg): 0 add BowVector arg as the next keyframe, 1 erase keyframe arg, 2 query with
// BowVector arg through DetectNBestCandidates_sp's front (the next connected set), 3 query through DetectRelocalizationCandidates' front
// (its connected set is ignored); bow_off i32 [n_bows + 1], bow_word i32, bow_value f64; conn_off i32 [n_queries + 1], conn i32
// (keyframe indices).  out, per query x keyframe (E = number of adds in the script): sharing u8 (in lKFsSharingWords), words i32
// (mnPlaceRecognitionWords / mnRelocWords; -1: untouched by this query), scored u8 (in lScoreAndMatch), score f32 (the stored float; -9.5
// where not scored), score64 f64 (Vocabulary::score of the pair, the double that float was made from; 0 where not scored); stats i32
// [n_queries * 5] = returned inside the range, maxCommonWords, minCommonWords, lKFsSharingWords.size(), lScoreAndMatch.size()
void op_kfdb(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 7 && in[0].n() == 1 && in[1].n() % 2 == 0 && in[2].n() >= 1 && in[3].n() == in[4].n() && in[5].n() >= 1, "kfdb: arguments");
    const int n_words = in[0].i32()[0], n_ops = (int)(in[1].n() / 2), n_bows = (int)in[2].n() - 1, n_q = (int)in[5].n() - 1;
    const int32_t *ops = in[1].i32(), *boff = in[2].i32(), *coff = in[5].i32(), *conn = in[6].i32();
    want(n_words > 0 && boff[0] == 0 && boff[n_bows] == (int)in[3].n() && coff[0] == 0 && coff[n_q] == (int)in[6].n(), "kfdb: offsets");
    std::vector<DBoW3::BowVector> bows;
    for (int b = 0; b < n_bows; ++b) {
        want(boff[b] <= boff[b + 1], "kfdb: bow offsets");
        bows.push_back(bow_of(in[3].i32() + boff[b], in[4].f64() + boff[b], (size_t)(boff[b + 1] - boff[b])));
        want(bows.back().empty() || (int)bows.back().rbegin()->first < n_words, "kfdb: a word outside the inverted file");
    }
    int E = 0, nq_seen = 0;
    for (int i = 0; i < n_ops; ++i) { E += ops[2 * i] == 0; nq_seen += ops[2 * i] >= 2; }
    want(nq_seen == n_q, "kfdb: one connected set per query");
    OpenVoc voc;
    ORB_SLAM3::KeyFrameDatabase db(voc, (size_t)n_words);
    std::vector<std::unique_ptr<ORB_SLAM3::KeyFrame> > kfs;
    std::vector<uint8_t> sharing((size_t)n_q * E, 0), scored((size_t)n_q * E, 0);
    std::vector<int32_t> words((size_t)n_q * E, -1), stats;
    std::vector<float> score((size_t)n_q * E, -9.5f); std::vector<double> score64((size_t)n_q * E, 0.0);
    int q = 0;
    for (int i = 0; i < n_ops; ++i) {
        const int op = ops[2 * i], arg = ops[2 * i + 1];
        if (op == 0) {
            want(arg >= 0 && arg < n_bows, "kfdb: add");
            kfs.emplace_back(new ORB_SLAM3::KeyFrame());
            ORB_SLAM3::KeyFrame& k = *kfs.back();
            k.mnId = kfs.size() - 1; k.mBow3Vec = bows[arg];
            k.mnPlaceRecognitionQuery = k.mnRelocQuery = std::numeric_limits<long unsigned int>::max();
            k.mnPlaceRecognitionWords = k.mnRelocWords = -1; k.mPlaceRecognitionScore = k.mRelocScore = -9.5f;
            db.add(&k);
        } else if (op == 1) {
            want(arg >= 0 && arg < (int)kfs.size(), "kfdb: erase");
            db.erase(kfs[arg].get());
        } else if (op == 2 || op == 3) {
            want(arg >= 0 && arg < n_bows, "kfdb: query");
            for (auto& k : kfs) { k->mnPlaceRecognitionWords = k->mnRelocWords = -1; k->mPlaceRecognitionScore = k->mRelocScore = -9.5f; }
            ORB_SLAM3::KeyFrameDatabase::Front front;
            const long unsigned int id = 1000000ul + (long unsigned int)q;
            if (op == 2) {
                ORB_SLAM3::KeyFrame cur; cur.mnId = id; cur.mBow3Vec = bows[arg];
                for (int c = coff[q]; c < coff[q + 1]; ++c) { want(conn[c] >= 0 && conn[c] < (int)kfs.size(), "kfdb: connected"); cur.connected.insert(kfs[conn[c]].get()); }
                db.FrontNBest_sp(&cur, front);
            } else {
                ORB_SLAM3::Frame F; F.mnId = id; F.mBow3Vec = bows[arg];
                db.FrontReloc(&F, front);
            }
            for (size_t e = 0; e < kfs.size(); ++e) words[(size_t)q * E + e] = op == 2 ? kfs[e]->mnPlaceRecognitionWords : kfs[e]->mnRelocWords;
            for (ORB_SLAM3::KeyFrame* k : front.sharing) sharing[(size_t)q * E + k->mnId] = 1;
            for (const auto& sk : front.scored) {
                const size_t at = (size_t)q * E + sk.second->mnId;
                want((op == 2 ? sk.second->mPlaceRecognitionScore : sk.second->mRelocScore) == sk.first, "kfdb: stored score");
                scored[at] = 1; score[at] = sk.first; score64[at] = voc.score(bows[arg], sk.second->mBow3Vec);
            }
            stats.push_back(front.early); stats.push_back(front.maxCommonWords); stats.push_back(front.minCommonWords);
            stats.push_back((int32_t)front.sharing.size()); stats.push_back((int32_t)front.scored.size());
            ++q;
        } else {
            throw std::runtime_error("kfdb: unknown operation");
        }
    }
    out.add(0, sharing); out.add(1, words); out.add(0, scored); out.add(2, score); out.add(3, score64); out.add(1, stats);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <op> <in> <out>\n", argv[0]); return 2; }
    try {
        const std::string op = argv[1];
        const std::vector<Arr> in = read_all(argv[2]);
        Writer out;
        if (op == "voc_dump") op_voc_dump(in, out);
        else if (op == "voc_write") op_voc_write(in, out);
        else if (op == "transform") op_transform(in, out);
        else if (op == "score") op_score(in, out);
        else if (op == "kfdb") op_kfdb(in, out);
        else throw std::runtime_error("unknown op " + op);
        out.write(argv[3]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_bow: %s\n", e.what());
        return 3;
    }
    return 0;
}
