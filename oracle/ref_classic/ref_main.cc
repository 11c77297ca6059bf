// Command-line harness around the reference's OWN function bodies (the *.inc files build_ref.py cuts out of the Rover-SLAM checkout;
// they are build products under oracle/_ref/ and never committed).  Everything in this file is the project's: argument plumbing only.
//   ref_classic <op> <in> <out>       op: stereo | geometry | distance | distinctive | normkp | binarize
// <in> / <out>: the array files of ref_io.h.
// A case outside the reference's defined behaviour ends THIS process (exception, library assertion, sanitizer), not the caller.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "ref_classes.h"
#include "ref_io.h"

// ---- the reference's text ---------------------------------------------------------------------------------------------------
namespace ORB_SLAM3 {
#include "spmatcher_th.inc"
#include "spmatcher_distance.inc"
#include "frame_stereo.inc"
#include "frame_binarize.inc"
#include "mappoint_distinctive.inc"
}  // namespace ORB_SLAM3

#include "transform_normkp.inc"

namespace ORB_SLAM3 {
using namespace cv;
void SPextractor::InitScales() {
#include "spx_scales.inc"
}
void SPextractor::InitFeaturesPerLevel() {
#include "spx_fpl.inc"   // ends with the constructor's own closing brace
cv::Size SPextractor::LevelSize(cv::Mat image, int level) {
#include "spx_levelsize.inc"
    return sz;
}
}  // namespace ORB_SLAM3

// ---- plumbing ---------------------------------------------------------------------------------------------------------------
namespace {
// in: pi [H, W, nlevels, N, Nr], pf [mb, mbf, scale_factor], imgL, imgR u8 [H*W] (level 0), kL f32 [N*2], octL i32 [N], kR, octR,
// dL f32 [N*256], dR.  out: mvuRight f32 [N], mvDepth f32 [N]
void op_stereo(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 10 && in[0].n() == 5 && in[1].n() == 3, "stereo: arguments");
    const int32_t* pi = in[0].i32(); const float* pf = in[1].f32();
    const int H = pi[0], W = pi[1], L = pi[2], N = pi[3], Nr = pi[4];
    want(H > 0 && W > 0 && L >= 1 && N >= 0 && Nr >= 0, "stereo: sizes");
    want(in[2].n() == (size_t)H * W && in[3].n() == (size_t)H * W, "stereo: images");
    want(in[4].n() == (size_t)N * 2 && in[5].n() == (size_t)N && in[6].n() == (size_t)Nr * 2 && in[7].n() == (size_t)Nr, "stereo: keypoints");
    want(in[8].n() == (size_t)N * 256 && in[9].n() == (size_t)Nr * 256, "stereo: descriptors");
    ORB_SLAM3::SPextractor ex(1000, pf[2], L);     // the Frame takes its scale tables from the extractor (GetScaleFactors)
    ORB_SLAM3::Frame F;
    F.mb = pf[0]; F.mbf = pf[1]; F.N = N;
    F.mvScaleFactors = ex.mvScaleFactor; F.mvInvScaleFactors = ex.mvInvScaleFactor;
    F.imgLeft = cv::Mat(H, W, CV_8UC1, (void*)in[2].u8()); F.imgRight = cv::Mat(H, W, CV_8UC1, (void*)in[3].u8());
    const float *kL = in[4].f32(), *kR = in[6].f32(); const int32_t *oL = in[5].i32(), *oR = in[7].i32();
    for (int i = 0; i < N; ++i) { want(oL[i] >= 0 && oL[i] < L, "stereo: left octave"); F.mvKeys.push_back(cv::KeyPoint(kL[2 * i], kL[2 * i + 1], 1.f, -1, 0, oL[i])); }
    for (int i = 0; i < Nr; ++i) { want(oR[i] >= 0 && oR[i] < L, "stereo: right octave"); F.mvKeysRight.push_back(cv::KeyPoint(kR[2 * i], kR[2 * i + 1], 1.f, -1, 0, oR[i])); }
    F.mDescriptors = cv::Mat(N, 256, CV_32F, (void*)in[8].f32()); F.mDescriptorsRight = cv::Mat(Nr, 256, CV_32F, (void*)in[9].f32());
    F.ComputeStereoMatches();
    want(F.mvuRight.size() == (size_t)N && F.mvDepth.size() == (size_t)N, "stereo: output size");
    out.add(2, F.mvuRight.data(), (size_t)N); out.add(2, F.mvDepth.data(), (size_t)N);
}

// in: pi [H, W, nlevels, nfeatures], pf [scale_factor].  out: scale f32 [L], inv f32 [L], level_w i32 [L], level_h i32 [L], fpl i32 [L]
void op_geometry(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 2 && in[0].n() == 4 && in[1].n() == 1, "geometry: arguments");
    const int32_t* pi = in[0].i32();
    const int H = pi[0], W = pi[1], L = pi[2];
    want(H > 0 && W > 0 && L >= 1, "geometry: sizes");
    ORB_SLAM3::SPextractor ex(pi[3], in[1].f32()[0], L);
    cv::Mat image(H, W, CV_8UC1);
    std::vector<int32_t> lw, lh;
    for (int l = 0; l < L; ++l) { cv::Size s = ex.LevelSize(image, l); lw.push_back(s.width); lh.push_back(s.height); }
    std::vector<int32_t> fpl(ex.mnFeaturesPerLevel.begin(), ex.mnFeaturesPerLevel.end());
    out.add(2, ex.mvScaleFactor.data(), (size_t)L); out.add(2, ex.mvInvScaleFactor.data(), (size_t)L);
    out.add(1, lw.data(), (size_t)L); out.add(1, lh.data(), (size_t)L); out.add(1, fpl.data(), (size_t)L);
}

// in: a f32 [M*256], b f32 [N*256].  out: f32 [M*N]
void op_distance(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 2 && in[0].n() % 256 == 0 && in[1].n() % 256 == 0, "distance: arguments");
    const int M = (int)(in[0].n() / 256), N = (int)(in[1].n() / 256);
    cv::Mat a(M, 256, CV_32F, (void*)in[0].f32()), b(N, 256, CV_32F, (void*)in[1].f32());
    std::vector<float> d((size_t)M * N);
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) d[(size_t)i * N + j] = ORB_SLAM3::SPmatcher::DescriptorDistance_sp(a.row(i), b.row(j));
    out.add(2, d.data(), d.size());
}

// in: desc f32 [total*256], offsets i32 [Np+1].  out: i32 [Np] = the observation whose row became mDescriptor (-1: the function
// returned without choosing).  The KeyFrame stand-ins of a point lie in ONE array, so that the reference's map<KeyFrame*, ...>
// iterates them in observation order; KeyFrame j of a point holds observation 2j as its left index and 2j+1 as its right index.
void op_distinctive(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 2 && in[0].n() % 256 == 0 && in[1].n() >= 1, "distinctive: arguments");
    const int total = (int)(in[0].n() / 256), Np = (int)in[1].n() - 1;
    const int32_t* off = in[1].i32();
    std::vector<int32_t> best((size_t)Np, -1);
    for (int p = 0; p < Np; ++p) {
        const int o = off[p], n = off[p + 1] - o;
        want(o >= 0 && n >= 0 && o + n <= total, "distinctive: offsets");
        std::vector<ORB_SLAM3::KeyFrame> kfs((size_t)(n + 1) / 2);
        ORB_SLAM3::MapPoint mp;
        for (int j = 0; j < (int)kfs.size(); ++j) {
            kfs[j].mDescriptors = cv::Mat(n, 256, CV_32F, (void*)(in[0].f32() + (size_t)o * 256));
            mp.mObservations[&kfs[j]] = std::make_tuple(2 * j, 2 * j + 1 < n ? 2 * j + 1 : -1);
        }
        mp.ComputeDistinctiveDescriptors();
        best[p] = mp.mDescriptor.empty() ? -1 : mp.mDescriptor.tag;
    }
    out.add(1, best.data(), best.size());
}

// in: kpts f32 [n*2], pi [h, w].  out: f32 [n*2]
void op_normkp(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 2 && in[0].n() % 2 == 0 && in[1].n() == 2, "normkp: arguments");
    const float* k = in[0].f32();
    std::vector<cv::Point2f> pts;
    for (size_t i = 0; i < in[0].n() / 2; ++i) pts.push_back(cv::Point2f(k[2 * i], k[2 * i + 1]));
    std::vector<cv::Point2f> r = NormalizeKeypoints(pts, in[1].i32()[0], in[1].i32()[1]);
    want(r.size() == pts.size(), "normkp: output size");
    std::vector<float> o;
    for (const cv::Point2f& p : r) { o.push_back(p.x); o.push_back(p.y); }
    out.add(2, o.data(), o.size());
}

// in: desc f32 [rows*256].  out: u8 [rows*256]
void op_binarize(const std::vector<Arr>& in, Writer& out) {
    want(in.size() == 1 && in[0].n() % 256 == 0, "binarize: arguments");
    const int rows = (int)(in[0].n() / 256);
    ORB_SLAM3::Frame F;
    F.mDescriptors = cv::Mat(rows, 256, CV_32F, (void*)in[0].f32());
    F.binarize_descriptors();
    want(F.mDescriptors_bin.rows == rows && F.mDescriptors_bin.cols == 256 && F.mDescriptors_bin.type() == CV_8UC1, "binarize: output");
    std::vector<uint8_t> o;
    for (int y = 0; y < rows; ++y) o.insert(o.end(), F.mDescriptors_bin.ptr(y), F.mDescriptors_bin.ptr(y) + 256);
    out.add(0, o.data(), o.size());
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <op> <in> <out>\n", argv[0]); return 2; }
    try {
        const std::string op = argv[1];
        const std::vector<Arr> in = read_all(argv[2]);
        Writer out;
        if (op == "stereo") op_stereo(in, out);
        else if (op == "geometry") op_geometry(in, out);
        else if (op == "distance") op_distance(in, out);
        else if (op == "distinctive") op_distinctive(in, out);
        else if (op == "normkp") op_normkp(in, out);
        else if (op == "binarize") op_binarize(in, out);
        else throw std::runtime_error("unknown op " + op);
        out.write(argv[3]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_classic: %s\n", e.what());
        return 3;
    }
    return 0;
}
