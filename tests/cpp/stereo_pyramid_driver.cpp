// stereo_pyramid_driver.cpp -- the stereo Frame constructor's sequence (reference src/Frame.cc:142-171) for pyramid users: two
// SPextractor(1000, 1.2f, nlevels, 20, 7) built with -DRFE_SP_PYRAMID=1 on a left / right pair, then ComputeStereoMatchesPyramid_rfe in
// both SAD modes (and, with nlevels == 1, ComputeStereoMatches_rfe); dumps the features, the level images and the answers for the
// Python test.
// usage: stereo_pyramid_driver <left.u8> <right.u8> H W nlevels <out.bin>     (weights via $RFE_SP_WEIGHTS)
// out.bin: i32 L | per view (left, right): i32 n | n x (x, y) f32 | n x octave i32 | n x 256 f32 | L x (i32 rows, i32 cols, rows*cols u8)
//          | per SAD mode (0, 1): i32 status | n_left x mvuRight f32 | n_left x mvDepth f32
//          | i32 status of ComputeStereoMatches_rfe | n_left x mvuRight f32 | n_left x mvDepth f32
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "Extractors/SPextractor.h"
#include "rfe/stereo_match.h"

struct MockStereoFrame {                // members Frame::ComputeStereoMatches uses (src/Frame.cc:1159-1446)
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
    cv::Mat mDescriptors, mDescriptorsRight, imgLeft, imgRight;
    float mb = 0.11f, mbf = 0.11f * 435.0f;
    std::vector<float> mvuRight, mvDepth;
};

static void put(FILE* f, const void* p, size_t n) { fwrite(p, 1, n, f); }

static void put_view(FILE* fo, const std::vector<cv::KeyPoint>& k, const cv::Mat& d, const cv::Mat& img, ORB_SLAM3::SPextractor& e, int L) {
    const int n = (int)k.size();
    put(fo, &n, 4);
    for (int i = 0; i < n; ++i) { const float v[2] = {k[i].pt.x, k[i].pt.y}; put(fo, v, 8); }
    for (int i = 0; i < n; ++i) put(fo, &k[i].octave, 4);
    for (int i = 0; i < n; ++i) put(fo, d.ptr<float>(i), 1024);
    for (int l = 0; l < L; ++l) {
        const cv::Mat& m = (l == 0 && e.mvImagePyramid[0].empty()) ? img : e.mvImagePyramid[l];
        put(fo, &m.rows, 4); put(fo, &m.cols, 4);
        for (int y = 0; y < m.rows; ++y) put(fo, m.ptr<unsigned char>(y), (size_t)m.cols);
    }
}

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[3]), W = atoi(argv[4]), L = atoi(argv[5]);
    std::vector<unsigned char> raw[2] = {std::vector<unsigned char>((size_t)H * W), std::vector<unsigned char>((size_t)H * W)};
    for (int v = 0; v < 2; ++v) {
        FILE* fi = fopen(argv[1 + v], "rb");
        if (!fi || fread(raw[v].data(), 1, raw[v].size(), fi) != raw[v].size()) { fprintf(stderr, "cannot read frame\n"); return 2; }
        fclose(fi);
    }
    ORB_SLAM3::SPextractor extL(1000, 1.2f, L, 20, 7), extR(1000, 1.2f, L, 20, 7);
    MockStereoFrame F;
    F.imgLeft = cv::Mat(H, W, CV_8UC1, raw[0].data());
    F.imgRight = cv::Mat(H, W, CV_8UC1, raw[1].data());
    extL(F.imgLeft, F.mvKeys, F.mDescriptors);
    extR(F.imgRight, F.mvKeysRight, F.mDescriptorsRight);
    FILE* fo = fopen(argv[6], "wb");
    if (!fo) return 5;
    put(fo, &L, 4);
    put_view(fo, F.mvKeys, F.mDescriptors, F.imgLeft, extL, L);
    put_view(fo, F.mvKeysRight, F.mDescriptorsRight, F.imgRight, extR, L);
    rfe_ctx* ctx = extL.featureExtractor->ExtractorSession;
    const size_t n = F.mvKeys.size();
    for (int mode = 0; mode < 3; ++mode) {
        int st;
        if (mode < 2) st = ORB_SLAM3::ComputeStereoMatchesPyramid_rfe(ctx, F, extL, extR, mode == 0 ? RFE_STEREO_SAD_LEVEL : RFE_STEREO_SAD_LEVEL0);
        else st = ORB_SLAM3::ComputeStereoMatches_rfe(ctx, F);
        if (F.mvuRight.size() != n || F.mvDepth.size() != n) return 6;
        put(fo, &st, 4);
        put(fo, F.mvuRight.data(), n * 4);
        put(fo, F.mvDepth.data(), n * 4);
    }
    fclose(fo);
    return 0;
}
