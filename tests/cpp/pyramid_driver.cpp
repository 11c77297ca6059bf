// pyramid_driver.cpp -- SPextractor(1000, 1.2f, 8, 20, 7) on one frame, the way Tracking constructs it with nLevels: 8 (reference
// src/Tracking.cc:645-651), built with or without -DRFE_SP_PYRAMID=1; dumps keypoints, descriptors, the level images and the stereo
// helper's answer for the Python test.
// usage: pyramid_driver <frame.u8> H W <out.bin>     (weights via $RFE_SP_WEIGHTS)
// out.bin: i32 n | n x (x, y, response, size) f32 | n x octave i32 | n x 256 f32 | i32 L | L x (i32 rows, i32 cols, rows*cols u8) |
//          i32 stereo status | i32 all mvuRight / mvDepth == -1
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

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[2]), W = atoi(argv[3]);
    std::vector<unsigned char> raw((size_t)H * W);
    FILE* fi = fopen(argv[1], "rb");
    if (!fi || fread(raw.data(), 1, raw.size(), fi) != raw.size()) { fprintf(stderr, "cannot read frame\n"); return 2; }
    fclose(fi);

    ORB_SLAM3::SPextractor ext(1000, 1.2f, 8, 20, 7);
    MockStereoFrame F;
    F.imgLeft = cv::Mat(H, W, CV_8UC1, raw.data());
    F.imgRight = F.imgLeft;
    const int n = ext(F.imgLeft, F.mvKeys, F.mDescriptors);
    if (n != (int)F.mvKeys.size() || (n > 0 && (F.mDescriptors.rows != n || F.mDescriptors.cols != 256))) return 4;
    FILE* fo = fopen(argv[4], "wb");
    if (!fo) return 5;
    put(fo, &n, 4);
    for (int i = 0; i < n; ++i) {
        const float v[4] = {F.mvKeys[i].pt.x, F.mvKeys[i].pt.y, F.mvKeys[i].response, F.mvKeys[i].size};
        put(fo, v, 16);
    }
    for (int i = 0; i < n; ++i) put(fo, &F.mvKeys[i].octave, 4);
    for (int i = 0; i < n; ++i) put(fo, F.mDescriptors.ptr<float>(i), 1024);
    const int L = (int)ext.mvImagePyramid.size();
    put(fo, &L, 4);
    for (int l = 0; l < L; ++l) {
        const cv::Mat& m = ext.mvImagePyramid[l];
        const int r = m.empty() ? 0 : m.rows, c = m.empty() ? 0 : m.cols;
        put(fo, &r, 4); put(fo, &c, 4);
        for (int y = 0; y < r; ++y) put(fo, m.ptr<unsigned char>(y), (size_t)c);
    }
    // Frame::ComputeStereoMatches on the same view as left and right: refused as soon as a keypoint has octave > 0
    F.mvKeysRight = F.mvKeys;
    F.mDescriptorsRight = F.mDescriptors;
    const int st = ORB_SLAM3::ComputeStereoMatches_rfe(ext.featureExtractor->ExtractorSession, F);
    int all_unset = (int)(F.mvuRight.size() == F.mvKeys.size() && F.mvDepth.size() == F.mvKeys.size());
    for (size_t i = 0; i < F.mvuRight.size(); ++i) all_unset &= (int)(F.mvuRight[i] == -1.0f && F.mvDepth[i] == -1.0f);
    put(fo, &st, 4);
    put(fo, &all_unset, 4);
    fclose(fo);
    return 0;
}
