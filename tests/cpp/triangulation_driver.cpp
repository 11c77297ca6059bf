// triangulation_driver.cpp -- LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:545-954) through the drop-ins of
// include/rfe/triangulation.h on a case read from a file, with minimal KeyFrame / camera / pose stand-ins that carry the reference's member
// names; dumps the list of new points, matchsum and the statistics for the Python test.
// usage: triangulation_driver <case.bin> <out.bin> [lightglue weights]    (without arguments: compile / link check only, exit 0)
//   without weights: TriangulateMatches_rfe on the case's own S / pairs; with weights (a bare float blob): CreateNewMapPoints_rfe, which runs
//   LightGlue on the case's descriptors, and the matches it used are dumped too.
// case.bin: i32 Nn, N1, N2max, Kmax, nlevels, bMonocular, bInertial, bFarPoints, NLeft of neighbour 0, has descriptors | f32 thFarPoints,
//           mfScaleFactor | nlevels x f32 mvScaleFactors | nlevels x f32 mvLevelSigma2 | the current keyframe | Nn neighbours | i32 S[Nn] |
//           i32 pairs[Nn,Kmax,2] | with descriptors: f32 [N1,256], then [N2max,256] per neighbour
//   a keyframe: f32 rcw[9], tcw[3], ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf, median depth | i32 N | N x (x, y) f32 mvKeysUn | N x (x, y)
//           f32 mvKeys | N x i32 octave | N x f32 mvuRight | N x f32 mvDepth | N x u8 GetMapPoint(i) != NULL      (N = N1, or N2max rows of
//           which the first n2 -- the i32 in front -- are features)
// out.bin:  i32 return value, Nn, Kmax, points | f32 matchsum | i32 matches[Nn] | i32 stats[8] | points x (i32 neighbour, idx1, idx2, stereo) |
//           points x 3 f32 | i32 S[Nn], pairs[Nn,Kmax,2] (with weights only)
#include "driver_common.h"
#include "rfe/triangulation.h"

struct MockMapPoint {};

struct MockKeyFrame {                   // members LocalMapping::CreateNewMapPoints and SearchForTriangulation read
    int NLeft = -1;
    MockCamera cam; MockCamera *mpCamera = &cam, *mpCamera2 = nullptr;
    MiniSE3 Tcw; Vec3 Ow;
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mb = 0, mbf = 0, median = 1.f;
    float mfScaleFactor = 1.2f; int mnScaleLevels = 1;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvuRight, mvDepth;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<uint8_t> has_mp;
    std::vector<float> desc;
    cv::Mat mDescriptors;
    MockMapPoint some;
    MiniSE3 GetPose() const { return Tcw; }
    Vec3 GetCameraCenter() const { return Ow; }
    MockMapPoint* GetMapPoint(size_t i) { return has_mp[i] ? &some : nullptr; }
    float ComputeSceneMedianDepth(int) const { return median; }
};

static bool read_keyframe(FILE* f, MockKeyFrame& kf, int rows, const std::vector<float>& sf, const std::vector<float>& sg, float scale) {
    float fl[24]; int32_t n;
    if (fread(fl, 4, 24, f) != 24 || fread(&n, 4, 1, f) != 1 || n < 0 || n > rows) return false;
    for (int k = 0; k < 9; ++k) kf.Tcw.R.m[k] = fl[k];
    for (int k = 0; k < 3; ++k) { kf.Tcw.t.v[k] = fl[9 + k]; kf.Ow.v[k] = fl[12 + k]; }
    kf.fx = fl[15]; kf.fy = fl[16]; kf.cx = fl[17]; kf.cy = fl[18]; kf.invfx = fl[19]; kf.invfy = fl[20]; kf.mb = fl[21]; kf.mbf = fl[22];
    kf.median = fl[23];
    kf.mfScaleFactor = scale; kf.mnScaleLevels = (int)sf.size(); kf.mvScaleFactors = sf; kf.mvLevelSigma2 = sg;
    std::vector<float> un, raw; std::vector<int32_t> oct;
    if (!get(f, un, (size_t)rows * 2) || !get(f, raw, (size_t)rows * 2) || !get(f, oct, rows) || !get(f, kf.mvuRight, rows) ||
        !get(f, kf.mvDepth, rows) || !get(f, kf.has_mp, rows)) return false;
    kf.mvKeys.resize((size_t)n); kf.mvKeysUn.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        kf.mvKeysUn[i].pt = cv::Point2f(un[2 * i], un[2 * i + 1]); kf.mvKeysUn[i].octave = oct[i];
        kf.mvKeys[i].pt = cv::Point2f(raw[2 * i], raw[2 * i + 1]); kf.mvKeys[i].octave = oct[i];
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[10]; float fl[2];
    if (fread(hd, 4, 10, fi) != 10 || fread(fl, 4, 2, fi) != 2) return EXIT_BAD_CASE;
    const int Nn = hd[0], N1 = hd[1], N2max = hd[2], Kmax = hd[3], nlevels = hd[4];
    std::vector<float> sf, sg;
    if (!get(fi, sf, nlevels) || !get(fi, sg, nlevels)) return EXIT_BAD_CASE;
    MockKeyFrame cur;
    std::vector<MockKeyFrame> neigh((size_t)Nn);
    if (!read_keyframe(fi, cur, N1, sf, sg, fl[1])) return short_case();
    for (MockKeyFrame& kf : neigh) if (!read_keyframe(fi, kf, N2max, sf, sg, fl[1])) return short_case();
    std::vector<int32_t> S, pairs;
    if (!get(fi, S, Nn) || !get(fi, pairs, (size_t)Nn * Kmax * 2)) return short_case();
    if (hd[9]) {
        if (!get(fi, cur.desc, (size_t)N1 * 256)) return EXIT_BAD_CASE;
        cur.mDescriptors = cv::Mat(N1, 256, CV_32F, cur.desc.data());
        for (MockKeyFrame& kf : neigh) {
            if (!get(fi, kf.desc, (size_t)N2max * 256)) return EXIT_BAD_CASE;
            kf.mDescriptors = cv::Mat(N2max, 256, CV_32F, kf.desc.data());
        }
    }
    fclose(fi);
    if (Nn > 0) neigh[0].NLeft = hd[8];
    std::vector<MockKeyFrame*> vp;
    for (MockKeyFrame& kf : neigh) { kf.mpCamera = &kf.cam; vp.push_back(&kf); }
    cur.mpCamera = &cur.cam;
    ORB_SLAM3::CreateNewMapPointsParams_rfe prm;
    prm.bMonocular = hd[5] != 0; prm.bInertial = hd[6] != 0; prm.bFarPoints = hd[7] != 0; prm.thFarPoints = fl[0];
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    ORB_SLAM3::CreateNewMapPointsOut_rfe out;
    int32_t ret;
    if (argc > 3) {
        FILE* fw = fopen(argv[3], "rb");
        std::vector<float> blob;
        const int64_t count = rfe_weight_count(RFE_KIND_LIGHTGLUE);
        if (!fw || !get(fw, blob, (size_t)count)) { fprintf(stderr, "cannot read %s\n", argv[3]); return EXIT_BAD_CASE; }
        fclose(fw);
        if (rfe_set_weights(ctx, RFE_KIND_LIGHTGLUE, blob.data(), count) != RFE_OK) { fprintf(stderr, "weights: %s\n", rfe_last_error(ctx)); return EXIT_LIBRARY; }
        prm.keep_matches = true;
        ret = ORB_SLAM3::CreateNewMapPoints_rfe(ctx, &cur, vp, prm, out);
    } else {
        int32_t *dS = nullptr, *dp = nullptr;
        if (rfe_malloc(ctx, S.size() * 4 + 4, (void**)&dS) || rfe_malloc(ctx, pairs.size() * 4 + 4, (void**)&dp)) return EXIT_LIBRARY;
        if ((!S.empty() && rfe_memcpy_h2d(ctx, dS, S.data(), S.size() * 4)) || (!pairs.empty() && rfe_memcpy_h2d(ctx, dp, pairs.data(), pairs.size() * 4)))
            return EXIT_LIBRARY;
        ret = ORB_SLAM3::TriangulateMatches_rfe(ctx, &cur, vp, prm, dS, dp, Kmax, out);
        rfe_free(ctx, dS); rfe_free(ctx, dp);
    }
    if (ret < -1) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    const int32_t head[4] = {ret, Nn, out.Kmax, (int32_t)out.points.size()};
    fwrite(head, 4, 4, fo);
    fwrite(&out.matchsum, 4, 1, fo);
    out.matches.resize((size_t)Nn);
    put(fo, out.matches);
    fwrite(out.stats, 4, 8, fo);
    std::vector<int32_t> idx; std::vector<float> xyz;
    for (const ORB_SLAM3::NewMapPoint_rfe& p : out.points) {
        idx.push_back(p.neighbour); idx.push_back(p.idx1); idx.push_back(p.idx2); idx.push_back(p.bPointStereo ? 1 : 0);
        xyz.push_back(p.x3D[0]); xyz.push_back(p.x3D[1]); xyz.push_back(p.x3D[2]);
    }
    put(fo, idx); put(fo, xyz);
    put(fo, out.S); put(fo, out.pairs);
    fclose(fo);
    return 0;
}
