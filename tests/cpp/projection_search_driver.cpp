// projection_search_driver.cpp -- Tracking::SearchLocalPoints' call of SPmatcher::SearchByProjection1 (reference src/Tracking.cc:4178)
// through the drop-in SearchByProjection1_rfe (include/rfe/projection_search.h) on a case read from a file, with minimal Frame / MapPoint
// stand-ins that carry the reference's member names; dumps the return value and who owns every feature afterwards for the Python test.
// usage: projection_search_driver <case.bin> <out.bin>           (without arguments: compile / link check only, exit 0)
// case.bin: i32 Nm, Nf, Nleft | f32 th | i32 bFarPoints | f32 thFarPoints | f32 mnMinX, mnMinY, mnMaxX, mnMaxY, mvScaleFactors[0]
//           | Nm x u8 mbTrackInView | Nm x u8 isBad | Nm x i32 Observations | Nm x f32 mTrackDepth | Nm x f32 mTrackViewCos
//           | Nm x (mTrackProjX, mTrackProjY) f32 | Nm x 256 f32 descriptor
//           | Nf x (x, y) f32 | Nf x i32 octave | Nf x i32 prior (-1: mvpMapPoints[j] is NULL, n >= 0: a map point with n observations)
//           | Nf x 256 f32 descriptor
// out.bin:  i32 return value | Nf x i32 owner (index into vpMapPoints, -1 = NULL, -2 = the map point the feature had before the call)
#include "driver_common.h"
#include "rfe/projection_search.h"

struct MockMapPoint {                   // members SearchByProjection1 reads (src/Matchers/SPmatcher.cc:1178-1211)
    bool mbTrackInView = false, bad = false;
    int nobs = 0;
    float mTrackDepth = 0, mTrackViewCos = 0, mTrackProjX = 0, mTrackProjY = 0;
    cv::Mat desc;
    bool isBad() const { return bad; }
    int Observations() const { return nobs; }
    cv::Mat GetDescriptor() const { return desc.clone(); }
};

struct MockFrame {                      // members SearchByProjection1 / GetFeaturesInArea read
    int Nleft = -1, N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    std::vector<MockMapPoint*> mvpMapPoints;
    std::vector<float> mvScaleFactors;
    static float mnMinX, mnMinY, mnMaxX, mnMaxY;
};
float MockFrame::mnMinX = 0, MockFrame::mnMinY = 0, MockFrame::mnMaxX = 0, MockFrame::mnMaxY = 0;

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[3]; float th; int32_t far; float fl[6];
    if (fread(hd, 4, 3, fi) != 3 || fread(&th, 4, 1, fi) != 1 || fread(&far, 4, 1, fi) != 1 || fread(fl, 4, 6, fi) != 6) return EXIT_BAD_CASE;
    const int Nm = hd[0], Nf = hd[1];
    std::vector<uint8_t> inview, bad; std::vector<int32_t> nobs, octave, prior; std::vector<float> depth, vcos, proj, qd, kp, fd;
    if (!get(fi, inview, Nm) || !get(fi, bad, Nm) || !get(fi, nobs, Nm) || !get(fi, depth, Nm) || !get(fi, vcos, Nm) ||
        !get(fi, proj, (size_t)Nm * 2) || !get(fi, qd, (size_t)Nm * 256) || !get(fi, kp, (size_t)Nf * 2) || !get(fi, octave, Nf) ||
        !get(fi, prior, Nf) || !get(fi, fd, (size_t)Nf * 256)) return short_case();
    fclose(fi);
    std::vector<MockMapPoint> mps((size_t)Nm), old((size_t)Nf);
    std::vector<MockMapPoint*> vp((size_t)Nm);
    for (int i = 0; i < Nm; ++i) {
        MockMapPoint& m = mps[i];
        m.mbTrackInView = inview[i] != 0; m.bad = bad[i] != 0; m.nobs = nobs[i]; m.mTrackDepth = depth[i]; m.mTrackViewCos = vcos[i];
        m.mTrackProjX = proj[2 * i]; m.mTrackProjY = proj[2 * i + 1];
        m.desc = cv::Mat(1, 256, CV_32F, qd.data() + (size_t)i * 256);
        vp[i] = &m;
    }
    MockFrame F;
    F.Nleft = hd[2]; F.N = Nf;
    MockFrame::mnMinX = fl[1]; MockFrame::mnMinY = fl[2]; MockFrame::mnMaxX = fl[3]; MockFrame::mnMaxY = fl[4];
    F.mvScaleFactors.assign(1, fl[5]);
    F.mvKeysUn.resize((size_t)Nf);
    F.mvpMapPoints.assign((size_t)Nf, nullptr);
    F.mDescriptors = cv::Mat(Nf, 256, CV_32F, fd.data());
    for (int j = 0; j < Nf; ++j) {
        F.mvKeysUn[j].pt = cv::Point2f(kp[2 * j], kp[2 * j + 1]); F.mvKeysUn[j].octave = octave[j];
        if (prior[j] >= 0) { old[j].nobs = prior[j]; F.mvpMapPoints[j] = &old[j]; }
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    const int32_t ret = ORB_SLAM3::SearchByProjection1_rfe(ctx, F, vp, th, far != 0, fl[0]);
    std::vector<int32_t> owner((size_t)Nf, -1);
    for (int j = 0; j < Nf; ++j) {
        MockMapPoint* p = F.mvpMapPoints[j];
        if (!p) owner[j] = -1;
        else if (p == &old[j]) owner[j] = -2;
        else owner[j] = (int32_t)(p - mps.data());
    }
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    fwrite(&ret, 4, 1, fo);
    put(fo, owner);
    fclose(fo);
    return 0;
}
