// local_points_driver.cpp -- steps 2 and 3 of Tracking::SearchLocalPoints (reference src/Tracking.cc:4119-4180) through the drop-in
// SearchLocalPoints_rfe (include/rfe/local_points_search.h) on a case read from a file, with minimal Frame / MapPoint / camera / pose
// stand-ins that carry the reference's member names; dumps the return value, nToMatch, F.mvpMapPoints and every tracking field of every map
// point for the Python test.
// usage: local_points_driver <case.bin> <out.bin>           (without arguments: compile / link check only, exit 0)
// case.bin: i32 Np, Nf, Nleft, nlevels, bFarPoints, frame id | f32 mRcw[9] (row-major), mtcw[3], mOw[3], fx, fy, cx, cy, mbf, mnMinX, mnMinY,
//           mnMaxX, mnMaxY, mfLogScaleFactor, th, thFarPoints | nlevels x f32 mvScaleFactors | Np x u8 isBad | Np x i32 mnLastFrameSeen
//           | Np x u8 Observations() > 0 | the fields before the call: Np x u8 mbTrackInView, Np x f32 mTrackProjX, mTrackProjY, mTrackProjXR,
//           mTrackDepth, Np x i32 mnTrackScaleLevel, Np x f32 mTrackViewCos, Np x i32 mnVisible
//           | Nf x i32 prior (-1: F.mvpMapPoints[j] is NULL, -2: an observed map point that is not in the list, -3: an unobserved one)
//           | Nf x i32 octave | Np x 3 f32 world position | Np x 3 f32 normal | Np x f32 GetMinDistanceInvariance | Np x f32
//           GetMaxDistanceInvariance | Np x f32 mfMaxDistance | Np x 256 f32 descriptor | Nf x (x, y) f32 | Nf x 256 f32 descriptor
// out.bin:  i32 return value, nToMatch | Nf x i32 F.mvpMapPoints (index into the list, or the prior code) | the fields after the call, laid out
//           as before it
#include <map>
#include "driver_common.h"
#include "rfe/local_points_search.h"

struct MockMapPoint {                   // members Tracking::SearchLocalPoints, Frame::isInFrustum and SearchByProjection1 read or write
    long unsigned int mnId = 0, mnLastFrameSeen = 0;
    bool bad = false, observed = true;
    int mnVisible = 1;
    Vec3 pos, nrm;
    float dmin = 0, dmax = 0, maxd = 0;
    cv::Mat desc;
    bool mbTrackInView = false;
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackDepth = 0, mTrackViewCos = 0;
    int mnTrackScaleLevel = 0;
    bool isBad() const { return bad; }
    int Observations() const { return observed ? 3 : 0; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    Vec3 GetWorldPos() const { return pos; }
    Vec3 GetNormal() const { return nrm; }
    float GetMinDistanceInvariance() const { return dmin; }
    float GetMaxDistanceInvariance() const { return dmax; }
    float GetMaxDistance() const { return maxd; }          // the accessor include/rfe/sim3_search.h asks the reference to add
    cv::Mat GetDescriptor() const { return desc.clone(); }
};

struct MockFrame {
    int Nleft = -1;
    long unsigned int mnId = 0;
    MiniSE3 Tcw; Vec3 Ow;
    MockCamera* mpCamera = nullptr;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    float mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;   // Frame keeps its bounds as static float (include/Frame.h)
    int mnScaleLevels = 1;
    float mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    std::vector<MockMapPoint*> mvpMapPoints;
    std::map<long unsigned int, cv::Point2f> mmProjectPoints;
    MiniSE3 GetPose() const { return Tcw; }
    Vec3 GetOw() const { return Ow; }
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[6]; float fl[27];
    if (fread(hd, 4, 6, fi) != 6 || fread(fl, 4, 27, fi) != 27) return EXIT_BAD_CASE;
    const int Np = hd[0], Nf = hd[1], nlevels = hd[3];
    std::vector<float> sf, px, py, pxr, dep, vc, pw, nr, dmin, dmax, maxd, qd, kp, fd;
    std::vector<uint8_t> bad, obs, inview; std::vector<int32_t> seen, lev, vis, prior, oct;
    if (!get(fi, sf, nlevels) || !get(fi, bad, Np) || !get(fi, seen, Np) || !get(fi, obs, Np) || !get(fi, inview, Np) || !get(fi, px, Np) ||
        !get(fi, py, Np) || !get(fi, pxr, Np) || !get(fi, dep, Np) || !get(fi, lev, Np) || !get(fi, vc, Np) || !get(fi, vis, Np) ||
        !get(fi, prior, Nf) || !get(fi, oct, Nf) || !get(fi, pw, (size_t)Np * 3) || !get(fi, nr, (size_t)Np * 3) || !get(fi, dmin, Np) ||
        !get(fi, dmax, Np) || !get(fi, maxd, Np) || !get(fi, qd, (size_t)Np * 256) || !get(fi, kp, (size_t)Nf * 2) ||
        !get(fi, fd, (size_t)Nf * 256)) return short_case();
    fclose(fi);
    std::vector<MockMapPoint> mps((size_t)Np);
    MockMapPoint other_observed, other_unobserved;
    other_unobserved.observed = false;
    std::vector<MockMapPoint*> vp((size_t)Np);
    for (int i = 0; i < Np; ++i) {
        MockMapPoint& m = mps[i];
        m.mnId = 1000 + (long unsigned int)i; m.mnLastFrameSeen = (long unsigned int)seen[i];
        m.bad = bad[i] != 0; m.observed = obs[i] != 0; m.mnVisible = vis[i];
        m.dmin = dmin[i]; m.dmax = dmax[i]; m.maxd = maxd[i];
        for (int k = 0; k < 3; ++k) { m.pos.v[k] = pw[3 * (size_t)i + k]; m.nrm.v[k] = nr[3 * (size_t)i + k]; }
        m.desc = cv::Mat(1, 256, CV_32F, qd.data() + (size_t)i * 256);
        m.mbTrackInView = inview[i] != 0; m.mTrackProjX = px[i]; m.mTrackProjY = py[i]; m.mTrackProjXR = pxr[i]; m.mTrackDepth = dep[i];
        m.mnTrackScaleLevel = lev[i]; m.mTrackViewCos = vc[i];
        vp[i] = &m;
    }
    MockCamera cam;
    MockFrame F;
    F.Nleft = hd[2]; F.mnId = (long unsigned int)hd[5]; F.mpCamera = &cam;
    for (int k = 0; k < 9; ++k) F.Tcw.R.m[k] = fl[k];
    for (int k = 0; k < 3; ++k) { F.Tcw.t.v[k] = fl[9 + k]; F.Ow.v[k] = fl[12 + k]; }
    F.fx = fl[15]; F.fy = fl[16]; F.cx = fl[17]; F.cy = fl[18]; F.mbf = fl[19];
    F.mnMinX = fl[20]; F.mnMinY = fl[21]; F.mnMaxX = fl[22]; F.mnMaxY = fl[23];
    F.mnScaleLevels = nlevels; F.mfLogScaleFactor = fl[24]; F.mvScaleFactors = sf;
    const float th = fl[25], thFarPoints = fl[26];
    F.mvKeysUn.resize((size_t)Nf);
    F.mDescriptors = cv::Mat(Nf, 256, CV_32F, fd.data());
    F.mvpMapPoints.assign((size_t)Nf, nullptr);
    for (int j = 0; j < Nf; ++j) {
        F.mvKeysUn[j].pt = cv::Point2f(kp[2 * j], kp[2 * j + 1]); F.mvKeysUn[j].octave = oct[j];
        F.mvpMapPoints[j] = prior[j] == -2 ? &other_observed : (prior[j] == -3 ? &other_unobserved : nullptr);
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    int nToMatch = -7;
    const int32_t ret = ORB_SLAM3::SearchLocalPoints_rfe(ctx, F, vp, th, hd[4] != 0, thFarPoints, &nToMatch);
    rfe_destroy(ctx);
    // mmProjectPoints holds the projection of exactly the points in view
    int in_view = 0;
    for (int i = 0; i < Np; ++i) {
        const MockMapPoint& m = mps[i];
        const bool fresh = m.mbTrackInView && !m.bad && m.mnLastFrameSeen != F.mnId && ret >= 0;
        if (!fresh) continue;
        ++in_view;
        const auto it = F.mmProjectPoints.find(m.mnId);
        const auto same = [](float a, float b) { return a == b || (a != a && b != b); };      // a NaN projection is stored as it is
        if (it == F.mmProjectPoints.end() || !same(it->second.x, m.mTrackProjX) || !same(it->second.y, m.mTrackProjY)) { fprintf(stderr, "mmProjectPoints\n"); return 4; }
    }
    if (ret >= 0 && (int)F.mmProjectPoints.size() > in_view) { fprintf(stderr, "mmProjectPoints holds too much\n"); return 4; }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    std::vector<int32_t> who((size_t)Nf);
    for (int j = 0; j < Nf; ++j) {
        MockMapPoint* p = F.mvpMapPoints[j];
        who[j] = !p ? -1 : (p == &other_observed ? -2 : (p == &other_unobserved ? -3 : (int32_t)(p - mps.data())));
    }
    for (int i = 0; i < Np; ++i) {
        const MockMapPoint& m = mps[i];
        inview[i] = m.mbTrackInView; px[i] = m.mTrackProjX; py[i] = m.mTrackProjY; pxr[i] = m.mTrackProjXR; dep[i] = m.mTrackDepth;
        lev[i] = m.mnTrackScaleLevel; vc[i] = m.mTrackViewCos; vis[i] = m.mnVisible;
    }
    const int32_t head[2] = {ret, nToMatch};
    fwrite(head, 4, 2, fo);
    put(fo, who); put(fo, inview); put(fo, px); put(fo, py); put(fo, pxr); put(fo, dep); put(fo, lev); put(fo, vc); put(fo, vis);
    fclose(fo);
    return 0;
}
