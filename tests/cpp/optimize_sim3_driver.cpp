// optimize_sim3_driver.cpp -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4195-4494) through the drop-in of
// include/rfe/optimize_sim3.h on a case read from a file, with its own minimal KeyFrame / MapPoint / Sim3 / 7x7 stand-ins that carry the
// reference's member names; dumps what the call left in vpMatches1, g2oS12 and mAcumHessian.
// usage: optimize_sim3_driver <case.bin> <out.bin>    (run with no arguments it only reports that it was built and linked: no device touched)
// case.bin: i32 N (= vpMatches1.size()), N2 (keypoints of KF2), levels of KF1, levels of KF2, bFixScale, bAllPoints, camera type of KF2 |
//           f32 th2 | f64 g2oS12 as qx qy qz qw tx ty tz s | f32 Rcw1[9] tcw1[3] Rcw2[9] tcw2[3] | f32 fx fy cx cy of KF1, of KF2 |
//           f32 mvInvLevelSigma2 of KF1, of KF2 | N x (i32 kind, octave in KF1, index in KF2; f32 mvKeysUn[i].pt of KF1 [2], world position
//           of pMP1 [3], of pMP2 [3]) | N2 x (f32 mvKeysUn[j].pt of KF2 [2]; i32 octave)
//           kind: 0 both map points good; 1 vpMatches1[i] NULL; 2 pKF1 has no map point there; 3 pMP1 bad; 4 pMP2 bad
// out.bin:  i32 return value, mAcumHessian all zero after the call (it goes in filled with ones), N | i32 stats[8] | f64 g2oS12 [8] |
//           N x u8 vpMatches1[i] != NULL
#include <map>
#include <tuple>
#include "driver_common.h"
#include "rfe/optimize_sim3.h"

struct MockKeyFrame;
struct MockMapPoint {
    Vec3 pos; bool bad = false;
    std::map<const MockKeyFrame*, int> index;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return pos; }
    std::tuple<int, int> GetIndexInKeyFrame(const MockKeyFrame* kf) const {
        const auto it = index.find(kf);
        return it == index.end() ? std::make_tuple(-1, -1) : std::make_tuple(it->second, -1);
    }
};
struct MockKeyFrame {
    Mat3 Rcw; Vec3 tcw;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    MockCamera cam; MockCamera* mpCamera = &cam;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MockMapPoint*> points;
    std::vector<MockMapPoint*> GetMapPointMatches() const { return points; }
    Mat3 GetRotation() const { return Rcw; }
    Vec3 GetTranslation() const { return tcw; }
};
struct MockQuat {                       // Eigen::Quaterniond: constructed as (w, x, y, z)
    double c[4];
    MockQuat(double w, double x, double y, double z) : c{x, y, z, w} {}
    double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
};
struct MockVec3d {
    double v[3];
    MockVec3d(double x, double y, double z) : v{x, y, z} {}
    double operator()(int i) const { return v[i]; }
};
struct MockSim3 {                       // g2o::Sim3
    MockQuat r; MockVec3d t; double s;
    MockSim3(const MockQuat& r_, const MockVec3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    const MockQuat& rotation() const { return r; }
    const MockVec3d& translation() const { return t; }
    const double& scale() const { return s; }
};
struct MockMat77 {
    double m[49];
    void setZero() { for (double& v : m) v = 0.0; }
};

int main(int argc, char** argv) {
    if (argc < 3) { printf("optimize_sim3_driver: built and linked; no device touched\n"); return 0; }
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[7]; float th2, pose[24], cam[8]; double s0[8];
    if (fread(hd, 4, 7, fi) != 7 || fread(&th2, 4, 1, fi) != 1 || fread(s0, 8, 8, fi) != 8 || fread(pose, 4, 24, fi) != 24 ||
        fread(cam, 4, 8, fi) != 8 || hd[0] < 0 || hd[1] < 0 || hd[2] < 0 || hd[3] < 0) return EXIT_BAD_CASE;
    const size_t N = (size_t)hd[0], N2 = (size_t)hd[1];
    MockKeyFrame K1, K2;
    struct Slot { int32_t kind, oct1, idx2; float kp[2], x1[3], x2[3]; };
    struct Key2 { float kp[2]; int32_t oct; };
    std::vector<Slot> slots;
    std::vector<Key2> keys2;
    if (!get(fi, K1.mvInvLevelSigma2, (size_t)hd[2]) || !get(fi, K2.mvInvLevelSigma2, (size_t)hd[3]) || !get(fi, slots, N) || !get(fi, keys2, N2))
        return short_case();
    fclose(fi);
    for (int k = 0; k < 9; ++k) { K1.Rcw.m[k] = pose[k]; K2.Rcw.m[k] = pose[12 + k]; }
    for (int k = 0; k < 3; ++k) { K1.tcw.v[k] = pose[9 + k]; K2.tcw.v[k] = pose[21 + k]; }
    K1.fx = cam[0]; K1.fy = cam[1]; K1.cx = cam[2]; K1.cy = cam[3]; K2.fx = cam[4]; K2.fy = cam[5]; K2.cx = cam[6]; K2.cy = cam[7];
    K2.cam.type = (unsigned int)hd[6];
    std::vector<MockMapPoint> p1(N), p2(N);
    std::vector<MockMapPoint*> matched(N, nullptr);
    K1.mvKeysUn.resize(N); K2.mvKeysUn.resize(N2); K1.points.assign(N, nullptr);
    for (size_t j = 0; j < N2; ++j) { K2.mvKeysUn[j].pt.x = keys2[j].kp[0]; K2.mvKeysUn[j].pt.y = keys2[j].kp[1]; K2.mvKeysUn[j].octave = keys2[j].oct; }
    for (size_t i = 0; i < N; ++i) {
        const Slot& s = slots[i];
        if (s.idx2 >= (int32_t)N2) return EXIT_BAD_CASE;
        for (int k = 0; k < 3; ++k) { p1[i].pos.v[k] = s.x1[k]; p2[i].pos.v[k] = s.x2[k]; }
        K1.mvKeysUn[i].pt.x = s.kp[0]; K1.mvKeysUn[i].pt.y = s.kp[1]; K1.mvKeysUn[i].octave = s.oct1;
        if (s.idx2 >= 0) p2[i].index[&K2] = s.idx2;
        p1[i].bad = s.kind == 3; p2[i].bad = s.kind == 4;
        K1.points[i] = s.kind == 2 ? nullptr : &p1[i];
        matched[i] = s.kind == 1 ? nullptr : &p2[i];
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    MockSim3 S(MockQuat(s0[3], s0[0], s0[1], s0[2]), MockVec3d(s0[4], s0[5], s0[6]), s0[7]);
    MockMat77 H;
    for (double& v : H.m) v = 1.0;
    int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int ret = ORB_SLAM3::OptimizeSim3_rfe(ctx, &K1, &K2, matched, S, th2, hd[4] != 0, H, hd[5] != 0, stats);
    if (ret < 0 && ret != ORB_SLAM3::RFE_OPTIMIZE_SIM3_NOT_SERVED) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    int32_t zeroed = 1;
    for (double v : H.m) if (v != 0.0) zeroed = 0;
    const int32_t head[3] = {ret, zeroed, (int32_t)N};
    const double s[8] = {S.r.x(), S.r.y(), S.r.z(), S.r.w(), S.t(0), S.t(1), S.t(2), S.s};
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    fwrite(head, 4, 3, fo); fwrite(stats, 4, 8, fo); fwrite(s, 8, 8, fo);
    std::vector<uint8_t> o(N);
    for (size_t i = 0; i < N; ++i) o[i] = matched[i] ? 1 : 0;
    put(fo, o);
    fclose(fo);
    return 0;
}
