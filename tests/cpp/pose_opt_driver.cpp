// pose_opt_driver.cpp -- Optimizer::PoseOptimization (reference src/Optimizer.cc:55-401) through the drop-in of include/rfe/pose_optimization.h
// on a case read from a file, with minimal Frame / MapPoint / pose stand-ins that carry the reference's member names; dumps the return value,
// the pose handed to SetPose and mvbOutlier for the Python test.
// usage: pose_opt_driver <case.bin> <out.bin>    (without arguments: compile / link check only, exit 0)
// case.bin: i32 N, nlevels, has a second camera | f32 fx, fy, cx, cy, mbf | nlevels x f32 mvInvLevelSigma2 | f32 pose qx qy qz qw tx ty tz |
//           N x (x, y) f32 mvKeysUn | N x i32 octave | N x f32 mvuRight | N x 3 f32 world positions | N x u8 mvpMapPoints[i] != NULL |
//           N x u8 mvbOutlier before the call
// out.bin:  i32 return value, SetPose calls, N | i32 stats[8] | f32 the pose as SetPose received it (the frame's own when it was not called) |
//           N x u8 mvbOutlier
#include "driver_common.h"
#include "rfe/pose_optimization.h"

struct Quat {
    float qx, qy, qz, qw;
    Quat() : qx(0), qy(0), qz(0), qw(1) {}
    Quat(float w, float x, float y, float z) : qx(x), qy(y), qz(z), qw(w) {}      // Eigen's order
    float x() const { return qx; }
    float y() const { return qy; }
    float z() const { return qz; }
    float w() const { return qw; }
};
struct QuatSE3 {                         // keeps what it is given: the test compares the values the drop-in hands over
    Quat q; Vec3 t;
    QuatSE3() {}
    QuatSE3(const Quat& q_, const Vec3& t_) : q(q_), t(t_) {}
    Quat unit_quaternion() const { return q; }
    Vec3 translation() const { return t; }
};
struct MockMapPoint {
    Vec3 pos;
    Vec3 GetWorldPos() const { return pos; }
};
struct MockFrame {                       // the members Optimizer::PoseOptimization reads and writes
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MockMapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    MockCamera rig; MockCamera* mpCamera2 = nullptr;
    QuatSE3 Tcw; int set_pose_calls = 0;
    QuatSE3 GetPose() const { return Tcw; }
    void SetPose(const QuatSE3& T) { Tcw = T; ++set_pose_calls; }
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[3]; float cam[5], pose[7];
    if (fread(hd, 4, 3, fi) != 3 || fread(cam, 4, 5, fi) != 5 || hd[0] < 0 || hd[1] < 0) return EXIT_BAD_CASE;
    const size_t N = (size_t)hd[0];
    MockFrame F;
    std::vector<float> kp, xw; std::vector<int32_t> oct; std::vector<uint8_t> mp, outl;
    if (!get(fi, F.mvInvLevelSigma2, (size_t)hd[1]) || fread(pose, 4, 7, fi) != 7 || !get(fi, kp, N * 2) || !get(fi, oct, N) ||
        !get(fi, F.mvuRight, N) || !get(fi, xw, N * 3) || !get(fi, mp, N) || !get(fi, outl, N)) return short_case();
    fclose(fi);
    F.N = (int)N; F.fx = cam[0]; F.fy = cam[1]; F.cx = cam[2]; F.cy = cam[3]; F.mbf = cam[4];
    F.Tcw = QuatSE3(Quat(pose[3], pose[0], pose[1], pose[2]), Vec3(pose[4], pose[5], pose[6]));
    if (hd[2]) F.mpCamera2 = &F.rig;
    std::vector<MockMapPoint> points(N);
    F.mvKeysUn.resize(N); F.mvpMapPoints.resize(N); F.mvbOutlier.resize(N);
    for (size_t i = 0; i < N; ++i) {
        F.mvKeysUn[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); F.mvKeysUn[i].octave = oct[i];
        points[i].pos = Vec3(xw[3 * i], xw[3 * i + 1], xw[3 * i + 2]);
        F.mvpMapPoints[i] = mp[i] ? &points[i] : nullptr;
        F.mvbOutlier[i] = outl[i] != 0;
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t ret = ORB_SLAM3::PoseOptimization_rfe(ctx, &F, stats);
    if (ret < -1) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    const int32_t head[3] = {ret, F.set_pose_calls, (int32_t)N};
    fwrite(head, 4, 3, fo);
    fwrite(stats, 4, 8, fo);
    const float got[7] = {F.Tcw.q.x(), F.Tcw.q.y(), F.Tcw.q.z(), F.Tcw.q.w(), F.Tcw.t(0), F.Tcw.t(1), F.Tcw.t(2)};
    fwrite(got, 4, 7, fo);
    std::vector<uint8_t> o(N);
    for (size_t i = 0; i < N; ++i) o[i] = F.mvbOutlier[i] ? 1 : 0;
    put(fo, o);
    fclose(fo);
    return 0;
}
