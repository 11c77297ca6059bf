// pose_inertial_driver.cpp -- Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (reference src/Optimizer.cc:416-968, :983-1623)
// through the drop-ins of include/rfe/pose_inertial_optimization.h on a case read from a file, with minimal Frame / KeyFrame / MapPoint /
// preintegration stand-ins that carry the reference's member names; dumps the return value, what SetImuPoseVelocity and mImuBias received,
// mvbOutlier and the stored constraint for the Python test.
// usage: pose_inertial_driver <case.bin> <out.bin>    (no arguments: the build and link check of test_pose_inertial_ref.py, exit 0)
// case.bin: i32 N, nlevels, mode (0 LastKeyFrame, 1 LastFrame), bRecInit, has a second camera, the previous frame has a constraint |
//           f32 fx, fy, cx, cy, mbf | nlevels x f32 mvInvLevelSigma2 | f32 cam [36], state [21], prev_state [21], preint [148], cov_rw [18] as
//           rfe_pose_inertial_optimization takes them | f64 the previous frame's constraint [246] | N x (x, y) f32 mvKeysUn | N x i32 octave |
//           N x f32 mvuRight | N x 3 f32 world positions | N x u8 mvpMapPoints[i] != NULL | N x f32 mTrackDepth | N x u8 mvbOutlier before
// out.bin:  i32 return value, SetImuPoseVelocity calls, N, the previous frame's constraint is gone, the frame holds a constraint |
//           i32 stats[16] | f32 Rwb 9, twb 3, v 3 as SetImuPoseVelocity received them (the frame's own when it was not called) |
//           f32 mImuBias bax bay baz bwx bwy bwz | f64 the frame's constraint [246] (0 without one) | f64 the same through
//           ToConstraintPoseImu (Rwb 9, twb 3, vwb 3, bg 3, ba 3, H 225) | N x u8 mvbOutlier
#include "driver_common.h"
#include "rfe/pose_inertial_optimization.h"

template <int R, int C, class T>
struct MatW {                            // writable with (r, c) and (i), as Eigen's fixed-size matrices are
    T m[R * C];
    MatW() { for (int i = 0; i < R * C; ++i) m[i] = 0; }
    T& operator()(int r, int c) { return m[C * r + c]; }
    T operator()(int r, int c) const { return m[C * r + c]; }
    T& operator()(int i) { return m[i]; }
    T operator()(int i) const { return m[i]; }
};
typedef MatW<3, 3, float> M3f;
typedef MatW<3, 1, float> V3f;
struct SE3w {
    M3f R; V3f t;
    M3f rotationMatrix() const { return R; }
    V3f translation() const { return t; }
};
struct MockBias {
    float bax, bay, baz, bwx, bwy, bwz;
    MockBias() : bax(0), bay(0), baz(0), bwx(0), bwy(0), bwz(0) {}
    MockBias(float ax, float ay, float az, float wx, float wy, float wz) : bax(ax), bay(ay), baz(az), bwx(wx), bwy(wy), bwz(wz) {}
};
struct MockPreintegrated {
    float dT = 0;
    M3f dR, JRg, JVg, JVa, JPg, JPa;
    V3f dV, dP;
    MockBias b;
    MatW<15, 15, float> C;
};
struct MockCalib { SE3w mTcb, mTbc; };
struct MockMapPoint {
    V3f pos; float mTrackDepth = 0;
    V3f GetWorldPos() const { return pos; }
};
struct MockBody {                        // what Frame and KeyFrame share
    M3f Rwb; V3f twb, vel;
    M3f GetImuRotation() const { return Rwb; }
    V3f GetImuPosition() const { return twb; }
    V3f GetVelocity() const { return vel; }
};
struct MockKeyFrame : MockBody {
    V3f bg, ba;
    V3f GetGyroBias() const { return bg; }
    V3f GetAccBias() const { return ba; }
};
struct MockFrame : MockBody {            // the members the two functions read and write
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MockMapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    MockCamera rig; MockCamera* mpCamera2 = nullptr;
    SE3w Tcw; MockCalib mImuCalib; MockBias mImuBias;
    MockPreintegrated *mpImuPreintegrated = nullptr, *mpImuPreintegratedFrame = nullptr;
    MockKeyFrame* mpLastKeyFrame = nullptr; MockFrame* mpPrevFrame = nullptr;
    ORB_SLAM3::PoseImuConstraint_rfe* mpcpi_rfe = nullptr;
    int set_calls = 0;
    SE3w GetPose() const { return Tcw; }
    void SetImuPoseVelocity(const M3f& R, const V3f& t, const V3f& v) { Rwb = R; twb = t; vel = v; ++set_calls; }
    ~MockFrame() { delete mpcpi_rfe; }
};
struct MockConstraint {                  // ConstraintPoseImu's members and constructor, without its clipping
    MatW<3, 3, double> Rwb; MatW<3, 1, double> twb, vwb, bg, ba; MatW<15, 15, double> H;
    MockConstraint(const MatW<3, 3, double>& R, const MatW<3, 1, double>& t, const MatW<3, 1, double>& v, const MatW<3, 1, double>& g,
                   const MatW<3, 1, double>& a, const MatW<15, 15, double>& H_) : Rwb(R), twb(t), vwb(v), bg(g), ba(a), H(H_) {}
};

static void set_se3(SE3w& T, const float* p) { for (int k = 0; k < 9; ++k) T.R.m[k] = p[k]; for (int k = 0; k < 3; ++k) T.t.m[k] = p[9 + k]; }
static void set_body(MockBody& b, const float* p) {
    for (int k = 0; k < 9; ++k) b.Rwb.m[k] = p[k];
    for (int k = 0; k < 3; ++k) { b.twb.m[k] = p[9 + k]; b.vel.m[k] = p[12 + k]; }
}

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[6]; float cam5[5];
    if (fread(hd, 4, 6, fi) != 6 || fread(cam5, 4, 5, fi) != 5 || hd[0] < 0 || hd[1] < 0) return EXIT_BAD_CASE;
    const size_t N = (size_t)hd[0];
    MockFrame F, Fp; MockKeyFrame KF; MockPreintegrated pre_edge, pre_kf;
    std::vector<float> cam, st, pst, pr, cov, kp, xw, depth; std::vector<double> prior; std::vector<int32_t> oct; std::vector<uint8_t> mp, outl;
    if (!get(fi, F.mvInvLevelSigma2, (size_t)hd[1]) || !get(fi, cam, 36) || !get(fi, st, 21) || !get(fi, pst, 21) || !get(fi, pr, 148) ||
        !get(fi, cov, 18) || !get(fi, prior, 246) || !get(fi, kp, N * 2) || !get(fi, oct, N) || !get(fi, F.mvuRight, N) || !get(fi, xw, N * 3) ||
        !get(fi, mp, N) || !get(fi, depth, N) || !get(fi, outl, N)) return short_case();
    fclose(fi);
    F.N = (int)N; F.fx = cam5[0]; F.fy = cam5[1]; F.cx = cam5[2]; F.cy = cam5[3]; F.mbf = cam5[4];
    set_se3(F.Tcw, &cam[0]); set_se3(F.mImuCalib.mTcb, &cam[12]); set_se3(F.mImuCalib.mTbc, &cam[24]);
    set_body(F, &st[0]);
    F.mImuBias = MockBias(st[18], st[19], st[20], st[15], st[16], st[17]);
    set_body(Fp, &pst[0]); set_body(KF, &pst[0]);
    Fp.mImuBias = MockBias(pst[18], pst[19], pst[20], pst[15], pst[16], pst[17]);
    for (int k = 0; k < 3; ++k) { KF.bg.m[k] = pst[15 + k]; KF.ba.m[k] = pst[18 + k]; }
    // the edge's preintegration, and another one that differs from it everywhere but carries the two random-walk blocks: LastKeyFrame reads
    // one object for both, LastFrame the edge from mpImuPreintegratedFrame and the blocks from mpImuPreintegrated
    pre_edge.dT = pr[0];
    for (int k = 0; k < 9; ++k) {
        pre_edge.dR.m[k] = pr[1 + k]; pre_edge.JRg.m[k] = pr[16 + k]; pre_edge.JVg.m[k] = pr[25 + k]; pre_edge.JVa.m[k] = pr[34 + k];
        pre_edge.JPg.m[k] = pr[43 + k]; pre_edge.JPa.m[k] = pr[52 + k];
    }
    for (int k = 0; k < 3; ++k) { pre_edge.dV.m[k] = pr[10 + k]; pre_edge.dP.m[k] = pr[13 + k]; }
    pre_edge.b = MockBias(pr[61], pr[62], pr[63], pr[64], pr[65], pr[66]);
    for (int k = 0; k < 81; ++k) pre_edge.C(k / 9, k % 9) = pr[67 + k];
    pre_kf.dT = 77.f;
    for (int k = 0; k < 9; ++k) { pre_kf.C(9 + k / 3, 9 + k % 3) = cov[k]; pre_kf.C(12 + k / 3, 12 + k % 3) = cov[9 + k]; }
    if (hd[2] == 0) {                    // LastKeyFrame: one preintegration
        for (int k = 0; k < 9; ++k) { pre_edge.C(9 + k / 3, 9 + k % 3) = cov[k]; pre_edge.C(12 + k / 3, 12 + k % 3) = cov[9 + k]; }
        F.mpImuPreintegrated = &pre_edge;
    } else {
        F.mpImuPreintegrated = &pre_kf; F.mpImuPreintegratedFrame = &pre_edge;
    }
    F.mpLastKeyFrame = &KF; F.mpPrevFrame = &Fp;
    if (hd[5]) {
        Fp.mpcpi_rfe = new ORB_SLAM3::PoseImuConstraint_rfe();
        double* d = reinterpret_cast<double*>(Fp.mpcpi_rfe);
        for (int k = 0; k < 246; ++k) d[k] = prior[k];
    }
    if (hd[4]) F.mpCamera2 = &F.rig;
    std::vector<MockMapPoint> points(N);
    F.mvKeysUn.resize(N); F.mvpMapPoints.resize(N); F.mvbOutlier.resize(N);
    for (size_t i = 0; i < N; ++i) {
        F.mvKeysUn[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); F.mvKeysUn[i].octave = oct[i];
        for (int k = 0; k < 3; ++k) points[i].pos.m[k] = xw[3 * i + k];
        points[i].mTrackDepth = depth[i];
        F.mvpMapPoints[i] = mp[i] ? &points[i] : nullptr;
        F.mvbOutlier[i] = outl[i] != 0;
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    int32_t stats[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t ret = hd[2] == 0 ? ORB_SLAM3::PoseInertialOptimizationLastKeyFrame_rfe(ctx, &F, hd[3] != 0, stats)
                                   : ORB_SLAM3::PoseInertialOptimizationLastFrame_rfe(ctx, &F, hd[3] != 0, stats);
    if (ret < -1) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    const int32_t head[5] = {ret, F.set_calls, (int32_t)N, Fp.mpcpi_rfe == nullptr ? 1 : 0, F.mpcpi_rfe != nullptr ? 1 : 0};
    fwrite(head, 4, 5, fo);
    fwrite(stats, 4, 16, fo);
    fwrite(F.Rwb.m, 4, 9, fo); fwrite(F.twb.m, 4, 3, fo); fwrite(F.vel.m, 4, 3, fo);
    const float bias[6] = {F.mImuBias.bax, F.mImuBias.bay, F.mImuBias.baz, F.mImuBias.bwx, F.mImuBias.bwy, F.mImuBias.bwz};
    fwrite(bias, 4, 6, fo);
    std::vector<double> stored(246, 0.0), conv(246, 0.0);
    if (F.mpcpi_rfe) {
        const double* d = reinterpret_cast<const double*>(F.mpcpi_rfe);
        for (int k = 0; k < 246; ++k) stored[k] = d[k];
        MockConstraint* c = ORB_SLAM3::ToConstraintPoseImu<MockConstraint>(*F.mpcpi_rfe);
        for (int k = 0; k < 9; ++k) conv[k] = c->Rwb.m[k];
        for (int k = 0; k < 3; ++k) { conv[9 + k] = c->twb.m[k]; conv[12 + k] = c->vwb.m[k]; conv[15 + k] = c->bg.m[k]; conv[18 + k] = c->ba.m[k]; }
        for (int k = 0; k < 225; ++k) conv[21 + k] = c->H.m[k];
        delete c;
    }
    put(fo, stored); put(fo, conv);
    std::vector<uint8_t> o(N);
    for (size_t i = 0; i < N; ++i) o[i] = F.mvbOutlier[i] ? 1 : 0;
    put(fo, o);
    fclose(fo);
    return 0;
}
