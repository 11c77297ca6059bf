// global_ba_driver.cpp -- Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (reference src/Optimizer.cc:2813-3220) through the drop-ins of
// include/rfe/global_ba.h on a small map read from a file, with KeyFrame / MapPoint / Map stand-ins that carry the reference's member
// names; dumps the return value, stats and what SetPose / SetWorldPos / mTcwGBA / mPosGBA / mnBAGlobalForKF received for the Python test.
// usage: global_ba_driver <case.bin> <out.bin>    (with fewer arguments it exits 0 at once: tests/test_global_ba_ref.py compiles it)
// case.bin: i32 nKF, nMP, init keyframe id, origin keyframe id, nLoopKF, bRobust, nIterations, keyframe with a second camera (-1: none),
//             keyframe with a fisheye camera (-1: none), through the map (GlobalBundleAdjustemnt_rfe) or the vectors (BundleAdjustment_rfe)
//           per keyframe: i32 mnId, state (0 good, 1 isBad, 2 good but not in the map's vectors: a late keyframe), N, nlevels |
//             f32 pose qx qy qz qw tx ty tz | f32 fx fy cx cy mbf | nlevels x f32 mvInvLevelSigma2 |
//             N x (x, y) f32 mvKeysUn | N x i32 octave | N x f32 mvuRight
//           per map point: i32 mnId, isBad, number of observations | f32 position | observations x (i32 keyframe index, i32 left index)
// out.bin:  i32 return value | i32 stats[8] | per keyframe: i32 SetPose calls, mnBAGlobalForKF (-1: never written), f32 pose, f32 mTcwGBA |
//           per map point: i32 SetWorldPos calls, UpdateNormalAndDepth calls, mnBAGlobalForKF (-1), f32 position, f32 mPosGBA
#include <map>
#include <tuple>
#include "driver_common.h"
#include "rfe/global_ba.h"

struct Quat {
    float qx, qy, qz, qw;
    Quat() : qx(0), qy(0), qz(0), qw(1) {}
    Quat(float w, float x, float y, float z) : qx(x), qy(y), qz(z), qw(w) {}      // Eigen's order
    float x() const { return qx; }
    float y() const { return qy; }
    float z() const { return qz; }
    float w() const { return qw; }
};
struct QuatSE3 {
    Quat q; Vec3 t;
    QuatSE3() {}
    QuatSE3(const Quat& q_, const Vec3& t_) : q(q_), t(t_) {}
    Quat unit_quaternion() const { return q; }
    Vec3 translation() const { return t; }
};
struct MockKeyFrame;
struct MockMapPoint;
struct MockMap {
    long unsigned int init_id = 0;
    MockKeyFrame* origin = nullptr;
    std::vector<MockKeyFrame*> kfs;
    std::vector<MockMapPoint*> mps;
    long unsigned int GetInitKFid() const { return init_id; }
    MockKeyFrame* GetOriginKF() const { return origin; }
    std::vector<MockKeyFrame*> GetAllKeyFrames() const { return kfs; }
    std::vector<MockMapPoint*> GetAllMapPoints() const { return mps; }
};
struct MockMapPoint {
    long unsigned int mnId = 0, mnBAGlobalForKF = ~0ul;
    bool bad = false; Vec3 pos, mPosGBA;
    std::map<MockKeyFrame*, std::tuple<int, int>> obs;
    int set_calls = 0, update_calls = 0;
    bool isBad() const { return bad; }
    std::map<MockKeyFrame*, std::tuple<int, int>> GetObservations() const { return obs; }
    Vec3 GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3& p) { pos = p; ++set_calls; }
    void UpdateNormalAndDepth() { ++update_calls; }
};
struct MockKeyFrame {
    long unsigned int mnId = 0, mnBAGlobalForKF = ~0ul;
    bool bad = false; MockMap* map = nullptr;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    MockCamera cam, cam2; MockCamera* mpCamera = &cam; MockCamera* mpCamera2 = nullptr;
    QuatSE3 Tcw, mTcwGBA; int set_pose_calls = 0;
    bool isBad() const { return bad; }
    MockMap* GetMap() const { return map; }
    QuatSE3 GetPose() const { return Tcw; }
    void SetPose(const QuatSE3& T) { Tcw = T; ++set_pose_calls; }
};

static void put_pose(FILE* fo, const QuatSE3& T) {
    const float p[7] = {T.q.x(), T.q.y(), T.q.z(), T.q.w(), T.t(0), T.t(1), T.t(2)};
    fwrite(p, 4, 7, fo);
}

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[10];
    if (fread(hd, 4, 10, fi) != 10 || hd[0] < 1 || hd[1] < 0) return EXIT_BAD_CASE;
    const int nKF = hd[0], nMP = hd[1];
    MockMap map;
    map.init_id = (long unsigned int)hd[2];
    std::vector<MockKeyFrame> kfs(nKF);
    std::vector<MockMapPoint> mps(nMP);
    for (int k = 0; k < nKF; ++k) {
        MockKeyFrame& kf = kfs[k];
        int32_t h[4]; float pose[7], cam[5];
        if (fread(h, 4, 4, fi) != 4 || h[2] < 0 || h[3] < 0 || fread(pose, 4, 7, fi) != 7 || fread(cam, 4, 5, fi) != 5) return short_case();
        const size_t N = (size_t)h[2];
        std::vector<float> kp; std::vector<int32_t> oct;
        if (!get(fi, kf.mvInvLevelSigma2, (size_t)h[3]) || !get(fi, kp, N * 2) || !get(fi, oct, N) || !get(fi, kf.mvuRight, N)) return short_case();
        kf.mnId = (long unsigned int)h[0]; kf.bad = h[1] == 1; kf.map = &map;
        kf.Tcw = QuatSE3(Quat(pose[3], pose[0], pose[1], pose[2]), Vec3(pose[4], pose[5], pose[6]));
        kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.mbf = cam[4];
        kf.mvKeysUn.resize(N);
        for (size_t i = 0; i < N; ++i) { kf.mvKeysUn[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); kf.mvKeysUn[i].octave = oct[i]; }
        if (hd[7] == k) kf.mpCamera2 = &kf.cam2;
        if (hd[8] == k) kf.cam.type = 1;             // GeometricCamera::CAM_FISHEYE
        if ((long unsigned int)hd[3] == kf.mnId) map.origin = &kf;
        if (h[1] != 2) map.kfs.push_back(&kf);
    }
    if (!map.origin) return EXIT_BAD_CASE;
    for (int p = 0; p < nMP; ++p) {
        MockMapPoint& mp = mps[p];
        int32_t h[3]; float pos[3];
        if (fread(h, 4, 3, fi) != 3 || h[2] < 0 || fread(pos, 4, 3, fi) != 3) return short_case();
        std::vector<int32_t> ob;
        if (!get(fi, ob, (size_t)h[2] * 2)) return short_case();
        mp.mnId = (long unsigned int)h[0]; mp.bad = h[1] != 0; mp.pos = Vec3(pos[0], pos[1], pos[2]);
        for (int i = 0; i < h[2]; ++i) {
            if (ob[2 * i] < 0 || ob[2 * i] >= nKF) return EXIT_BAD_CASE;
            mp.obs[&kfs[ob[2 * i]]] = std::make_tuple((int)ob[2 * i + 1], -1);
        }
        map.mps.push_back(&mp);
    }
    fclose(fi);
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool stop = false;
    const int32_t ret = hd[9] ? ORB_SLAM3::GlobalBundleAdjustemnt_rfe(ctx, &map, hd[6], &stop, (unsigned long)hd[4], hd[5] != 0, stats)
                              : ORB_SLAM3::BundleAdjustment_rfe(ctx, map.kfs, map.mps, hd[6], &stop, (unsigned long)hd[4], hd[5] != 0, stats);
    if (ret < 0 && ret != ORB_SLAM3::RFE_GBA_NOT_SERVED) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    fwrite(&ret, 4, 1, fo);
    fwrite(stats, 4, 8, fo);
    for (const MockKeyFrame& kf : kfs) {
        const int32_t c[2] = {kf.set_pose_calls, kf.mnBAGlobalForKF == ~0ul ? -1 : (int32_t)kf.mnBAGlobalForKF};
        fwrite(c, 4, 2, fo);
        put_pose(fo, kf.Tcw);
        put_pose(fo, kf.mTcwGBA);
    }
    for (const MockMapPoint& mp : mps) {
        const int32_t c[3] = {mp.set_calls, mp.update_calls, mp.mnBAGlobalForKF == ~0ul ? -1 : (int32_t)mp.mnBAGlobalForKF};
        const float p[6] = {mp.pos(0), mp.pos(1), mp.pos(2), mp.mPosGBA(0), mp.mPosGBA(1), mp.mPosGBA(2)};
        fwrite(c, 4, 3, fo); fwrite(p, 4, 6, fo);
    }
    fclose(fo);
    return 0;
}
