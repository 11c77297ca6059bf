// local_ba_driver.cpp -- Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1740-2188) through the drop-in of include/rfe/local_ba.h
// on a small map read from a file, with KeyFrame / MapPoint / Map stand-ins that carry the reference's member names; dumps the return value,
// the four counters, what SetPose / SetWorldPos received and the erased observations for the Python test.
// usage: local_ba_driver <case.bin> <out.bin>    (with fewer arguments it exits 0 at once: tests/test_local_ba_ref.py compiles it)
// case.bin: i32 nKF, nMP, current keyframe, init keyframe id, inertial, stop flag set, keyframe with a second camera (-1: none), keyframe
//             with a fisheye camera (-1: none), number of covisibles | covisibles x i32 keyframe index
//           per keyframe: i32 mnId, isBad, N, nlevels | f32 pose qx qy qz qw tx ty tz | f32 fx fy cx cy mbf | nlevels x f32 mvInvLevelSigma2 |
//             N x (x, y) f32 mvKeysUn | N x i32 octave | N x f32 mvuRight | N x i32 map point index of mvpMapPoints[i] (-1: none)
//           per map point: i32 mnId, isBad, number of observations | f32 position | observations x (i32 keyframe index, i32 left index)
// out.bin:  i32 return value, num_fixedKF, num_OptKF, num_MPs, num_edges, change index, erased pairs | i32 stats[8] |
//           per keyframe: i32 SetPose calls, f32 pose | per map point: i32 SetWorldPos calls, UpdateNormalAndDepth calls, f32 position |
//           erased pairs x (i32 keyframe index, i32 map point index)
#include <map>
#include <mutex>
#include <set>
#include <tuple>
#include "driver_common.h"
#include "rfe/local_ba.h"

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
struct MockMap {
    long unsigned int init_id = 0; bool inertial = false; int change_index = 0;
    std::mutex mMutexMapUpdate;
    std::set<long unsigned int> msOptKFs, msFixedKFs;
    long unsigned int GetInitKFid() const { return init_id; }
    bool IsInertial() const { return inertial; }
    void IncreaseChangeIndex() { ++change_index; }
};
struct MockKeyFrame;
struct MockMapPoint {
    long unsigned int mnId = 0, mnBALocalForKF = ~0ul;
    bool bad = false; MockMap* map = nullptr; Vec3 pos;
    std::map<MockKeyFrame*, std::tuple<int, int>> obs;
    int set_calls = 0, update_calls = 0, index = 0;
    std::vector<std::pair<int, int>>* erased = nullptr;
    bool isBad() const { return bad; }
    MockMap* GetMap() const { return map; }
    std::map<MockKeyFrame*, std::tuple<int, int>> GetObservations() const { return obs; }
    Vec3 GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3& p) { pos = p; ++set_calls; }
    void UpdateNormalAndDepth() { ++update_calls; }
    void EraseObservation(MockKeyFrame* pKF) { obs.erase(pKF); }
};
struct MockKeyFrame {
    long unsigned int mnId = 0, mnBALocalForKF = ~0ul, mnBAFixedForKF = ~0ul;
    bool bad = false; MockMap* map = nullptr; int index = 0;
    std::vector<MockKeyFrame*> covisibles;
    std::vector<MockMapPoint*> mvpMapPoints;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    MockCamera cam, cam2; MockCamera* mpCamera = &cam; MockCamera* mpCamera2 = nullptr;
    QuatSE3 Tcw; int set_pose_calls = 0;
    std::vector<std::pair<int, int>>* erased = nullptr;
    bool isBad() const { return bad; }
    MockMap* GetMap() const { return map; }
    std::vector<MockKeyFrame*> GetVectorCovisibleKeyFrames() const { return covisibles; }
    std::vector<MockMapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    QuatSE3 GetPose() const { return Tcw; }
    void SetPose(const QuatSE3& T) { Tcw = T; ++set_pose_calls; }
    void EraseMapPointMatch(MockMapPoint* pMP) {
        for (auto& p : mvpMapPoints) if (p == pMP) p = nullptr;
        erased->push_back(std::make_pair(index, pMP->index));
    }
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[9];
    if (fread(hd, 4, 9, fi) != 9 || hd[0] < 1 || hd[1] < 0 || hd[2] < 0 || hd[2] >= hd[0] || hd[8] < 0) return EXIT_BAD_CASE;
    const int nKF = hd[0], nMP = hd[1];
    std::vector<int32_t> cov;
    if (!get(fi, cov, (size_t)hd[8])) return short_case();
    MockMap map;
    map.init_id = (long unsigned int)hd[3]; map.inertial = hd[4] != 0;
    bool stop = hd[5] != 0;
    std::vector<std::pair<int, int>> erased;
    std::vector<MockKeyFrame> kfs(nKF);
    std::vector<MockMapPoint> mps(nMP);
    std::vector<std::vector<int32_t>> kf_mp(nKF);
    for (int k = 0; k < nKF; ++k) {
        MockKeyFrame& kf = kfs[k];
        int32_t h[4]; float pose[7], cam[5];
        if (fread(h, 4, 4, fi) != 4 || h[2] < 0 || h[3] < 0 || fread(pose, 4, 7, fi) != 7 || fread(cam, 4, 5, fi) != 5) return short_case();
        const size_t N = (size_t)h[2];
        std::vector<float> kp; std::vector<int32_t> oct;
        if (!get(fi, kf.mvInvLevelSigma2, (size_t)h[3]) || !get(fi, kp, N * 2) || !get(fi, oct, N) || !get(fi, kf.mvuRight, N) || !get(fi, kf_mp[k], N))
            return short_case();
        kf.mnId = (long unsigned int)h[0]; kf.bad = h[1] != 0; kf.map = &map; kf.index = k; kf.erased = &erased;
        kf.Tcw = QuatSE3(Quat(pose[3], pose[0], pose[1], pose[2]), Vec3(pose[4], pose[5], pose[6]));
        kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3]; kf.mbf = cam[4];
        kf.mvKeysUn.resize(N);
        for (size_t i = 0; i < N; ++i) { kf.mvKeysUn[i].pt = cv::Point2f(kp[2 * i], kp[2 * i + 1]); kf.mvKeysUn[i].octave = oct[i]; }
        if (hd[6] == k) kf.mpCamera2 = &kf.cam2;
        if (hd[7] == k) kf.cam.type = 1;             // GeometricCamera::CAM_FISHEYE
    }
    for (int p = 0; p < nMP; ++p) {
        MockMapPoint& mp = mps[p];
        int32_t h[3]; float pos[3];
        if (fread(h, 4, 3, fi) != 3 || h[2] < 0 || fread(pos, 4, 3, fi) != 3) return short_case();
        std::vector<int32_t> ob;
        if (!get(fi, ob, (size_t)h[2] * 2)) return short_case();
        mp.mnId = (long unsigned int)h[0]; mp.bad = h[1] != 0; mp.map = &map; mp.index = p; mp.pos = Vec3(pos[0], pos[1], pos[2]);
        for (int i = 0; i < h[2]; ++i) {
            if (ob[2 * i] < 0 || ob[2 * i] >= nKF) return EXIT_BAD_CASE;
            mp.obs[&kfs[ob[2 * i]]] = std::make_tuple((int)ob[2 * i + 1], -1);
        }
    }
    fclose(fi);
    for (int k = 0; k < nKF; ++k)
        for (int32_t m : kf_mp[k]) {
            if (m >= nMP) return EXIT_BAD_CASE;
            kfs[k].mvpMapPoints.push_back(m < 0 ? nullptr : &mps[m]);
        }
    for (int32_t k : cov) {
        if (k < 0 || k >= nKF) return EXIT_BAD_CASE;
        kfs[hd[2]].covisibles.push_back(&kfs[k]);
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    int nf = -7, no = -7, nm = -7, ne = -7;
    int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t ret = ORB_SLAM3::LocalBundleAdjustment_rfe(ctx, &kfs[hd[2]], &stop, &map, nf, no, nm, ne, stats);
    if (ret < 0 && ret > ORB_SLAM3::RFE_LBA_NO_FIXED_KF) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    const int32_t head[7] = {ret, nf, no, nm, ne, map.change_index, (int32_t)erased.size()};
    fwrite(head, 4, 7, fo);
    fwrite(stats, 4, 8, fo);
    for (const MockKeyFrame& kf : kfs) {
        const int32_t c = kf.set_pose_calls;
        const float p[7] = {kf.Tcw.q.x(), kf.Tcw.q.y(), kf.Tcw.q.z(), kf.Tcw.q.w(), kf.Tcw.t(0), kf.Tcw.t(1), kf.Tcw.t(2)};
        fwrite(&c, 4, 1, fo); fwrite(p, 4, 7, fo);
    }
    for (const MockMapPoint& mp : mps) {
        const int32_t c[2] = {mp.set_calls, mp.update_calls};
        const float p[3] = {mp.pos(0), mp.pos(1), mp.pos(2)};
        fwrite(c, 4, 2, fo); fwrite(p, 4, 3, fo);
    }
    for (const auto& e : erased) { const int32_t v[2] = {e.first, e.second}; fwrite(v, 4, 2, fo); }
    fclose(fo);
    return 0;
}
