// essential_graph_driver.cpp -- Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:4509-4840) through the drop-in of
// include/rfe/essential_graph.h on a small map read from a file, with KeyFrame / MapPoint / Map / Sim3 stand-ins that carry the reference's
// member names; dumps the return value and what SetPose / SetWorldPos received, and whether the map's mutex was held, for the Python test.
// usage: essential_graph_driver <case.bin> <out.bin>    (with fewer arguments it exits 0 at once: tests/test_essential_graph_ref.py compiles it)
// case.bin: i32 nKF, nMP, current keyframe, loop keyframe, init keyframe id, fix scale, corrected entries, non-corrected entries, loop
//             connection entries
//           per keyframe: i32 mnId, isBad, parent (-1: none), bImu, previous keyframe (-1: none), loop edges, covisibles, children |
//             f32 pose qx qy qz qw tx ty tz | loop edges x i32 keyframe | covisibles x (i32 keyframe, i32 weight) | children x i32 keyframe
//           per corrected, then per non-corrected entry: i32 keyframe, f64 q xyzw t s
//           per loop connection entry: i32 keyframe, i32 n, n x i32 keyframe
//           per map point: i32 isBad, mnCorrectedByKF, mnCorrectedReference, reference keyframe | f32 position
// out.bin:  i32 return value, change index, calls made without the mutex held | i32 stats[8] |
//           per keyframe: i32 SetPose calls, f32 pose | per map point: i32 SetWorldPos calls, UpdateNormalAndDepth calls, f32 position
#include <map>
#include <set>
#include "driver_common.h"
#include "rfe/essential_graph.h"

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
struct QuatD { double c[4]; double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; } };
struct Vec3D { double v[3]; double operator()(int i) const { return v[i]; } };
struct MockSim3 {                      // g2o::Sim3's three accessors
    QuatD r; Vec3D t; double s;
    QuatD rotation() const { return r; }
    Vec3D translation() const { return t; }
    double scale() const { return s; }
};
struct MockMutex {                     // BasicLockable; remembers whether it is held
    bool held = false;
    void lock() { held = true; }
    void unlock() { held = false; }
};
struct MockKeyFrame;
struct MockMapPoint;
struct MockMap {
    long unsigned int init_id = 0; int change_index = 0, unlocked_calls = 0;
    MockMutex mMutexMapUpdate;
    std::vector<MockKeyFrame*> kfs; std::vector<MockMapPoint*> mps;
    std::vector<MockKeyFrame*> GetAllKeyFrames() const { return kfs; }
    std::vector<MockMapPoint*> GetAllMapPoints() const { return mps; }
    long unsigned int GetInitKFid() const { return init_id; }
    void IncreaseChangeIndex() { ++change_index; if (!mMutexMapUpdate.held) ++unlocked_calls; }
};
struct MockKeyFrame {
    long unsigned int mnId = 0;
    bool bad = false, bImu = false; MockMap* map = nullptr;
    MockKeyFrame *parent = nullptr, *mPrevKF = nullptr;
    std::set<MockKeyFrame*> loop_edges, children;
    std::vector<std::pair<MockKeyFrame*, int>> covisibles;
    QuatSE3 Tcw; int set_pose_calls = 0;
    bool isBad() const { return bad; }
    QuatSE3 GetPose() const { return Tcw; }
    void SetPose(const QuatSE3& T) { Tcw = T; ++set_pose_calls; if (!map->mMutexMapUpdate.held) ++map->unlocked_calls; }
    MockKeyFrame* GetParent() const { return parent; }
    std::set<MockKeyFrame*> GetLoopEdges() const { return loop_edges; }
    bool hasChild(MockKeyFrame* p) const { return children.count(p) != 0; }
    int GetWeight(MockKeyFrame* p) const {
        for (const auto& c : covisibles) if (c.first == p) return c.second;
        return 0;
    }
    std::vector<MockKeyFrame*> GetCovisiblesByWeight(int w) const {
        std::vector<MockKeyFrame*> out;
        for (const auto& c : covisibles) if (c.second >= w) out.push_back(c.first);
        return out;
    }
};
struct MockMapPoint {
    bool bad = false; MockMap* map = nullptr; Vec3 pos;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    MockKeyFrame* ref = nullptr;
    int set_calls = 0, update_calls = 0;
    bool isBad() const { return bad; }
    MockKeyFrame* GetReferenceKeyFrame() const { return ref; }
    Vec3 GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3& p) { pos = p; ++set_calls; if (!map->mMutexMapUpdate.held) ++map->unlocked_calls; }
    void UpdateNormalAndDepth() { ++update_calls; }
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[9];
    if (fread(hd, 4, 9, fi) != 9 || hd[0] < 1 || hd[1] < 0 || hd[2] < 0 || hd[2] >= hd[0] || hd[3] < 0 || hd[3] >= hd[0]) return EXIT_BAD_CASE;
    const int nKF = hd[0], nMP = hd[1];
    MockMap map;
    map.init_id = (long unsigned int)hd[4];
    const bool fix_scale = hd[5] != 0;
    std::vector<MockKeyFrame> kfs(nKF);
    std::vector<MockMapPoint> mps(nMP);
    const auto kf_at = [&](int32_t k) -> MockKeyFrame* { return k >= 0 && k < nKF ? &kfs[k] : nullptr; };
    for (int k = 0; k < nKF; ++k) {
        MockKeyFrame& kf = kfs[k];
        int32_t h[8]; float pose[7];
        if (fread(h, 4, 8, fi) != 8 || h[5] < 0 || h[6] < 0 || h[7] < 0 || fread(pose, 4, 7, fi) != 7) return short_case();
        std::vector<int32_t> le, cv, ch;
        if (!get(fi, le, (size_t)h[5]) || !get(fi, cv, (size_t)h[6] * 2) || !get(fi, ch, (size_t)h[7])) return short_case();
        kf.mnId = (long unsigned int)h[0]; kf.bad = h[1] != 0; kf.parent = kf_at(h[2]); kf.bImu = h[3] != 0; kf.mPrevKF = kf_at(h[4]); kf.map = &map;
        kf.Tcw = QuatSE3(Quat(pose[3], pose[0], pose[1], pose[2]), Vec3(pose[4], pose[5], pose[6]));
        for (int32_t v : le) { if (!kf_at(v)) return EXIT_BAD_CASE; kf.loop_edges.insert(kf_at(v)); }
        for (size_t i = 0; i < cv.size(); i += 2) { if (!kf_at(cv[i])) return EXIT_BAD_CASE; kf.covisibles.push_back(std::make_pair(kf_at(cv[i]), (int)cv[i + 1])); }
        for (int32_t v : ch) { if (!kf_at(v)) return EXIT_BAD_CASE; kf.children.insert(kf_at(v)); }
        map.kfs.push_back(&kf);
    }
    std::map<MockKeyFrame*, MockSim3> corrected, non_corrected;
    for (int pass = 0; pass < 2; ++pass)
        for (int n = 0; n < hd[6 + pass]; ++n) {
            int32_t k; double v[8];
            if (fread(&k, 4, 1, fi) != 1 || fread(v, 8, 8, fi) != 8) return short_case();
            if (!kf_at(k)) return EXIT_BAD_CASE;
            MockSim3 S;
            for (int c = 0; c < 4; ++c) S.r.c[c] = v[c];
            for (int c = 0; c < 3; ++c) S.t.v[c] = v[4 + c];
            S.s = v[7];
            (pass ? non_corrected : corrected)[kf_at(k)] = S;
        }
    std::map<MockKeyFrame*, std::set<MockKeyFrame*>> connections;
    for (int n = 0; n < hd[8]; ++n) {
        int32_t h[2];
        std::vector<int32_t> to;
        if (fread(h, 4, 2, fi) != 2 || h[1] < 0 || !get(fi, to, (size_t)h[1])) return short_case();
        if (!kf_at(h[0])) return EXIT_BAD_CASE;
        for (int32_t v : to) { if (!kf_at(v)) return EXIT_BAD_CASE; connections[kf_at(h[0])].insert(kf_at(v)); }
    }
    for (int p = 0; p < nMP; ++p) {
        MockMapPoint& mp = mps[p];
        int32_t h[4]; float pos[3];
        if (fread(h, 4, 4, fi) != 4 || fread(pos, 4, 3, fi) != 3) return short_case();
        if (!kf_at(h[3])) return EXIT_BAD_CASE;
        mp.bad = h[0] != 0; mp.mnCorrectedByKF = (long unsigned int)h[1]; mp.mnCorrectedReference = (long unsigned int)h[2]; mp.ref = kf_at(h[3]);
        mp.map = &map; mp.pos = Vec3(pos[0], pos[1], pos[2]);
        map.mps.push_back(&mp);
    }
    fclose(fi);
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t ret = ORB_SLAM3::OptimizeEssentialGraph_rfe(ctx, &map, &kfs[hd[3]], &kfs[hd[2]], non_corrected, corrected, connections, fix_scale, stats);
    if (ret < 0 && ret != ORB_SLAM3::RFE_EG_NOT_SERVED) fprintf(stderr, "drop-in: %d %s\n", ret, rfe_last_error(ctx));
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    const int32_t head[3] = {ret, map.change_index, map.unlocked_calls + (map.mMutexMapUpdate.held ? 1000 : 0)};
    fwrite(head, 4, 3, fo);
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
    fclose(fo);
    return 0;
}
