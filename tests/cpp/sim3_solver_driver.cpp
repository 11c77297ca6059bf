// sim3_solver_driver.cpp -- Sim3Solver (reference src/Sim3Solver.cc) through the drop-in of include/rfe/sim3_solver.h on a case read from a
// file, with minimal KeyFrame / MapPoint stand-ins that carry the reference's member names; runs the loop of
// LoopClosing::DetectCommonRegionsFromBoW (while(!bConverge && !bNoMore) iterate(20, ..)) or find() and dumps what came back.
// usage: sim3_solver_driver <case.bin> <out.bin>    (without arguments: compile / link check only, exit 0)
// case.bin: i32 mN1, levels of KF1, levels of KF2, bFixScale, minInliers, maxIterations, mode (0 the loop, 1 find), camera type of KF2,
//               number of draws, pass a vpKeyFrameMatchedMP list (of a third keyframe that holds no point) |
//           f64 probability | f32 Rcw1[9] tcw1[3] Rcw2[9] tcw2[3] | f32 fx fy cx cy of KF1, of KF2 | f32 mvLevelSigma2 of KF1, of KF2 |
//           mN1 x (i32 kind, octave in KF1, octave in KF2, index in KF2; f32 world position of pMP1 [3], of pMP2 [3]) | draws x i32
//           kind: 0 a correspondence; 1 vpMatched12[i] NULL; 2 pKF1 has no map point there; 3 pMP1 bad; 4 pMP2 bad; 5 pMP1 not in pKF1;
//                 6 pMP2 not in pKF2
// out.bin:  i32 status, bConverge, bNoMore, nInliers, calls of iterate, draws taken, mN1, correspondences, iterations, a draw was asked
//               for with other bounds than (0, N - 1 - k) | i32 stats[8] | f32 the returned matrix [16], GetEstimatedTransformation [16],
//               Rotation [9], Translation [3], Scale | mN1 x u8 vbInliers
#include <map>
#include <tuple>
#include "driver_common.h"
#include "rfe/sim3_solver.h"

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
    std::vector<float> mvLevelSigma2;
    std::vector<MockMapPoint*> points;
    std::vector<MockMapPoint*> GetMapPointMatches() const { return points; }
    Mat3 GetRotation() const { return Rcw; }
    Vec3 GetTranslation() const { return tcw; }
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[10]; double prob; float pose[24], cam[8];
    if (fread(hd, 4, 10, fi) != 10 || fread(&prob, 8, 1, fi) != 1 || fread(pose, 4, 24, fi) != 24 || fread(cam, 4, 8, fi) != 8 || hd[0] < 0 ||
        hd[1] < 1 || hd[2] < 1 || hd[8] < 0) return EXIT_BAD_CASE;
    const size_t M = (size_t)hd[0];
    MockKeyFrame K1, K2, K3;
    std::vector<int32_t> draws;
    struct Slot { int32_t kind, oct1, oct2, idx2; float x1[3], x2[3]; };
    std::vector<Slot> slots;
    if (!get(fi, K1.mvLevelSigma2, (size_t)hd[1]) || !get(fi, K2.mvLevelSigma2, (size_t)hd[2]) || !get(fi, slots, M) ||
        !get(fi, draws, (size_t)hd[8])) return short_case();
    fclose(fi);
    for (int k = 0; k < 9; ++k) { K1.Rcw.m[k] = pose[k]; K2.Rcw.m[k] = pose[12 + k]; }
    for (int k = 0; k < 3; ++k) { K1.tcw.v[k] = pose[9 + k]; K2.tcw.v[k] = pose[21 + k]; }
    K1.fx = cam[0]; K1.fy = cam[1]; K1.cx = cam[2]; K1.cy = cam[3]; K2.fx = cam[4]; K2.fy = cam[5]; K2.cx = cam[6]; K2.cy = cam[7];
    K2.cam.type = hd[7];
    K3.mvLevelSigma2 = K2.mvLevelSigma2;
    std::vector<MockMapPoint> p1(M), p2(M);
    std::vector<MockMapPoint*> matched(M, nullptr);
    K1.mvKeysUn.resize(M); K2.mvKeysUn.resize(M); K1.points.assign(M, nullptr);
    for (size_t i = 0; i < M; ++i) {
        const Slot& s = slots[i];
        if (s.idx2 < 0 || (size_t)s.idx2 >= M) return EXIT_BAD_CASE;
        for (int k = 0; k < 3; ++k) { p1[i].pos.v[k] = s.x1[k]; p2[i].pos.v[k] = s.x2[k]; }
        K1.mvKeysUn[i].octave = s.oct1; K2.mvKeysUn[s.idx2].octave = s.oct2;
        if (s.kind != 5) p1[i].index[&K1] = (int)i;
        if (s.kind != 6) p2[i].index[&K2] = s.idx2;
        p1[i].bad = s.kind == 3; p2[i].bad = s.kind == 4;
        K1.points[i] = s.kind == 2 ? nullptr : &p1[i];
        matched[i] = s.kind == 1 ? nullptr : &p2[i];
    }
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    size_t taken = 0; int bad_bounds = 0, expect_hi = -1, k3 = 0;
    auto random_int = [&](int lo, int hi) {
        if (k3 == 0) expect_hi = hi;                                     // the first draw of an iteration tells N - 1
        if (lo != 0 || hi != expect_hi - k3) bad_bounds = 1;
        k3 = (k3 + 1) % 3;
        return taken < draws.size() ? draws[taken++] : (++taken, 0);
    };
    typedef ORB_SLAM3::Sim3Solver_rfe<MockKeyFrame, MockMapPoint> Solver;
    Solver solver(ctx, random_int, &K1, &K2, matched, hd[3] != 0, hd[9] ? std::vector<MockKeyFrame*>(M, &K3) : std::vector<MockKeyFrame*>());
    solver.SetRansacParameters(prob, hd[4], hd[5]);
    bool bNoMore = false, bConverge = false; int nInliers = 0, calls = 0;
    std::vector<bool> vbInliers;
    Solver::Mat4 T;
    if (hd[6] == 0) {
        while (!bConverge && !bNoMore) { T = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge); ++calls; }
    } else {
        T = solver.find(vbInliers, nInliers); calls = 1;
    }
    if (solver.status() < -1) fprintf(stderr, "drop-in: %d %s\n", solver.status(), rfe_last_error(ctx));
    const Solver::Mat4 Tb = solver.GetEstimatedTransformation();
    const Solver::Mat3 Rb = solver.GetEstimatedRotation();
    const Solver::Vec3 tb = solver.GetEstimatedTranslation();
    const float sb = solver.GetEstimatedScale();
    int32_t stats[8];
    for (int k = 0; k < 8; ++k) stats[k] = solver.stats()[k];
    const int32_t head[10] = {solver.status(), bConverge, bNoMore, nInliers, calls, (int32_t)taken, (int32_t)M, solver.correspondences(),
                              solver.iterations(), bad_bounds};
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    fwrite(head, 4, 10, fo); fwrite(stats, 4, 8, fo);
    fwrite(T.data(), 4, 16, fo); fwrite(Tb.data(), 4, 16, fo); fwrite(Rb.data(), 4, 9, fo); fwrite(tb.data(), 4, 3, fo); fwrite(&sb, 4, 1, fo);
    std::vector<uint8_t> o(vbInliers.size());
    for (size_t i = 0; i < o.size(); ++i) o[i] = vbInliers[i] ? 1 : 0;
    put(fo, o);
    fclose(fo);
    return 0;
}
