// sim3_search_driver.cpp -- LoopClosing's calls of the two Sim3 SPmatcher::SearchByProjection overloads (reference src/LoopClosing.cc:1477,
// :1508, :1774) through the drop-ins SearchByProjectionSim3_rfe (include/rfe/sim3_search.h) on a case read from a file, with minimal
// KeyFrame / MapPoint / Sim3 / SE3 stand-ins that carry the reference's member names; dumps both return values and what vpMatched /
// vpMatchedKF hold afterwards for the Python test.
// usage: sim3_search_driver <case.bin> <out.bin>           (without arguments: compile / link check only, exit 0)
// case.bin: i32 Np, Nf, NLeft, th, nlevels | f32 quat[4] (x, y, z, w), translation[3], scale (the Sim3), fx, fy, cx, cy, mnMinX, mnMinY,
//           mnMaxX, mnMaxY, mfLogScaleFactor, ratioHamming | nlevels x f32 mvScaleFactors | Np x u8 isBad
//           | Nf x i32 prior (-1: vpMatched[j] is NULL, -2: a map point that is not in vpPoints, k >= 0: vpPoints[k])
//           | Np x 3 f32 world position | Np x 3 f32 normal | Np x f32 GetMinDistanceInvariance | Np x f32 GetMaxDistanceInvariance
//           | Np x f32 mfMaxDistance | Np x 256 f32 descriptor
//           | Nf x (x, y) f32 | Nf x 256 f32 descriptor
// out.bin:  per overload (first :1558, then :2076): i32 return value | Nf x i32 vpMatched (index into vpPoints, -1 = NULL, -2 = the other
//           map point) | Nf x i32 vpMatchedKF (index of the keyframe, -1 = NULL; all -1 for the second overload, which has none)
#include "driver_common.h"
#include "rfe/sim3_search.h"

static Vec3 operator/(const Vec3& a, float s) { return Vec3(a(0) / s, a(1) / s, a(2) / s); }      // Scw.translation() / Scw.scale()
struct Quat {
    float qx, qy, qz, qw;
    float x() const { return qx; } float y() const { return qy; } float z() const { return qz; } float w() const { return qw; }
};
struct Rotation { Quat q; };            // what rotationMatrix() hands to the SE3 constructor: here the unit quaternion itself

static Vec3 cross(const Vec3& a, const Vec3& b) {
    return Vec3(a(1) * b(2) - a(2) * b(1), a(2) * b(0) - a(0) * b(2), a(0) * b(1) - a(1) * b(0));
}
static Vec3 rotate(const Quat& q, const Vec3& p) {       // uv = qv x p; uv += uv; p + qw * uv + qv x uv
    const Vec3 qv(q.qx, q.qy, q.qz);
    Vec3 uv = cross(qv, p);
    for (float& c : uv.v) c = c + c;
    const Vec3 w = cross(qv, uv);
    return Vec3((p(0) + q.qw * uv(0)) + w(0), (p(1) + q.qw * uv(1)) + w(1), (p(2) + q.qw * uv(2)) + w(2));
}

struct QuatSE3 {                        // quaternion-backed on purpose: the drop-in reads unit_quaternion() and inverse()
    Quat q; Vec3 t;
    QuatSE3(const Rotation& R, const Vec3& tr) : q(R.q), t(tr) {}
    Quat unit_quaternion() const { return q; }
    Vec3 translation() const { return t; }
    QuatSE3 inverse() const {
        const Quat c{-q.qx, -q.qy, -q.qz, q.qw};
        const Vec3 r = rotate(c, t);
        return QuatSE3(Rotation{c}, Vec3(-r(0), -r(1), -r(2)));
    }
};
struct MiniSim3 {
    Quat q; Vec3 tr; float s;
    Rotation rotationMatrix() const { return Rotation{q}; }
    Vec3 translation() const { return tr; }
    float scale() const { return s; }
};

struct MockMapPoint {                   // members the Sim3 SearchByProjection overloads read (src/Matchers/SPmatcher.cc:1578-1633)
    bool bad = false;
    Vec3 pos, nrm;
    float dmin = 0, dmax = 0, maxd = 0;
    cv::Mat desc;
    bool isBad() const { return bad; }
    Vec3 GetWorldPos() const { return pos; }
    Vec3 GetNormal() const { return nrm; }
    float GetMinDistanceInvariance() const { return dmin; }
    float GetMaxDistanceInvariance() const { return dmax; }
    float GetMaxDistance() const { return maxd; }          // the accessor include/rfe/sim3_search.h asks the reference to add
    cv::Mat GetDescriptor() const { return desc.clone(); }
};

struct MockKeyFrame {
    int NLeft = -1, N = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;     // KeyFrame keeps its bounds as const int (include/KeyFrame.h)
    int mnScaleLevels = 1;
    float mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[5]; float fl[18];
    if (fread(hd, 4, 5, fi) != 5 || fread(fl, 4, 18, fi) != 18) return EXIT_BAD_CASE;
    const int Np = hd[0], Nf = hd[1], th = hd[3], nlevels = hd[4];
    std::vector<float> sf, pw, nr, dmin, dmax, maxd, qd, kp, fd; std::vector<uint8_t> bad; std::vector<int32_t> prior;
    if (!get(fi, sf, nlevels) || !get(fi, bad, Np) || !get(fi, prior, Nf) || !get(fi, pw, (size_t)Np * 3) || !get(fi, nr, (size_t)Np * 3) ||
        !get(fi, dmin, Np) || !get(fi, dmax, Np) || !get(fi, maxd, Np) || !get(fi, qd, (size_t)Np * 256) || !get(fi, kp, (size_t)Nf * 2) ||
        !get(fi, fd, (size_t)Nf * 256)) return short_case();
    fclose(fi);
    MiniSim3 Scw{Quat{fl[0], fl[1], fl[2], fl[3]}, Vec3(fl[4], fl[5], fl[6]), fl[7]};
    const float ratioHamming = fl[17];
    std::vector<MockMapPoint> mps((size_t)Np);
    MockMapPoint other;
    std::vector<MockMapPoint*> vp((size_t)Np);
    std::vector<MockKeyFrame> kfs(7);
    std::vector<MockKeyFrame*> vpKFs((size_t)Np);
    for (int i = 0; i < Np; ++i) {
        MockMapPoint& m = mps[i];
        m.bad = bad[i] != 0; m.dmin = dmin[i]; m.dmax = dmax[i]; m.maxd = maxd[i];
        for (int k = 0; k < 3; ++k) { m.pos.v[k] = pw[3 * (size_t)i + k]; m.nrm.v[k] = nr[3 * (size_t)i + k]; }
        m.desc = cv::Mat(1, 256, CV_32F, qd.data() + (size_t)i * 256);
        vp[i] = &m; vpKFs[i] = &kfs[i % 7];
    }
    MockKeyFrame KF;
    KF.NLeft = hd[2]; KF.N = Nf;
    KF.fx = fl[8]; KF.fy = fl[9]; KF.cx = fl[10]; KF.cy = fl[11];
    KF.mnMinX = (int)fl[12]; KF.mnMinY = (int)fl[13]; KF.mnMaxX = (int)fl[14]; KF.mnMaxY = (int)fl[15];
    KF.mnScaleLevels = nlevels; KF.mfLogScaleFactor = fl[16]; KF.mvScaleFactors = sf;
    KF.mvKeysUn.resize((size_t)Nf);
    KF.mDescriptors = cv::Mat(Nf, 256, CV_32F, fd.data());
    for (int j = 0; j < Nf; ++j) KF.mvKeysUn[j].pt = cv::Point2f(kp[2 * j], kp[2 * j + 1]);
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    for (int overload = 0; overload < 2; ++overload) {
        std::vector<MockMapPoint*> vpMatched((size_t)Nf, nullptr);
        std::vector<MockKeyFrame*> vpMatchedKF((size_t)Nf, nullptr);
        for (int j = 0; j < Nf; ++j) vpMatched[j] = prior[j] == -1 ? nullptr : (prior[j] == -2 ? &other : &mps[prior[j]]);
        const int32_t ret = overload == 0
            ? ORB_SLAM3::SearchByProjectionSim3_rfe<QuatSE3>(ctx, &KF, Scw, vp, vpKFs, vpMatched, vpMatchedKF, th, ratioHamming)
            : ORB_SLAM3::SearchByProjectionSim3_rfe<QuatSE3>(ctx, &KF, Scw, vp, vpMatched, th, ratioHamming);
        std::vector<int32_t> who((size_t)Nf), kf((size_t)Nf);
        for (int j = 0; j < Nf; ++j) {
            who[j] = !vpMatched[j] ? -1 : (vpMatched[j] == &other ? -2 : (int32_t)(vpMatched[j] - mps.data()));
            kf[j] = vpMatchedKF[j] ? (int32_t)(vpMatchedKF[j] - kfs.data()) : -1;
        }
        fwrite(&ret, 4, 1, fo);
        put(fo, who); put(fo, kf);
    }
    fclose(fo);
    rfe_destroy(ctx);
    return 0;
}
