// rfe/triangulation.h -- drop-in body for LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:545-954) up to `new MapPoint`: the
// baseline test of every neighbour, SPmatcher::SearchForTriangulation (src/Matchers/SPmatcher.cc:1355-1399: one LightGlue match per
// neighbour plus the map-point filter) and the geometry loop, on top of rfe_match_dev and rfe_triangulate_neighbours_dev.
// The matches of ALL neighbours come from one rfe_match_dev with P = Nn and never leave the device; what comes back is the list of new
// points in the reference's creation order.  The caller keeps :921-942 (new MapPoint, AddObservation, AddMapPoint, ...) per list entry.
// Works on any KeyFrame-like class with the reference's member names:
//   NLeft, mpCamera->GetType(), mpCamera2, GetPose() (rotationMatrix() indexable with (r, c), translation() with (i)), GetCameraCenter()
//   (indexable with (i)), fx, fy, cx, cy, invfx, invfy, mb, mbf, mfScaleFactor, mnScaleLevels, mvScaleFactors, mvLevelSigma2, mvKeys,
//   mvKeysUn, mvuRight, mvDepth, mDescriptors (N x 256 CV_32F), GetMapPoint(i), ComputeSceneMedianDepth(2).
// One pinhole camera per keyframe: a two-camera rig (NLeft != -1 or mpCamera2) or a KannalaBrandt8 camera is refused with -1 and nothing is
// computed -- such a caller keeps the reference's loop.  The scale pyramid (mvScaleFactors, mvLevelSigma2) is the current keyframe's: all
// keyframes of a map come from one extractor.  The neighbours must be distinct keyframes, at most 64 of them: the reference's early return
// between neighbours (`if (i > 0 && CheckNewKeyFrames()) return;`, :583) becomes "pass fewer neighbours".
// `ctx` can be the session of the matcher; it needs LightGlue weights for CreateNewMapPoints_rfe, none for TriangulateMatches_rfe.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "dropin_detail.h"

namespace ORB_SLAM3 {

struct NewMapPoint_rfe {
    int neighbour, idx1, idx2;     // vpNeighKFs[neighbour], index in the current keyframe, index in the neighbour
    float x3D[3];
    bool bPointStereo;
};
struct CreateNewMapPointsParams_rfe {
    bool bMonocular = true;        // mbMonocular: the baseline test uses the scene's median depth instead of mb
    bool bInertial = false;        // mbInertial
    bool bFarPoints = false;       // mbFarPoints
    float thFarPoints = 0.f;       // mThFarPoints
    float filter_thr = 0.1f;       // LightGlue's in-graph match filter
    bool keep_matches = false;     // also copy S / pairs back (tests; costs the download this header exists to avoid)
};
struct CreateNewMapPointsOut_rfe {
    std::vector<NewMapPoint_rfe> points;   // creation order: neighbour ascending, then idx1 ascending
    float matchsum = 0.f;                  // the reference's matchsum: LightGlue matches of the neighbours that pass the baseline test
    std::vector<int32_t> matches;          // per neighbour
    int32_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // as rfe_triangulate_neighbours
    int Kmax = 0;
    std::vector<int32_t> S, pairs;         // keep_matches
};

namespace rfe_tri_detail {
template <class KeyFrameT>
inline bool one_pinhole(KeyFrameT* kf) { return kf->NLeft == -1 && !kf->mpCamera2 && kf->mpCamera->GetType() == 0 /*GeometricCamera::CAM_PINHOLE*/; }
template <class KeyFrameT>
inline void fill_view(KeyFrameT* kf, rfe_tri_view& v) {
    const auto Tcw = kf->GetPose();
    rfe_detail::copy_rotation(Tcw.rotationMatrix(), v.rcw); rfe_detail::copy_vec3(Tcw.translation(), v.tcw); rfe_detail::copy_vec3(kf->GetCameraCenter(), v.ow);
    v.fx = kf->fx; v.fy = kf->fy; v.cx = kf->cx; v.cy = kf->cy; v.invfx = kf->invfx; v.invfy = kf->invfy; v.mb = kf->mb; v.mbf = kf->mbf;
}
// one device allocation, carved in 256-byte steps
struct DevBlock {
    rfe_ctx* ctx; char* base = nullptr; size_t off = 0;
    explicit DevBlock(rfe_ctx* c) : ctx(c) {}
    ~DevBlock() { if (base) rfe_free(ctx, base); }
    template <class T> size_t reserve(size_t n) { const size_t o = off; off += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255; return o; }
    template <class T> T* at(size_t o) const { return (T*)(base + o); }
};
}  // namespace rfe_tri_detail

// The filter and the geometry loop over matches that are on the device already: S_dev [Nn], pairs_dev [Nn,Kmax,2] as rfe_match_dev wrote
// them for the pairs (pKF1, vpNeighKFs[n]).  Returns the number of new points (>= 0), -1 for a refused keyframe, a negative rfe_status when
// the library refuses or fails.
template <class KeyFrameT>
int TriangulateMatches_rfe(rfe_ctx* ctx, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, const CreateNewMapPointsParams_rfe& prm,
                           const int32_t* S_dev, const int32_t* pairs_dev, int Kmax, CreateNewMapPointsOut_rfe& out) {
    using namespace rfe_tri_detail;
    out = CreateNewMapPointsOut_rfe();
    out.Kmax = Kmax;
    const int Nn = (int)vpNeighKFs.size(), N1 = (int)pKF1->mvKeysUn.size();
    if (!one_pinhole(pKF1)) return -1;
    for (KeyFrameT* kf : vpNeighKFs) if (!one_pinhole(kf)) return -1;
    if (Nn == 0) return 0;
    if (Nn > 64 || (int)pKF1->mvScaleFactors.size() < pKF1->mnScaleLevels || (int)pKF1->mvLevelSigma2.size() < pKF1->mnScaleLevels) return RFE_ERR_INVALID;
    rfe_tri_params P = rfe_tri_params();
    P.inertial = prm.bInertial ? 1 : 0; P.far_points = prm.bFarPoints ? 1 : 0; P.th_far = prm.thFarPoints;
    P.ratio_factor = 1.5f * pKF1->mfScaleFactor;                       // :566
    P.nlevels = pKF1->mnScaleLevels;
    rfe_detail::copy_levels(pKF1->mvScaleFactors, P.nlevels, P.scale_factors); rfe_detail::copy_levels(pKF1->mvLevelSigma2, P.nlevels, P.level_sigma2);
    rfe_tri_view v1;
    fill_view(pKF1, v1);
    int N2max = 0;
    for (KeyFrameT* kf : vpNeighKFs) N2max = std::max(N2max, (int)kf->mvKeysUn.size());
    const size_t n1 = (size_t)N1, f2 = (size_t)Nn * N2max;
    std::vector<float> k1(n1 * 2), r1(n1 * 2), u1(n1), d1(n1), k2(f2 * 2), r2(f2 * 2), u2(f2, -1.f), d2(f2, -1.f);
    std::vector<int32_t> o1(n1), o2(f2), n2((size_t)Nn);
    std::vector<uint8_t> m1(n1), m2(f2), valid((size_t)Nn);
    std::vector<rfe_tri_view> v2((size_t)Nn);
    rfe_detail::gather_keypoints(pKF1->mvKeysUn, n1, k1.data(), o1.data());
    rfe_detail::gather_keypoints(pKF1->mvKeys, n1, r1.data());
    for (int i = 0; i < N1; ++i) { u1[i] = pKF1->mvuRight[i]; d1[i] = pKF1->mvDepth[i]; m1[i] = pKF1->GetMapPoint(i) != nullptr; }
    for (int n = 0; n < Nn; ++n) {
        KeyFrameT* kf = vpNeighKFs[n];
        fill_view(kf, v2[n]);
        // the baseline test, :593-620
        const float bx = v2[n].ow[0] - v1.ow[0], by = v2[n].ow[1] - v1.ow[1], bz = v2[n].ow[2] - v1.ow[2];
        const float baseline = std::sqrt((bx * bx + by * by) + bz * bz);
        if (!prm.bMonocular) valid[n] = !(baseline < kf->mb);
        else {
            const float medianDepthKF2 = kf->ComputeSceneMedianDepth(2);
            const float ratioBaselineDepth = baseline / medianDepthKF2;
            valid[n] = !(ratioBaselineDepth < 0.01);
        }
        const int cnt = (int)kf->mvKeysUn.size();
        n2[n] = cnt;
        const size_t b = (size_t)n * N2max;
        rfe_detail::gather_keypoints(kf->mvKeysUn, (size_t)cnt, k2.data() + 2 * b, o2.data() + b);
        rfe_detail::gather_keypoints(kf->mvKeys, (size_t)cnt, r2.data() + 2 * b);
        for (int j = 0; j < cnt; ++j) { u2[b + j] = kf->mvuRight[j]; d2[b + j] = kf->mvDepth[j]; m2[b + j] = kf->GetMapPoint(j) != nullptr; }
    }
    DevBlock D(ctx);
    const size_t ok1 = D.reserve<float>(n1 * 2), or1 = D.reserve<float>(n1 * 2), oo1 = D.reserve<int32_t>(n1), ou1 = D.reserve<float>(n1),
                 od1 = D.reserve<float>(n1), om1 = D.reserve<uint8_t>(n1), ov2 = D.reserve<rfe_tri_view>(Nn), ok2 = D.reserve<float>(f2 * 2),
                 or2 = D.reserve<float>(f2 * 2), oo2 = D.reserve<int32_t>(f2), ou2 = D.reserve<float>(f2), od2 = D.reserve<float>(f2),
                 om2 = D.reserve<uint8_t>(f2), on2 = D.reserve<int32_t>(Nn), onv = D.reserve<uint8_t>(Nn);
    const size_t in_bytes = D.off;
    // the outputs, back to back: one download
    const size_t ost = D.reserve<int32_t>(8), omt = D.reserve<int32_t>(Nn), oon = D.reserve<int32_t>(n1), oi1 = D.reserve<int32_t>(n1),
                 oi2 = D.reserve<int32_t>(n1), ox = D.reserve<float>(n1 * 3), os = D.reserve<uint8_t>(n1);
    int rc = rfe_malloc(ctx, D.off, (void**)&D.base);
    if (rc) return rc;
    std::vector<char> stage(in_bytes);
    auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::copy((const char*)src, (const char*)src + bytes, stage.begin() + o); };
    put(ok1, k1.data(), n1 * 8); put(or1, r1.data(), n1 * 8); put(oo1, o1.data(), n1 * 4); put(ou1, u1.data(), n1 * 4); put(od1, d1.data(), n1 * 4);
    put(om1, m1.data(), n1); put(ov2, v2.data(), (size_t)Nn * sizeof(rfe_tri_view)); put(ok2, k2.data(), f2 * 8); put(or2, r2.data(), f2 * 8);
    put(oo2, o2.data(), f2 * 4); put(ou2, u2.data(), f2 * 4); put(od2, d2.data(), f2 * 4); put(om2, m2.data(), f2); put(on2, n2.data(), (size_t)Nn * 4);
    put(onv, valid.data(), (size_t)Nn);
    if ((rc = rfe_memcpy_h2d(ctx, D.base, stage.data(), in_bytes))) return rc;
    rc = rfe_triangulate_neighbours_dev(ctx, &P, &v1, D.at<float>(ok1), D.at<float>(or1), D.at<int32_t>(oo1), D.at<float>(ou1), D.at<float>(od1),
                                        D.at<uint8_t>(om1), N1, D.at<rfe_tri_view>(ov2), D.at<float>(ok2), D.at<float>(or2), D.at<int32_t>(oo2),
                                        D.at<float>(ou2), D.at<float>(od2), D.at<uint8_t>(om2), D.at<int32_t>(on2), D.at<uint8_t>(onv), Nn, N2max,
                                        S_dev, pairs_dev, Kmax, nullptr, nullptr, nullptr, D.at<int32_t>(oon), D.at<int32_t>(oi1),
                                        D.at<int32_t>(oi2), D.at<float>(ox), D.at<uint8_t>(os), D.at<int32_t>(omt), D.at<int32_t>(ost));
    if (rc) return rc;
    std::vector<char> back(D.off - in_bytes);
    if ((rc = rfe_memcpy_d2h(ctx, back.data(), D.base + in_bytes, back.size()))) return rc;      // waits for the stream
    auto get = [&](size_t o) { return back.data() + (o - in_bytes); };
    std::copy((const int32_t*)get(ost), (const int32_t*)get(ost) + 8, out.stats);
    out.matches.assign((const int32_t*)get(omt), (const int32_t*)get(omt) + Nn);
    for (int32_t m : out.matches) out.matchsum += (float)m;
    const int created = std::min<int>(out.stats[0], N1);
    const int32_t *pn = (const int32_t*)get(oon), *p1 = (const int32_t*)get(oi1), *p2 = (const int32_t*)get(oi2);
    const float* px = (const float*)get(ox);
    const uint8_t* ps = (const uint8_t*)get(os);
    out.points.resize((size_t)created);
    for (int k = 0; k < created; ++k) out.points[k] = NewMapPoint_rfe{pn[k], p1[k], p2[k], {px[3 * k], px[3 * k + 1], px[3 * k + 2]}, ps[k] != 0};
    if (prm.keep_matches) {
        out.S.resize((size_t)Nn); out.pairs.resize((size_t)Nn * Kmax * 2);
        if ((rc = rfe_memcpy_d2h(ctx, out.S.data(), S_dev, (size_t)Nn * 4))) return rc;
        if (!out.pairs.empty() && (rc = rfe_memcpy_d2h(ctx, out.pairs.data(), pairs_dev, out.pairs.size() * 4))) return rc;
    }
    return created;
}

// The whole of CreateNewMapPoints up to `new MapPoint`: LightGlue for all neighbours as ONE rfe_match_dev (P = Nn, the current keyframe as
// set 0 of every pair, keypoints normalised with the hard-coded 300 x 400 of the overload SearchForTriangulation calls), then
// TriangulateMatches_rfe on the same stream.  Returns as TriangulateMatches_rfe.
template <class KeyFrameT>
int CreateNewMapPoints_rfe(rfe_ctx* ctx, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, const CreateNewMapPointsParams_rfe& prm,
                           CreateNewMapPointsOut_rfe& out) {
    using namespace rfe_tri_detail;
    out = CreateNewMapPointsOut_rfe();
    const int Nn = (int)vpNeighKFs.size(), N1 = (int)pKF1->mvKeys.size();
    if (!one_pinhole(pKF1)) return -1;
    for (KeyFrameT* kf : vpNeighKFs) if (!one_pinhole(kf)) return -1;
    if (Nn == 0) return 0;
    if (Nn > 64) return RFE_ERR_INVALID;
    int N2max = 0;
    for (KeyFrameT* kf : vpNeighKFs) N2max = std::max(N2max, (int)kf->mvKeys.size());
    const int Kmax = std::min(N1, N2max);
    if (Kmax == 0) { out.matches.assign((size_t)Nn, 0); return 0; }   // a keyframe without features: nothing to match
    const size_t s0 = (size_t)Nn * N1, s1 = (size_t)Nn * N2max;
    // NormalizeKeypoints(kpts, 300, 400), src/Matchers/transform.cpp:19-32: shift (w / 2, h / 2) = (200, 150), scale max(w, h) / 2 = 200
    auto norm = [](const cv::KeyPoint& kp, float* dst) { dst[0] = (kp.pt.x - 200.f) / 200.f; dst[1] = (kp.pt.y - 150.f) / 200.f; };
    std::vector<float> k0(s0 * 2), k1(s1 * 2), d0(s0 * 256), d1(s1 * 256);
    std::vector<int32_t> m((size_t)Nn, N1), n((size_t)Nn);
    for (int p = 0; p < Nn; ++p) {
        KeyFrameT* kf = vpNeighKFs[p];
        for (int i = 0; i < N1; ++i) {
            norm(pKF1->mvKeys[i], &k0[2 * ((size_t)p * N1 + i)]);
            rfe_detail::copy_descriptor(pKF1->mDescriptors, i, &d0[((size_t)p * N1 + i) * 256]);
        }
        n[p] = (int)kf->mvKeys.size();
        for (int j = 0; j < n[p]; ++j) {
            norm(kf->mvKeys[j], &k1[2 * ((size_t)p * N2max + j)]);
            rfe_detail::copy_descriptor(kf->mDescriptors, j, &d1[((size_t)p * N2max + j) * 256]);
        }
    }
    DevBlock D(ctx);
    const size_t ok0 = D.reserve<float>(s0 * 2), ok1 = D.reserve<float>(s1 * 2), od0 = D.reserve<float>(s0 * 256), od1 = D.reserve<float>(s1 * 256),
                 om = D.reserve<int32_t>(Nn), on = D.reserve<int32_t>(Nn), oS = D.reserve<int32_t>(Nn), op = D.reserve<int32_t>((size_t)Nn * Kmax * 2),
                 oms = D.reserve<float>((size_t)Nn * Kmax);
    int rc = rfe_malloc(ctx, D.off, (void**)&D.base);
    if (rc) return rc;
    if ((rc = rfe_memcpy_h2d(ctx, D.at<float>(ok0), k0.data(), s0 * 8)) || (rc = rfe_memcpy_h2d(ctx, D.at<float>(ok1), k1.data(), s1 * 8)) ||
        (rc = rfe_memcpy_h2d(ctx, D.at<float>(od0), d0.data(), s0 * 1024)) || (rc = rfe_memcpy_h2d(ctx, D.at<float>(od1), d1.data(), s1 * 1024)) ||
        (rc = rfe_memcpy_h2d(ctx, D.at<int32_t>(om), m.data(), (size_t)Nn * 4)) || (rc = rfe_memcpy_h2d(ctx, D.at<int32_t>(on), n.data(), (size_t)Nn * 4)))
        return rc;
    rc = rfe_match_dev(ctx, D.at<float>(ok0), D.at<float>(ok1), D.at<float>(od0), D.at<float>(od1), D.at<int32_t>(om), D.at<int32_t>(on), Nn, N1, N2max,
                       prm.filter_thr, D.at<int32_t>(oS), D.at<int32_t>(op), D.at<float>(oms));
    if (rc) return rc;
    return TriangulateMatches_rfe(ctx, pKF1, vpNeighKFs, prm, D.at<int32_t>(oS), D.at<int32_t>(op), Kmax, out);
}

}  // namespace ORB_SLAM3
