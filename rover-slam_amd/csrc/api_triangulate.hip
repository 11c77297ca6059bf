// api_triangulate.hip -- C ABI of librover_fe.so: LocalMapping::CreateNewMapPoints behind the matcher, all neighbours of a keyframe in one
// call (triangulate.hip).
#include <string.h>
#include <algorithm>
#include "api_internal.h"

using namespace rfe;

static int tri_check(rfe_ctx* c, const rfe_tri_params* P, const rfe_tri_view* view1, const void* kpts1, const void* oct1, const void* ur1,
                     const void* dep1, const void* mp1, int N1, const void* views2, const void* kpts2, const void* oct2, const void* ur2,
                     const void* dep2, const void* mp2, const void* n2, int Nn, int N2max, const void* S, const void* pairs, int Kmax,
                     const void* stats) {
    if (!P || !view1 || !stats) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: null pointer");
    if (Nn < 0 || Nn > 64) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: Nn outside 0..64");
    if (N1 < 0 || N1 > 4096) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: N1 outside 0..4096");
    if (N2max < 0 || N2max > 4096) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: N2max outside 0..4096");
    if (Kmax < 0 || Kmax > 4096) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: Kmax outside 0..4096");
    if (P->nlevels < 1 || P->nlevels > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: nlevels outside 1..16");
    if ((N1 > 0 && (!kpts1 || !oct1 || !ur1 || !dep1 || !mp1)) || (Nn > 0 && (!views2 || !n2 || !S)) || (Nn > 0 && Kmax > 0 && !pairs) ||
        (Nn > 0 && N2max > 0 && (!kpts2 || !oct2 || !ur2 || !dep2 || !mp2)))
        return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: null pointer");
    return RFE_OK;
}

extern "C" int rfe_triangulate_neighbours_dev(rfe_ctx* c, const rfe_tri_params* P, const rfe_tri_view* view1, const float* kpts1,
                                              const float* kpts1_raw, const int32_t* octave1, const float* uright1, const float* depth1,
                                              const uint8_t* has_mp1, int N1, const rfe_tri_view* views2, const float* kpts2,
                                              const float* kpts2_raw, const int32_t* octave2, const float* uright2, const float* depth2,
                                              const uint8_t* has_mp2, const int32_t* n2, const uint8_t* neighbour_valid, int Nn, int N2max,
                                              const int32_t* S, const int32_t* pairs, int Kmax, int32_t* code, float* x3d, uint8_t* point_stereo,
                                              int32_t* out_n, int32_t* out_idx1, int32_t* out_idx2, float* out_x3d, uint8_t* out_stereo,
                                              int32_t* matches, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = tri_check(c, P, view1, kpts1, octave1, uright1, depth1, has_mp1, N1, views2, kpts2, octave2, uright2, depth2, has_mp2, n2, Nn, N2max, S,
                       pairs, Kmax, stats);
    if (rc) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    TriBuffers b;
    rc = ws_carve(c, &c->ws_tri, &c->ws_tri_bytes, [&](Bump& a) { tri_layout(a, N1, Nn, Kmax, b); });
    if (rc) return rc;
    hipStream_t s = c->stream;
    RFE_HIP(c, hipMemsetAsync(stats, 0, 32, s));
    if (Nn > 0) {
        // claim and count lie side by side at the head of the workspace: 0x7f7f7f7f is above every neighbour index
        RFE_HIP(c, hipMemsetAsync(b.claim, 0x7f, (size_t)((char*)b.count - (char*)b.claim), s));
        RFE_HIP(c, hipMemsetAsync(b.count, 0, 64 * sizeof(int32_t), s));
    }
    { ProfScope ps(c, "tri_eval");
      launch_tri_eval(s, *P, *view1, kpts1, kpts1_raw, octave1, uright1, depth1, has_mp1, N1, views2, kpts2, kpts2_raw, octave2, uright2, depth2,
                      has_mp2, n2, neighbour_valid, Nn, N2max, S, pairs, Kmax, b.code, b.x3d, b.stereo, b.claim); }
    { ProfScope ps(c, "tri_resolve");
      launch_tri_resolve(s, S, neighbour_valid, pairs, N1, Nn, Kmax, b.code, b.x3d, b.stereo, b.claim, b.count, code, x3d, point_stereo, out_n,
                         out_idx1, out_idx2, out_x3d, out_stereo, matches, stats); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

static bool tri_view_finite(const rfe_tri_view& v) {
    return finite(v.rcw) && finite(v.tcw) && finite(v.ow) && finite({v.fx, v.fy, v.cx, v.cy, v.invfx, v.invfy, v.mb, v.mbf});
}

extern "C" int rfe_triangulate_neighbours(rfe_ctx* c, const rfe_tri_params* P, const rfe_tri_view* view1, const float* kpts1,
                                          const float* kpts1_raw, const int32_t* octave1, const float* uright1, const float* depth1,
                                          const uint8_t* has_mp1, int N1, const rfe_tri_view* views2, const float* kpts2, const float* kpts2_raw,
                                          const int32_t* octave2, const float* uright2, const float* depth2, const uint8_t* has_mp2,
                                          const int32_t* n2, const uint8_t* neighbour_valid, int Nn, int N2max, const int32_t* S,
                                          const int32_t* pairs, int Kmax, int32_t* code, float* x3d, uint8_t* point_stereo, int32_t* out_n,
                                          int32_t* out_idx1, int32_t* out_idx2, float* out_x3d, uint8_t* out_stereo, int32_t* matches,
                                          int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = tri_check(c, P, view1, kpts1, octave1, uright1, depth1, has_mp1, N1, views2, kpts2, octave2, uright2, depth2, has_mp2, n2, Nn, N2max, S,
                       pairs, Kmax, stats);
    if (rc) return rc;
    bool ok = finite({P->th_far, P->ratio_factor}) && tri_view_finite(*view1) && finite(P->scale_factors, P->nlevels) && finite(P->level_sigma2, P->nlevels);
    for (int n = 0; n < Nn; ++n) ok = ok && tri_view_finite(views2[n]);
    if (!ok) return fail(c, RFE_ERR_INVALID, "triangulate_neighbours: non-finite argument");
    RFE_HIP(c, hipSetDevice(c->device));
    const size_t f2 = (size_t)Nn * N2max, slots = (size_t)Nn * Kmax;
    float *dk1, *dr1, *du1, *dd1, *dk2, *dr2, *du2, *dd2, *dx3d, *dox; int32_t *do1, *do2, *dn2, *dS, *dpairs, *dcode, *don, *doi1, *doi2, *dm, *dst;
    uint8_t *dm1, *dm2, *dnv, *dps, *dos; rfe_tri_view* dv2;
    HostIo io(c, HostIo::DIRECT);
    io.in(dk1, kpts1, (size_t)N1 * 2); io.in_opt(dr1, kpts1_raw, (size_t)N1 * 2); io.in(do1, octave1, N1); io.in(du1, uright1, N1);
    io.in(dd1, depth1, N1); io.in(dm1, has_mp1, N1);
    io.in(dv2, views2, Nn); io.in(dk2, kpts2, f2 * 2); io.in_opt(dr2, kpts2_raw, f2 * 2); io.in(do2, octave2, f2); io.in(du2, uright2, f2);
    io.in(dd2, depth2, f2); io.in(dm2, has_mp2, f2); io.in(dn2, n2, Nn); io.in_opt(dnv, neighbour_valid, Nn);
    io.in(dS, S, Nn); io.in(dpairs, pairs, slots * 2);
    io.out_opt(dcode, code, slots); io.out_opt(dx3d, x3d, slots * 3); io.out_opt(dps, point_stereo, slots);
    io.out_opt(don, out_n, N1); io.out_opt(doi1, out_idx1, N1); io.out_opt(doi2, out_idx2, N1); io.out_opt(dox, out_x3d, (size_t)N1 * 3);
    io.out_opt(dos, out_stereo, N1); io.out_opt(dm, matches, Nn);
    io.scratch(dst, 8);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_triangulate_neighbours_dev(c, P, view1, dk1, dr1, do1, du1, dd1, dm1, N1, dv2, dk2, dr2, do2, du2, dd2, dm2, dn2, dnv, Nn, N2max, dS,
                                             dpairs, Kmax, dcode, dx3d, dps, don, doi1, doi2, dox, dos, dm, dst))) return rc;
    int32_t st[8];
    RFE_HIP(c, hipMemcpyAsync(st, dst, 32, hipMemcpyDeviceToHost, c->stream));
    if ((rc = io.download())) return rc;                                // waits for the stream
    memcpy(stats, st, 32);
    return st[0];
}
