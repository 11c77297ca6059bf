// api_stereo.hip -- C ABI of librover_fe.so: sparse stereo matching (plain and octave-aware) and the device-resident stereo-frame entries.
#include <string.h>
#include <algorithm>
#include "api_internal.h"

using namespace rfe;

// =====================================================================================
// sparse stereo matching (Frame::ComputeStereoMatches, src/Frame.cc:1159-1446)
// =====================================================================================
// the argument check of both forms.  They have always differed and callers see it: the host form reports a bad shape without the hint and
// leaves mb to the device form it calls behind its uploads (so mb <= 0 passes when N == 0)
static int stereo_check(rfe_ctx* c, int H, int W, int stride, int N, int Nr, float mb, bool dev_form) {
    if (!c) return RFE_ERR_INVALID;
    if (N < 0 || Nr < 0 || N > 4096 || H <= 0 || W <= 0 || stride < W || (dev_form && !(mb > 0.f)))
        return fail(c, RFE_ERR_INVALID, dev_form ? "stereo_match: bad argument (0 <= N <= 4096, mb > 0, stride >= W)" : "stereo_match: bad argument");
    return RFE_OK;
}

extern "C" int rfe_stereo_match_dev(rfe_ctx* c, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride,
                                    const float* kL, int N, const float* kR, int Nr, const float* dL, const float* dR,
                                    float mb, float mbf, float* uRight, float* depth) {
    int rc = stereo_check(c, H, W, stride, N, Nr, mb, true);
    if (rc || N == 0) return rc;
    if (!imgL || !imgR || !kL || !dL || !uRight || !depth || (Nr > 0 && (!kR || !dR))) return fail(c, RFE_ERR_INVALID, "stereo_match: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure_ws(c, &c->ws_tmp, &c->ws_tmp_bytes, al((size_t)N * 4)))) return rc;
    ProfScope p(c, "stereo_match");
    launch_stereo_match(c->stream, imgL, imgR, H, W, stride, kL, N, kR, Nr, dL, dR, mb, mbf, uRight, depth, (int32_t*)c->ws_tmp);
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_stereo_match(rfe_ctx* c, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride,
                                const float* kL, int N, const float* kR, int Nr, const float* dL, const float* dR,
                                float mb, float mbf, float* uRight, float* depth) {
    int rc = stereo_check(c, H, W, stride, N, Nr, mb, false);
    if (rc || N == 0) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    uint8_t *dIL, *dIR; float *dkl, *dkr, *ddl, *ddr, *du, *dz;
    HostIo io(c, HostIo::DIRECT);
    io.image(dIL, imgL, (size_t)W, (size_t)H, (size_t)stride);   // tight device copy (ROI-safe)
    io.image(dIR, imgR, (size_t)W, (size_t)H, (size_t)stride);
    io.in(dkl, kL, (size_t)N * 2); io.in(ddl, dL, (size_t)N * 256);
    io.in(dkr, kR, (size_t)Nr * 2); io.in(ddr, dR, (size_t)Nr * 256);
    io.out(du, uRight, N); io.out(dz, depth, N);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_stereo_match_dev(c, dIL, dIR, H, W, W, dkl, N, dkr, Nr, ddl, ddr, mb, mbf, du, dz))) return rc;
    return io.download();
}

// =====================================================================================
// stereo stream (BASELINE configs[4]): one device-resident entry point per stereo frame
// =====================================================================================
__global__ void st_zero_count_kernel(int32_t* S) { S[0] = 0; }

// One launch in front of the temporal match of a stereo frame (round 5: it replaced normalize_kpts + lg_stage + the save kernel behind the match).  One wave per
// token row of the pair layout [side 0 = this left view | side 1 = the previous left view], L rows each:
//   side 0: NormalizeKeypoints (reference src/Matchers/transform.cpp:19-32) of the integer keypoint, descriptor row -> x, rotary table row -> csn, AND both into
//           the state slot that becomes "previous" for the next frame (two slots, flipped per frame: nothing is copied after the match);
//   side 1: the stored normalised keypoint / descriptor of the previous view -> x, csn;
// workgroup 0: clamped lengths, cross-attention map, the next slot's keypoint count.  have_prev = 0 (first frame of a stream): side 1 is zero-filled, length 0.
// KT: int32 (rfe_stereo_frame_dev: the extractor's integer pixels) or float (rfe_stereo_frame_pyramid_dev: level-0 coordinates of the merged levels)
template <typename KT>
__device__ __forceinline__ void st_stage_body(const KT* __restrict__ kxy, const float* __restrict__ desc, const int32_t* __restrict__ n, int Kmax, int L,
                                              float sx, float sy, float scale, const float* __restrict__ kn_prev, const float* __restrict__ desc_prev,
                                              const int32_t* __restrict__ n_prev, int have_prev, const float* __restrict__ wr, float* __restrict__ x,
                                              float* __restrict__ kn, float2* __restrict__ csn, int32_t* __restrict__ lens, int32_t* __restrict__ kvmap,
                                              float* __restrict__ kn_next, float* __restrict__ desc_next, int32_t* __restrict__ n_next) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int v0 = n[0]; v0 = v0 < 0 ? 0 : (v0 > Kmax ? Kmax : v0);
        int v1 = have_prev ? n_prev[0] : 0; v1 = v1 < 0 ? 0 : (v1 > Kmax ? Kmax : v1);
        lens[0] = v0; lens[1] = v1; kvmap[0] = 1; kvmap[1] = 0;
        n_next[0] = n[0];
    }
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= 2 * L) return;
    const int side = row >= L, i = side ? row - L : row;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float kx = 0.f, ky = 0.f;
    if (i < Kmax) {
        if (!side) {
            v = reinterpret_cast<const float4*>(desc + (size_t)i * 256)[lane];
            kx = ((float)kxy[2 * i] - sx) / scale; ky = ((float)kxy[2 * i + 1] - sy) / scale;
            reinterpret_cast<float4*>(desc_next + (size_t)i * 256)[lane] = v;
            if (lane == 0) reinterpret_cast<float2*>(kn_next)[i] = make_float2(kx, ky);
        } else if (have_prev) {
            v = reinterpret_cast<const float4*>(desc_prev + (size_t)i * 256)[lane];
            const float2 kp = reinterpret_cast<const float2*>(kn_prev)[i];
            kx = kp.x; ky = kp.y;
        }
    }
    reinterpret_cast<float4*>(x + (size_t)row * 256)[lane] = v;
    if (lane == 0) reinterpret_cast<float2*>(kn)[row] = make_float2(kx, ky);
    if (lane < 32) {
        const float th = fmaf(wr[2 * lane + 1], ky, wr[2 * lane] * kx);
        csn[(size_t)row * 32 + lane] = make_float2(cosf(th), sinf(th));
    }
}
__global__ __launch_bounds__(256) void st_stage_kernel(const int32_t* __restrict__ kxy, const float* __restrict__ desc, const int32_t* __restrict__ n, int Kmax, int L,
                                                       float sx, float sy, float scale, const float* __restrict__ kn_prev, const float* __restrict__ desc_prev,
                                                       const int32_t* __restrict__ n_prev, int have_prev, const float* __restrict__ wr, float* __restrict__ x,
                                                       float* __restrict__ kn, float2* __restrict__ csn, int32_t* __restrict__ lens, int32_t* __restrict__ kvmap,
                                                       float* __restrict__ kn_next, float* __restrict__ desc_next, int32_t* __restrict__ n_next) {
    st_stage_body<int32_t>(kxy, desc, n, Kmax, L, sx, sy, scale, kn_prev, desc_prev, n_prev, have_prev, wr, x, kn, csn, lens, kvmap, kn_next, desc_next, n_next);
}
__global__ __launch_bounds__(256) void st_stage_f32_kernel(const float* __restrict__ kpts, const float* __restrict__ desc, const int32_t* __restrict__ n, int Kmax, int L,
                                                           float sx, float sy, float scale, const float* __restrict__ kn_prev, const float* __restrict__ desc_prev,
                                                           const int32_t* __restrict__ n_prev, int have_prev, const float* __restrict__ wr, float* __restrict__ x,
                                                           float* __restrict__ kn, float2* __restrict__ csn, int32_t* __restrict__ lens, int32_t* __restrict__ kvmap,
                                                           float* __restrict__ kn_next, float* __restrict__ desc_next, int32_t* __restrict__ n_next) {
    st_stage_body<float>(kpts, desc, n, Kmax, L, sx, sy, scale, kn_prev, desc_prev, n_prev, have_prev, wr, x, kn, csn, lens, kvmap, kn_next, desc_next, n_next);
}

// ws_st, the stereo stream state: sadv [K] | two slots of { kn [K,2], desc [K,256], n [1] }: the previous left
// view lives in slot st_flip, this frame's staging kernel fills the other one, then the slots swap -- nothing is copied behind the match
struct StState { int32_t* sadv; float* kn[2]; float* desc[2]; int32_t* n[2]; };
static int st_carve(rfe_ctx* c, int K, StState& st) {
    return ws_carve(c, &c->ws_st, &c->ws_st_bytes, [&](Bump& a) {
        st.sadv = a.take<int32_t>(K);
        for (int q = 0; q < 2; ++q) { st.kn[q] = a.take<float>((size_t)K * 2); st.desc[q] = a.take<float>((size_t)K * 256); st.n[q] = a.take<int32_t>(1); }
    });
}

// The temporal match of a stereo frame and its join with the stereo kernels the caller has just enqueued (st_fork: on the side stream, ev_join recorded
// behind them).  kxy: the extractor's integer pixels (rfe_stereo_frame_dev) or level-0 float coordinates (rfe_stereo_frame_pyramid_dev).
static auto st_stage_for(const int32_t*) { return st_stage_kernel; }
static auto st_stage_for(const float*) { return st_stage_f32_kernel; }
template <typename KT>
static int st_temporal_match(rfe_ctx* c, bool st_fork, const KT* kxy, const float* desc, const int32_t* n, int K, int H, int W, float filter_thr, const StState& st,
                             int32_t* S, int32_t* pairs, float* ms) {
    hipStream_t s = c->stream;
    // every exit below -- the error returns of ensure_ws / lg_forward included -- joins the side stream first: the caller's NEXT call
    // rewrites uRight / depth (and its image buffers) on the ctx stream, which must not overtake stereo kernels still reading or writing them
    struct JoinGuard { rfe_ctx* c; hipStream_t s; bool on; ~JoinGuard() { if (on) (void)hipStreamWaitEvent(s, c->ev_join, 0); } } join_guard{c, s, st_fork};
    // temporal match exactly as Tracking issues it: SearchBySP(mCurrentFrame, mLastFrame) (src/Tracking.cc:3465) ->
    // MatchingPoints_onnx(CurrentFrame, LastFrame, vnMatches1) (src/Matchers/SPmatcher.cc:1050-1054): THIS left view is set 0,
    // the previous left view set 1, so pairs are (current index, previous index) like vnMatches1[IdxCF] = IdxLF; true image
    // size like the Frame overload (:457-542, :463-464)
    const int L = ((K + 3) / 4) * 4, prev = c->st_flip & 1, next = prev ^ 1;
    LgBuffers b;
    int rc = lg_carve(c, 1, L, b);
    if (rc) return rc;
    const float sx = (float)W / 2, sy = (float)H / 2, scale = (float)(H > W ? H : W) / 2;     // launch_normalize_kpts' constants
    { ProfScope ps(c, "lg_misc");   // ONE staging launch: normalise, rotary table, token rows of both sides, lengths -- and this view into the next slot
      hipLaunchKernelGGL(st_stage_for(kxy), dim3((unsigned)((2 * L + 3) / 4)), dim3(256), 0, s, kxy, desc, n, K, L, sx, sy, scale, st.kn[prev], st.desc[prev],
                         st.n[prev], c->st_have_prev ? 1 : 0, c->lg.wr, b.x, b.kn, reinterpret_cast<float2*>(b.csn), b.lens, b.kvmap, st.kn[next], st.desc[next],
                         st.n[next]); }
    if (c->st_have_prev) {
        if ((rc = lg_forward(c, b, 1, L, filter_thr, K, S, pairs, ms, nullptr, false, true))) return rc;
    } else {
        hipLaunchKernelGGL(st_zero_count_kernel, dim3(1), dim3(1), 0, s, S);
    }
    c->st_flip = next;
    if (st_fork) { join_guard.on = false; RFE_HIP(c, hipStreamWaitEvent(s, c->ev_join, 0)); }   // uRight / depth are complete when the ctx stream is
    c->st_have_prev = true;
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_stereo_frame_dev(rfe_ctx* c, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride, int Kmax,
                                    float thr, float filter_thr, float mb, float mbf, int reset, int32_t* n, int32_t* kxy,
                                    float* score, float* desc, float* uRight, float* depth, int32_t* S, int32_t* pairs,
                                    float* ms) {
    int rc = sp_check(c, H, W, 2, Kmax);
    if (rc) return rc;
    if ((rc = lg_check(c, 1, Kmax, Kmax))) return rc;
    if (!imgL || !imgR || !n || !kxy || !score || !desc || !uRight || !depth || !S || !pairs || !ms || stride < W || !(mb > 0.f))
        return fail(c, RFE_ERR_INVALID, "stereo_frame: null pointer, stride < W or mb <= 0");
    RFE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const bool fresh = c->st_H != H || c->st_W != W || c->st_K != Kmax || !c->st_pyr_key.empty();   // st_pyr_key: the stored view is rfe_stereo_frame_pyramid_dev's
    StState st;
    if ((rc = st_carve(c, Kmax, st))) return rc;
    if (fresh || reset) { c->st_have_prev = false; c->st_H = H; c->st_W = W; c->st_K = Kmax; c->st_pyr_key.clear(); }
    // both views as ONE batch of 2 (the reference runs them on two threads, src/Frame.cc:142-147).  Measured alternative: the
    // right view + stereo match on a second lane (own streams / workspace) next to left view + LightGlue -- 3.52 ms per stereo
    // frame against 3.26 ms for this form: two batch-1 extractions are no faster than one batch of 2, and the co-running
    // kernels slow the latency-bound LightGlue chain (profiles/r02_ab_notes.md).  The two views are read where the caller has them (round 5: conv1's
    // tile loader takes the distance between frame 0 and frame 1 -- any distance, here imgR - imgL; the two staging copies are gone).  The caller keeps
    // them valid until the ctx stream has passed this call, like every input of a *_dev entry.
    if ((rc = sp_forward(c, imgL, H, W, stride, 2, Kmax, thr, n, kxy, score, desc, nullptr, false, (long long)(imgR - imgL)))) return rc;
    // Frame::ComputeStereoMatches (src/Frame.cc:1159-1446) on the device-resident features; counts stay on the device
    // ... on the SIDE stream: the stereo kernels (45 us of small launches) and the temporal LightGlue match below only share their inputs, and
    // the one-pair LightGlue is a chain of latency-bound kernels that leaves room next to it (with an event pair around every stage, full
    // profiling pass, everything stays serial so that the stage times are clean)
    const bool st_fork = c->st_have_prev && !(c->prof && c->prof_filter.empty());
    hipStream_t ss = st_fork ? c->side_stream : s;
    if (st_fork) { RFE_HIP(c, hipEventRecord(c->ev_fork, s)); RFE_HIP(c, hipStreamWaitEvent(ss, c->ev_fork, 0)); }
    { ProfScope ps(c, "stereo_match", ss);
      launch_stereo_match_counts(ss, imgL, imgR, H, W, stride, kxy, kxy + (size_t)Kmax * 2, Kmax, n, desc,
                                 desc + (size_t)Kmax * 256, mb, mbf, uRight, depth, st.sadv); }
    if (st_fork) RFE_HIP(c, hipEventRecord(c->ev_join, ss));
    return st_temporal_match(c, st_fork, kxy, desc, n, Kmax, H, W, filter_thr, st, S, pairs, ms);
}

// =====================================================================================
// octave-aware sparse stereo matching: Frame::ComputeStereoMatches for keypoints of a scale pyramid
// =====================================================================================
namespace {

// validation of the level geometry shared by the three entries + the kernel's level table; frame = sum_l H_l * W_l
int stereo_pyr_table(rfe_ctx* c, int H, int W, int L, float sf, int sad_source, float mb, StereoPyrTable& T, size_t& frame) {
    int32_t h[RFE_MAX_LEVELS], w[RFE_MAX_LEVELS]; float sc[RFE_MAX_LEVELS];
    if (pyramid_geometry(H, W, L, sf, h, w, sc) != RFE_OK)
        return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: H, W >= 8, nlevels in 1..16, scale_factor in (1, 4] when nlevels > 1, no level of zero pixels");
    if (sad_source != RFE_STEREO_SAD_LEVEL && sad_source != RFE_STEREO_SAD_LEVEL0)
        return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: sad_source must be RFE_STEREO_SAD_LEVEL or RFE_STEREO_SAD_LEVEL0");
    if (!(mb > 0.f)) return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: mb must be positive");
    memset(&T, 0, sizeof(T));
    T.L = L; frame = 0;
    for (int l = 0; l < L; ++l) {
        T.h[l] = h[l]; T.w[l] = w[l]; T.off[l] = (uint32_t)frame; T.s[l] = sc[l]; T.inv[l] = 1.0f / sc[l];
        frame += (size_t)h[l] * w[l];
    }
    if (frame > 0x7fffffffull) return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: level buffer above 2 GiB");
    return RFE_OK;
}

}  // namespace

// the argument check of both forms (the pointers are the caller's, whichever side they live on); N == 0 passes without a look at them
static int stereo_pyr_check(rfe_ctx* c, const void* levelsL, const void* levelsR, int H, int W, int nlevels, float scale_factor, const void* kL, const void* octL,
                            int N, const void* kR, const void* octR, int Nr, const void* dL, const void* dR, float mb, int sad_source, const void* uRight,
                            const void* depth, StereoPyrTable& T, size_t& frame) {
    if (!c) return RFE_ERR_INVALID;
    int rc = stereo_pyr_table(c, H, W, nlevels, scale_factor, sad_source, mb, T, frame);
    if (rc) return rc;
    if (N < 0 || Nr < 0 || N > 4096 || Nr > 4096) return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: N and Nr must be in 0..4096");
    if (N == 0) return RFE_OK;
    if (!levelsL || !levelsR || !kL || !octL || !dL || !uRight || !depth || (Nr > 0 && (!kR || !octR || !dR)))
        return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: null pointer");
    return RFE_OK;
}
extern "C" int rfe_stereo_match_pyramid_dev(rfe_ctx* c, const uint8_t* levelsL, const uint8_t* levelsR, int H, int W, int nlevels, float scale_factor,
                                            const float* kL, const int32_t* octL, int N, const float* kR, const int32_t* octR, int Nr,
                                            const float* dL, const float* dR, float mb, float mbf, int sad_source, float* uRight, float* depth) {
    StereoPyrTable T; size_t frame;
    int rc = stereo_pyr_check(c, levelsL, levelsR, H, W, nlevels, scale_factor, kL, octL, N, kR, octR, Nr, dL, dR, mb, sad_source, uRight, depth, T, frame);
    if (rc || N == 0) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure_ws(c, &c->ws_tmp, &c->ws_tmp_bytes, al((size_t)N * 4)))) return rc;
    ProfScope p(c, "stereo_match");
    launch_stereo_match_pyr(c->stream, levelsL, levelsR, T, kL, octL, N, kR, octR, Nr, nullptr, dL, dR, mb, mbf, sad_source == RFE_STEREO_SAD_LEVEL0,
                            uRight, depth, (int32_t*)c->ws_tmp);
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_stereo_match_pyramid(rfe_ctx* c, const uint8_t* levelsL, const uint8_t* levelsR, int H, int W, int nlevels, float scale_factor,
                                        const float* kL, const int32_t* octL, int N, const float* kR, const int32_t* octR, int Nr,
                                        const float* dL, const float* dR, float mb, float mbf, int sad_source, float* uRight, float* depth) {
    StereoPyrTable T; size_t frame;
    int rc = stereo_pyr_check(c, levelsL, levelsR, H, W, nlevels, scale_factor, kL, octL, N, kR, octR, Nr, dL, dR, mb, sad_source, uRight, depth, T, frame);
    if (rc || N == 0) return rc;
    // the kernel treats an octave outside [0, nlevels) as "no match / not a candidate"; here the arrays are readable, so it is refused
    for (int i = 0; i < N; ++i) if (octL[i] < 0 || octL[i] >= nlevels) return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: left octave outside [0, nlevels)");
    for (int i = 0; i < Nr; ++i) if (octR[i] < 0 || octR[i] >= nlevels) return fail(c, RFE_ERR_INVALID, "stereo_match_pyramid: right octave outside [0, nlevels)");
    RFE_HIP(c, hipSetDevice(c->device));
    uint8_t *dVL, *dVR; float *dkl, *dkr, *ddl, *ddr, *du, *dz; int32_t *dol, *dor;
    HostIo io(c, HostIo::DIRECT);
    io.in(dVL, levelsL, frame); io.in(dVR, levelsR, frame);
    io.in(dkl, kL, (size_t)N * 2); io.in(dol, octL, N); io.in(ddl, dL, (size_t)N * 256);
    io.in(dkr, kR, (size_t)Nr * 2); io.in(dor, octR, Nr); io.in(ddr, dR, (size_t)Nr * 256);
    io.out(du, uRight, N); io.out(dz, depth, N);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_stereo_match_pyramid_dev(c, dVL, dVR, H, W, nlevels, scale_factor, dkl, dol, N, dkr, dor, Nr, ddl, ddr, mb, mbf, sad_source, du, dz))) return rc;
    return io.download();
}

// rfe_stereo_frame_dev for pyramids: the same three stages, with pyr_forward in place of sp_forward, the octave-aware stereo kernels and the
// float-keypoint staging kernel.  The previous-view state lives in the same ws_st slots; st_pyr_key names the shape it was stored under.
extern "C" int rfe_stereo_frame_pyramid_dev(rfe_ctx* c, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride, int nlevels,
                                            float scale_factor, const int32_t* kmax, float thr, float filter_thr, float mb, float mbf,
                                            int sad_source, int reset, int32_t* n, int32_t* level_n, float* kpts, int32_t* octave,
                                            float* score, float* desc, float* uRight, float* depth, int32_t* S, int32_t* pairs, float* ms) {
    PyrPlan P;
    int rc = pyr_check(c, H, W, stride, 2, nlevels, scale_factor, kmax, P);
    if (rc) return rc;
    if (P.Ktot > 4096) return fail(c, RFE_ERR_INVALID, "stereo_frame_pyramid: the sum of kmax must be at most 4096");
    const int K = P.Ktot;
    if ((rc = lg_check(c, 1, K, K))) return rc;
    StereoPyrTable T; size_t frame;
    if ((rc = stereo_pyr_table(c, H, W, nlevels, scale_factor, sad_source, mb, T, frame))) return rc;
    if (!imgL || !imgR || !n || !kpts || !octave || !score || !desc || !uRight || !depth || !S || !pairs || !ms)
        return fail(c, RFE_ERR_INVALID, "stereo_frame_pyramid: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int sf_bits; memcpy(&sf_bits, &scale_factor, 4);
    std::string key = std::to_string(H) + "x" + std::to_string(W) + "|" + std::to_string(nlevels) + "|" + std::to_string(nlevels > 1 ? sf_bits : 0);
    for (int l = 0; l < nlevels; ++l) key += "," + std::to_string(kmax[l]);
    const bool fresh = c->st_pyr_key != key;
    // every allocation before the first kernel of the call (ensure_ws synchronises the ctx stream only; the side stream is idle between calls)
    StState st;
    if ((rc = st_carve(c, K, st))) return rc;
    if ((rc = ensure_ws(c, &c->ws_lg, &c->ws_lg_bytes, lg_ws_bytes(c, 1, ((K + 3) / 4) * 4)))) return rc;
    if ((rc = pyr_prepare(c, H, W, 2, scale_factor, P, true))) return rc;
    if (fresh || reset) { c->st_have_prev = false; c->st_H = H; c->st_W = W; c->st_K = K; c->st_pyr_key = key; }
    // both views as one batch of 2, read where the caller has them (frame distance imgR - imgL); every level image, level 0 included, is
    // kept in ws_pyr for the SAD refinement: view b's levels at lv + b * frame
    uint8_t* lv = (uint8_t*)c->ws_pyr;
    if ((rc = pyr_forward(c, imgL, H, W, stride, 2, P, thr, lv, true, n, level_n, kpts, octave, score, desc, (long long)(imgR - imgL)))) return rc;
    // the stereo kernels on the side stream next to the temporal match, joined on every exit path, as in rfe_stereo_frame_dev
    const bool st_fork = c->st_have_prev && !(c->prof && c->prof_filter.empty());
    hipStream_t ss = st_fork ? c->side_stream : s;
    if (st_fork) { RFE_HIP(c, hipEventRecord(c->ev_fork, s)); RFE_HIP(c, hipStreamWaitEvent(ss, c->ev_fork, 0)); }
    { ProfScope ps(c, "stereo_match", ss);
      launch_stereo_match_pyr(ss, lv, lv + frame, T, kpts, octave, K, kpts + (size_t)K * 2, octave + K, K, n, desc, desc + (size_t)K * 256, mb, mbf,
                              sad_source == RFE_STEREO_SAD_LEVEL0, uRight, depth, st.sadv); }
    if (st_fork) RFE_HIP(c, hipEventRecord(c->ev_join, ss));
    // temporal match: THIS left view (set 0) against the previous left view (set 1), true image size, NormalizeKeypoints of the float keypoints
    return st_temporal_match(c, st_fork, kpts, desc, n, K, H, W, filter_thr, st, S, pairs, ms);
}
