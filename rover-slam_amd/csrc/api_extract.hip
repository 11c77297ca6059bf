// api_extract.hip -- C ABI of librover_fe.so: the SuperPoint pipeline (forward pass, plain entries) and SuperPoint on a scale pyramid.
#include <string.h>
#include "api_internal.h"

using namespace rfe;

// =====================================================================================
// SuperPoint pipeline
// =====================================================================================
namespace rfe {

static void sp_layout(Bump& a, int B, int H, int W, SpBuffers& b) {   // ws_sp
    const size_t hw = (size_t)B * H * W, cells = hw / 64;
    b.p1 = a.take<float>(hw / 4 * 64); b.a2 = a.take<float>(hw / 4 * 64);
    b.p2 = a.take<float>(hw / 16 * 64); b.a3 = a.take<float>(hw / 16 * 128);
    b.p3 = a.take<float>(cells * 128); b.a4 = a.take<float>(cells * 128); b.f4 = a.take<float>(cells * 128);
    b.pa = a.take<float>(cells * 256); b.da = a.take<float>(cells * 256); b.dmap = a.take<float>(cells * 256);
    b.logits = a.take<float>(cells * 65);
    b.smap = a.take<float>(hw); b.nmap = a.take<float>(hw); b.ss = a.take<float>(hw);
    b.mask = a.take<uint8_t>(hw); b.supp = a.take<uint8_t>(hw);
    b.cand_score = a.take<float>(hw); b.cand_idx = a.take<int32_t>(hw);
    b.sel_keys = a.take<unsigned long long>((size_t)B * 4096); b.sel_n = a.take<int32_t>(B);   // Kmax <= 4096
    // sparse descriptor head: cell_cnt = [B] rows per frame, [B + 1] their prefix sums; the patches lie over p1 | a2 (see SpBuffers)
    b.cell_row = a.take<int32_t>(cells); b.row_cell = a.take<int32_t>(cells); b.cell_cnt = a.take<int32_t>(2 * (size_t)B + 1);
    b.patch = b.p1;
}
size_t sp_ws_bytes(int B, int H, int W) { SpBuffers b; return layout_bytes([&](Bump& a) { sp_layout(a, B, H, W, b); }); }
int sp_carve(rfe_ctx* c, int B, int H, int W, SpBuffers& b) {
    return ws_carve(c, &c->ws_sp, &c->ws_sp_bytes, [&](Bump& a) { sp_layout(a, B, H, W, b); });
}

GemmArgs gemm_plain(const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.B = Bw; g.ldb = ldb; g.bias = bias; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.alpha = 1.0f; g.batch = 1;
    return g;
}

int sp_check(rfe_ctx* c, int H, int W, int B, int Kmax) {
    if (!c) return RFE_ERR_INVALID;
    if (!c->has_sp) return fail(c, RFE_ERR_NO_WEIGHTS, "SuperPoint weights not loaded (rfe_load_weights / rfe_set_weights)");
    if (H < 8 || W < 8 || B <= 0) return fail(c, RFE_ERR_INVALID, "extract: H and W must be at least 8, B > 0");
    if (Kmax <= 0 || Kmax > 4096) return fail(c, RFE_ERR_INVALID, "extract: Kmax must be in 1..4096");
    return RFE_OK;
}

// backbone + heads up to the NMS'ed score map and the normalised descriptor map (dense_head = false: no descriptor head at all -- the caller runs
// sp_desc_rows behind its keypoint selection; nothing is forked then)
// join = false: the caller still has detector-only work to enqueue and joins the descriptor stream itself
// (hipStreamWaitEvent(c->stream, c->ev_join)) when `forked` comes back true
int sp_forward_maps(rfe_ctx* c, const void* img, int H, int W, int stride, int B, SpBuffers& b, bool join, bool& forked, bool img_f32, long long frame_step,
                    float thr, bool want_maps, bool dense_head) {
    forked = false;
    int rc = sp_carve(c, B, H, W, b);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const SpWeightsDev& w = c->sp;
    // Any H, W >= 8 (the ONNX graph has dynamic axes): every 2x2/2 max-pool floors, so the levels are H1 = H/2, H2 = H1/2,
    // Hc = H2/2 and the score map / NMS / selection live on the 8Hc x 8Wc frame (= the image when H, W are multiples of 8;
    // KITTI 1241 x 376 -> 155 x 47 cells, score map 1240 x 376).  The workspace carve (sized from B*H*W) is an upper bound.
    const int H1 = H / 2, W1 = W / 2, H2 = H1 / 2, W2 = W1 / 2, Hc = H2 / 2, Wc = W2 / 2, cells = B * Hc * Wc;
    { ProfScope p(c, "conv1ab");   // conv1a recomputed inside conv1b's LDS staging: the [B,H,W,64] activation never touches HBM
      launch_conv1ab_fused(s, img, img_f32, stride, B, H, W, w.conv1a_w, w.bias[L_1A], w.packed[L_1B], w.bias[L_1B], b.p1, frame_step); }
    { ProfScope p(c, "conv2a"); launch_conv3x3(s, b.p1, B, H1, W1, 64, w.packed[L_2A], w.bias[L_2A], 64, true, kSpLayers[L_2A].pool, b.a2, L_2A); }
    { ProfScope p(c, "conv2b"); launch_conv3x3(s, b.a2, B, H1, W1, 64, w.packed[L_2B], w.bias[L_2B], 64, true, kSpLayers[L_2B].pool, b.p2, L_2B); }
    { ProfScope p(c, "conv3a"); launch_conv3x3(s, b.p2, B, H2, W2, 64, w.packed[L_3A], w.bias[L_3A], 128, true, kSpLayers[L_3A].pool, b.a3, L_3A); }
    { ProfScope p(c, "conv3b"); launch_conv3x3(s, b.a3, B, H2, W2, 128, w.packed[L_3B], w.bias[L_3B], 128, true, kSpLayers[L_3B].pool, b.p3, L_3B); }
    { ProfScope p(c, "conv4a"); launch_conv3x3(s, b.p3, B, Hc, Wc, 128, w.packed[L_4A], w.bias[L_4A], 128, true, kSpLayers[L_4A].pool, b.a4, L_4A); }
    { ProfScope p(c, "conv4b"); launch_conv3x3(s, b.a4, B, Hc, Wc, 128, w.packed[L_4B], w.bias[L_4B], 128, true, kSpLayers[L_4B].pool, b.f4, L_4B); }
    // The two heads only share their input f4.  The descriptor head (convDa, convDb, L2 norm: MFMA work) runs on the
    // side stream while the detector head continues on the main one with its tail of small bandwidth / latency-bound
    // kernels (convPb, softmax, 5 NMS passes, selection), which would otherwise leave most of the chip idle.
    // With events around every stage (full profiling pass) the heads stay serial so that the stage times are clean.
    const bool fork = dense_head && !(c->prof && c->prof_filter.empty());
    hipStream_t sd = fork ? c->side_stream : s;
    if (fork) { RFE_HIP(c, hipEventRecord(c->ev_fork, s)); RFE_HIP(c, hipStreamWaitEvent(sd, c->ev_fork, 0)); }
    if (dense_head) {
        { ProfScope p(c, "convDa", sd); launch_conv3x3(sd, b.f4, B, Hc, Wc, 128, w.packed[L_DA], w.bias[L_DA], 256, true, kSpLayers[L_DA].pool, b.da, L_DA); }
        { ProfScope p(c, "convDb", sd); launch_gemm_nt(sd, gemm_plain(b.da, 256, w.packed[L_DB], 256, w.bias[L_DB], b.dmap, 256, cells, 256, 256)); }
        { ProfScope p(c, "sp_post", sd); launch_descmap_norm(sd, b.dmap, cells); }
    }
    if (fork) RFE_HIP(c, hipEventRecord(c->ev_join, sd));
    { ProfScope p(c, "convPa"); launch_conv3x3(s, b.f4, B, Hc, Wc, 128, w.packed[L_PA], w.bias[L_PA], 256, true, kSpLayers[L_PA].pool, b.pa, L_PA); }
    { ProfScope p(c, "convPb"); launch_gemm_nt(s, gemm_plain(b.pa, 256, w.packed[L_PB], 256, w.bias[L_PB], b.logits, 65, cells, 65, 256)); }
    { ProfScope p(c, "sp_post");
      // one to four frames, published radius: softmax + NMS + candidate compaction in ONE launch (sp_post.hip: sp_tail_lat_kernel); otherwise the separate launches
      if (B <= 4 && c->hp.sp_nms_radius == 4) {
          if (!c->sp_cnt) { RFE_HIP(c, hipMalloc((void**)&c->sp_cnt, 8 * sizeof(int32_t))); c->sp_cnt_dirty = true; }
          if (c->sp_cnt_dirty) { RFE_HIP(c, hipMemsetAsync(c->sp_cnt, 0, 8 * sizeof(int32_t), s)); c->sp_cnt_dirty = false; }
          b.tail_fused = launch_sp_tail_lat(s, b.logits, B, Hc, Wc, c->hp.sp_nms_radius, c->hp.sp_remove_borders, thr, (unsigned long long*)b.cand_score, c->sp_cnt,
                                            want_maps ? b.smap : nullptr, want_maps ? b.nmap : nullptr);
          if (b.tail_fused) c->sp_cnt_dirty = true;      // until the ranking kernel (which zeroes the counters) is enqueued behind it
      }
      if (!b.tail_fused) {
          launch_softmax65_d2s(s, b.logits, 65, B, Hc, Wc, b.smap);
          launch_nms(s, b.smap, B, 8 * Hc, 8 * Wc, c->hp.sp_nms_radius, c->hp.sp_remove_borders, b.ss, b.mask, b.supp, b.nmap);
      } }
    if (fork && join) RFE_HIP(c, hipStreamWaitEvent(s, c->ev_join, 0));
    forked = fork && !join;
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

// The descriptor head on the cells the keypoints sample, for calls of more than four frames (the regime split of the detector tail).  desc_sample_kernel
// reads the <= 4 cells around each of <= Kmax keypoints and nothing else of the map -- 30 % of a VGA frame's 4800 cells at Kmax = 1024 -- so the two
// matrix stages run on those cells only, as rows of two plain GEMMs, on the main stream behind the selection:
//   cell list (ascending cell order per frame, no atomics; the frames' rows packed back to back) -> patch [rows, 1152] = each cell's 3x3x128 neighbourhood of f4 in the conv's reduction order,
//   +0.0f outside the map -> convDa as relu(bias + patch . W^T) with W = the OIHW weight [256][1152] -> convDb -> L2 norm, every stage on the live rows
//   (launches sized for B cap rows, the count read on the device: workgroups past it return at once; no host synchronisation).
// The plain GEMM path is the k-ascending chain from the bias that the conv kernels run per output, and it does not care which matrix
// row a cell sits in: the rows equal the dense map's cells bit for bit (tests/test_gpu_sparse_desc.py).  Leaves b.dmap = rows [row_base[B], 256].
int sp_desc_rows(rfe_ctx* c, SpBuffers& b, int B, int Hc, int Wc, int Kmax, const int32_t* n, const int32_t* kxy) {
    hipStream_t s = c->stream;
    const SpWeightsDev& w = c->sp;
    const int cap = sp_desc_cap(Kmax, Hc, Wc);
    int32_t* const row_base = b.cell_cnt + B;
    { ProfScope p(c, "sp_desc_cells");
      launch_desc_cells(s, B, Hc, Wc, 8 * Hc, 8 * Wc, n, kxy, Kmax, cap, b.cell_row, b.row_cell, b.cell_cnt, row_base);
      launch_desc_gather(s, b.f4, B, Hc, Wc, cap, b.row_cell, b.cell_cnt, row_base, b.patch); }
    { ProfScope p(c, "convDa_rows");
      GemmArgs g = gemm_plain(b.patch, 1152, w.da_rows, 1152, w.bias[L_DA], b.da, 256, B * cap, 256, 1152);
      g.relu = 1; g.m_valid = row_base + B;
      launch_gemm_nt(s, g); }
    { ProfScope p(c, "convDb_rows");
      GemmArgs g = gemm_plain(b.da, 256, w.packed[L_DB], 256, w.bias[L_DB], b.dmap, 256, B * cap, 256, 256);
      g.m_valid = row_base + B;
      launch_gemm_nt(s, g); }
    { ProfScope p(c, "sp_desc_norm"); launch_descrows_norm(s, b.dmap, B, cap, b.cell_cnt, row_base); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

int sp_forward(rfe_ctx* c, const void* img, int H, int W, int stride, int B, int Kmax, float thr,
               int32_t* n, int32_t* kxy, float* score, float* desc, uint8_t* desc_bin, bool img_f32, long long frame_step) {
    SpBuffers b;
    bool forked;
    const bool sparse = B > 4;   // up to four frames the dense head on the side stream hides under the detector tail and wins
    int rc = sp_forward_maps(c, img, H, W, stride, B, b, false, forked, img_f32, frame_step, thr, false, !sparse);
    if (rc) return rc;
    const int Hc = H / 2 / 2 / 2, Wc = W / 2 / 2 / 2, Hs = 8 * Hc, Ws = 8 * Wc;   // score-map frame, see sp_forward_maps
    { ProfScope p(c, "sp_select");
      if (b.tail_fused) {
          launch_select_keys(c->stream, (const unsigned long long*)b.cand_score, c->sp_cnt, B, Hs, Ws, Kmax, c->hp.sp_topk_always != 0, n, kxy, score);
          c->sp_cnt_dirty = false;
      } else
      launch_select(c->stream, b.nmap, B, Hs, Ws, Kmax, thr, b.cand_score, b.cand_idx, n, kxy, score, (int32_t*)b.ss /*NMS scratch, free by now*/, c->hp.sp_topk_always != 0, b.sel_keys, b.sel_n);
      if (forked) RFE_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));   // descriptor map ready
      if (!sparse) launch_desc_sample(c->stream, b.dmap, B, Hc, Wc, Hs, Ws, n, kxy, Kmax, desc, desc_bin); }
    if (sparse) {
        if ((rc = sp_desc_rows(c, b, B, Hc, Wc, Kmax, n, kxy))) return rc;
        ProfScope p(c, "sp_desc_sample");
        launch_desc_sample(c->stream, b.dmap, B, Hc, Wc, Hs, Ws, n, kxy, Kmax, desc, desc_bin, b.cell_row, b.cell_cnt + B);
    }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

}  // namespace rfe

// the argument check of every plain extract entry, host and device form alike (the pointers are the caller's, whichever side they live on)
static int extract_check(rfe_ctx* c, const void* img, int H, int W, int stride, int B, int Kmax, const void* n, const void* kxy, const void* score,
                         const void* desc) {
    int rc = sp_check(c, H, W, B, Kmax);
    if (rc) return rc;
    if (!img || !n || !kxy || !score || !desc || stride < W) return fail(c, RFE_ERR_INVALID, "extract: null pointer or stride < W");
    RFE_HIP(c, hipSetDevice(c->device));
    return RFE_OK;
}

extern "C" int rfe_extract_u8_bin_dev(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int Kmax,
                                      float thr, int32_t* n, int32_t* kxy, float* score, float* desc, uint8_t* desc_bin) {
    int rc = extract_check(c, img, H, W, stride, B, Kmax, n, kxy, score, desc);
    if (rc) return rc;
    return sp_forward(c, img, H, W, stride, B, Kmax, thr, n, kxy, score, desc, desc_bin);
}

extern "C" int rfe_extract_u8_dev(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int Kmax,
                                  float thr, int32_t* n, int32_t* kxy, float* score, float* desc) {
    return rfe_extract_u8_bin_dev(c, img, H, W, stride, B, Kmax, thr, n, kxy, score, desc, nullptr);
}

// The reference's float entry (Extractor_Inference on an already normalised CV_32F image, src/Extractors/superpoint_onnx.cc:88-118): the
// pixel values go into conv1a as they are, whatever their range -- no u8 round trip, no NormalizeImage.  stride in floats.
extern "C" int rfe_extract_f32_dev(rfe_ctx* c, const float* img, int H, int W, int stride, int B, int Kmax,
                                   float thr, int32_t* n, int32_t* kxy, float* score, float* desc) {
    int rc = extract_check(c, img, H, W, stride, B, Kmax, n, kxy, score, desc);
    if (rc) return rc;
    return sp_forward(c, img, H, W, stride, B, Kmax, thr, n, kxy, score, desc, nullptr, true);
}

// the host form of all three: px = bytes per pixel (1: u8 through the fused NormalizeImage, 4: normalised floats), stride in pixels.
// The device copy of the image is tight (pitch W): see HostIo::image.
static int extract_host(rfe_ctx* c, const void* img, size_t px, int H, int W, int stride, int B, int Kmax, float thr, int32_t* n, int32_t* kxy,
                        float* score, float* desc, uint8_t* desc_bin) {
    int rc = extract_check(c, img, H, W, stride, B, Kmax, n, kxy, score, desc);
    if (rc) return rc;
    const size_t K = (size_t)B * Kmax;
    uint8_t *d_img, *d_b; int32_t *d_n, *d_k; float *d_s, *d_d;
    HostIo io(c, HostIo::PINNED);
    io.image(d_img, (const uint8_t*)img, (size_t)W * px, (size_t)B * H, (size_t)stride * px);
    io.out(d_n, n, B); io.out(d_k, kxy, K * 2); io.out(d_s, score, K);
    // descriptors in rfe_host_malloc'ed memory (the class shims' tensors are): the DMA engine writes them where the caller wants them
    io.out(d_d, desc, K * 256, true);
    io.out_opt(d_b, desc_bin, K * 256);
    if ((rc = io.upload())) return rc;
    if ((rc = ensure_ws(c, &c->ws_sp, &c->ws_sp_bytes, sp_ws_bytes(B, H, W)))) return rc;   // before the key is formed: a capture must not allocate
    int thr_bits; memcpy(&thr_bits, &thr, 4);
    const std::string key = px == 1 ? host_graph_key(c, "xu8", {H, W, B, Kmax, thr_bits, desc_bin != nullptr}) : host_graph_key(c, "xf32", {H, W, B, Kmax, thr_bits});
    if ((rc = run_host_graph(c, c->g_extract, key, [&] { return sp_forward(c, d_img, H, W, W, B, Kmax, thr, d_n, d_k, d_s, d_d, d_b, px == 4); }))) return rc;
    return io.download();
}

extern "C" int rfe_extract_u8(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int Kmax, float thr,
                              int32_t* n, int32_t* kxy, float* score, float* desc) {
    return extract_host(c, img, 1, H, W, stride, B, Kmax, thr, n, kxy, score, desc, nullptr);
}
extern "C" int rfe_extract_u8_bin(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int Kmax, float thr,
                                  int32_t* n, int32_t* kxy, float* score, float* desc, uint8_t* desc_bin) {
    return extract_host(c, img, 1, H, W, stride, B, Kmax, thr, n, kxy, score, desc, desc_bin);
}
extern "C" int rfe_extract_f32(rfe_ctx* c, const float* img, int H, int W, int stride, int B, int Kmax, float thr,
                               int32_t* n, int32_t* kxy, float* score, float* desc) {
    return extract_host(c, img, 4, H, W, stride, B, Kmax, thr, n, kxy, score, desc, nullptr);
}

// =====================================================================================
// SuperPoint on a scale pyramid: the level chain on the side stream behind level 0's SuperPoint, every level through
// sp_forward into per-level staging (ws_pyr: sp_forward carves ws_sp from offset 0 on every call), one merge launch
// =====================================================================================
extern "C" int rfe_pyramid_geometry(int H, int W, int nlevels, float scale_factor, int32_t* level_h, int32_t* level_w, float* level_scale) {
    return pyramid_geometry(H, W, nlevels, scale_factor, level_h, level_w, level_scale);
}

namespace rfe {

int pyr_check(rfe_ctx* c, int H, int W, int stride, int B, int L, float sf, const int32_t* kmax, PyrPlan& P) {
    if (!c) return RFE_ERR_INVALID;
    if (!c->has_sp) return fail(c, RFE_ERR_NO_WEIGHTS, "SuperPoint weights not loaded (rfe_load_weights / rfe_set_weights)");
    if (L < 1 || L > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, "extract_pyramid: nlevels must be in 1..16");
    if (L > 1 && !(sf > 1.0f && sf <= 4.0f)) return fail(c, RFE_ERR_INVALID, "extract_pyramid: scale_factor must be in (1, 4] when nlevels > 1");
    if (H < 8 || W < 8 || B < 1 || stride < W) return fail(c, RFE_ERR_INVALID, "extract_pyramid: H and W must be at least 8, B > 0, stride >= W");
    if (!kmax) return fail(c, RFE_ERR_INVALID, "extract_pyramid: null pointer");
    P.L = L; P.Ktot = 0;
    for (int l = 0; l < L; ++l) {
        if (kmax[l] < 0 || kmax[l] > 4096) return fail(c, RFE_ERR_INVALID, "extract_pyramid: every kmax[l] must be in 0..4096");
        P.kmax[l] = kmax[l]; P.Ktot += kmax[l];
    }
    if (P.Ktot == 0) return fail(c, RFE_ERR_INVALID, "extract_pyramid: every kmax[l] is 0");
    if (pyramid_geometry(H, W, L, sf, P.h, P.w, P.s) != RFE_OK) return fail(c, RFE_ERR_INVALID, "extract_pyramid: a level rounds to zero pixels");
    P.frame = 0;
    for (int l = 0; l < L; ++l) {
        P.off[l] = P.frame; P.frame += (size_t)P.h[l] * P.w[l];
        P.run[l] = P.kmax[l] > 0 && P.h[l] >= 8 && P.w[l] >= 8;
    }
    return RFE_OK;
}

// ws_pyr: the internal level images (own_levels: the caller passed none) and every run level's SuperPoint staging
struct PyrStage { uint8_t* levels; int32_t *n[RFE_MAX_LEVELS], *kxy[RFE_MAX_LEVELS]; float *sc[RFE_MAX_LEVELS], *desc[RFE_MAX_LEVELS]; };
static void pyr_layout(Bump& a, const PyrPlan& P, int B, bool own_levels, PyrStage& st) {
    st.levels = own_levels ? a.take<uint8_t>((size_t)B * P.frame) : nullptr;
    for (int l = 0; l < P.L; ++l) {
        if (!P.run[l]) continue;
        st.n[l] = a.take<int32_t>((size_t)B); st.kxy[l] = a.take<int32_t>((size_t)B * P.kmax[l] * 2);
        st.sc[l] = a.take<float>((size_t)B * P.kmax[l]); st.desc[l] = a.take<float>((size_t)B * P.kmax[l] * 256);
    }
}

// Every allocation of the call happens here// Every allocation of the call happens here, before the first kernel is enqueued (ensure_ws synchronises and frees when it grows):
// ws_sp for the largest level, ws_pyr for the internal level images (own_levels) + staging, the tables of this geometry, sp_cnt.
int pyr_prepare(rfe_ctx* c, int H, int W, int B, float sf, const PyrPlan& P, bool own_levels) {
    int rc;
    if ((rc = ensure_ws(c, &c->ws_sp, &c->ws_sp_bytes, sp_ws_bytes(B, H, W)))) return rc;
    PyrStage st;
    if ((rc = ensure_ws(c, &c->ws_pyr, &c->ws_pyr_bytes, layout_bytes([&](Bump& a) { pyr_layout(a, P, B, own_levels, st); })))) return rc;
    if (!c->sp_cnt) { RFE_HIP(c, hipMalloc((void**)&c->sp_cnt, 8 * sizeof(int32_t))); c->sp_cnt_dirty = true; }
    int sf_bits; memcpy(&sf_bits, &sf, 4);
    const std::string key = std::to_string(H) + "x" + std::to_string(W) + "|" + std::to_string(P.L) + "|" + std::to_string(P.L > 1 ? sf_bits : 0);
    if (P.L > 1 && key != c->ptab_key) {
        std::vector<int2> tab;
        pyramid_tables(P.L, P.h, P.w, tab, c->ptab_off);
        c->ptab_key.clear();
        const void* before = c->ws_ptab;
        if ((rc = ensure_ws(c, &c->ws_ptab, &c->ws_ptab_bytes, tab.size() * sizeof(int2)))) return rc;
        if (before == c->ws_ptab) RFE_HIP(c, hipStreamSynchronize(c->stream));   // earlier calls may still read the old tables
        RFE_HIP(c, hipMemcpy(c->ws_ptab, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice));
        c->ptab_key = key;
    }
    return RFE_OK;
}

// img: level 0 (caller's pitch); lv: the level buffer [B, P.frame] (caller's or ws_pyr's); outputs device pointers
// img_frame: bytes from frame b to b + 1 of img (0 = stride * H)
int pyr_forward(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, const PyrPlan& P, float thr, uint8_t* lv, bool copy_level0,
                int32_t* n, int32_t* level_n, float* kpts, int32_t* octave, float* score, float* desc, long long img_frame) {
    if (img_frame == 0) img_frame = (long long)stride * H;
    hipStream_t s = c->stream;
    // the level chain runs on the side stream, concurrently with level 0's backbone; with events around every stage (full profiling
    // pass) it runs at the front of the main stream, so that the stage times stay clean
    const bool side = !(c->prof && c->prof_filter.empty());
    hipStream_t sc = side ? c->side_stream : s;
    if (side) { RFE_HIP(c, hipEventRecord(c->ev_fork, s)); RFE_HIP(c, hipStreamWaitEvent(sc, c->ev_fork, 0)); }
    { ProfScope p(c, "sp_pyramid", sc);
      if (copy_level0) launch_pyr_resample(sc, img, img_frame, stride, H, W, lv, (long long)P.frame, H, W, B, nullptr, nullptr);
      const int2* tab = (const int2*)c->ws_ptab;
      for (int l = 1; l < P.L; ++l) {
          const uint8_t* src = l == 1 ? img : lv + P.off[l - 1];
          const long long src_frame = l == 1 ? img_frame : (long long)P.frame;
          const int src_stride = l == 1 ? stride : P.w[l - 1];
          launch_pyr_resample(sc, src, src_frame, src_stride, P.h[l - 1], P.w[l - 1], lv + P.off[l], (long long)P.frame, P.h[l], P.w[l], B,
                              tab + c->ptab_off[l], tab + c->ptab_off[l] + P.w[l]);
      } }
    if (side) RFE_HIP(c, hipEventRecord(c->ev_pyr, sc));
    PyrMergeArgs m;
    memset(&m, 0, sizeof(m));
    m.L = P.L; m.Ktot = P.Ktot;
    PyrStage st;
    Bump a(c->ws_pyr);
    pyr_layout(a, P, B, lv == (uint8_t*)c->ws_pyr, st);
    int rc;
    bool joined = !side;
    for (int l = 0; l < P.L; ++l) {
        m.kmax[l] = P.kmax[l]; m.scale[l] = P.s[l];
        if (!P.run[l]) continue;
        int32_t* ln = st.n[l]; int32_t* lk = st.kxy[l]; float* ls = st.sc[l]; float* ld = st.desc[l];
        if (l >= 1 && !joined) { RFE_HIP(c, hipStreamWaitEvent(s, c->ev_pyr, 0)); joined = true; }   // levels >= 1 read the chain's output
        if (l == 0) rc = sp_forward(c, img, H, W, stride, B, P.kmax[0], thr, ln, lk, ls, ld, nullptr, false, img_frame);
        else rc = sp_forward(c, lv + P.off[l], P.h[l], P.w[l], P.w[l], B, P.kmax[l], thr, ln, lk, ls, ld, nullptr, false, (long long)P.frame);
        if (rc) return rc;
        m.n[l] = ln; m.kxy[l] = lk; m.sc[l] = ls; m.desc_l[l] = ld;
    }
    // a pyramid whose levels >= 1 all yield nothing still joins the chain before returning (the caller may read `levels`)
    if (!joined) RFE_HIP(c, hipStreamWaitEvent(s, c->ev_pyr, 0));
    m.n_out = n; m.level_n = level_n; m.kpts = kpts; m.octave = octave; m.score = score; m.desc = desc;
    { ProfScope p(c, "sp_merge"); launch_pyr_merge(s, m, B); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

}  // namespace rfe

// the argument check of both pyramid entries; fills the plan
static int pyr_entry_check(rfe_ctx* c, const void* img, int H, int W, int stride, int B, int nlevels, float scale_factor, const int32_t* kmax, const void* n,
                           const void* kpts, const void* octave, const void* score, const void* desc, PyrPlan& P) {
    int rc = pyr_check(c, H, W, stride, B, nlevels, scale_factor, kmax, P);
    if (rc) return rc;
    if (!img || !n || !kpts || !octave || !score || !desc) return fail(c, RFE_ERR_INVALID, "extract_pyramid: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    return RFE_OK;
}

extern "C" int rfe_extract_pyramid_u8_dev(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int nlevels, float scale_factor,
                                          const int32_t* kmax, float thr, int32_t* n, int32_t* level_n, float* kpts, int32_t* octave,
                                          float* score, float* desc, uint8_t* levels) {
    PyrPlan P;
    int rc = pyr_entry_check(c, img, H, W, stride, B, nlevels, scale_factor, kmax, n, kpts, octave, score, desc, P);
    if (rc) return rc;
    if ((rc = pyr_prepare(c, H, W, B, scale_factor, P, levels == nullptr))) return rc;
    return pyr_forward(c, img, H, W, stride, B, P, thr, levels ? levels : (uint8_t*)c->ws_pyr, levels != nullptr, n, level_n, kpts, octave,
                       score, desc);
}

extern "C" int rfe_extract_pyramid_u8(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int nlevels, float scale_factor,
                                      const int32_t* kmax, float thr, int32_t* n, int32_t* level_n, float* kpts, int32_t* octave,
                                      float* score, float* desc, uint8_t* levels) {
    PyrPlan P;
    int rc = pyr_entry_check(c, img, H, W, stride, B, nlevels, scale_factor, kmax, n, kpts, octave, score, desc, P);
    if (rc) return rc;
    // one pinned block each way: [img] in; [n | level_n | kpts | octave | score | desc | levels] out (desc DMA'd straight into an
    // rfe_host_malloc block, as rfe_extract_u8 does)
    const size_t K = (size_t)B * P.Ktot;
    uint8_t *d_img, *d_v; int32_t *d_n, *d_ln, *d_o; float *d_k, *d_s, *d_d;
    HostIo io(c, HostIo::PINNED);
    io.image(d_img, img, (size_t)W, (size_t)B * H, (size_t)stride);
    io.out(d_n, n, B); io.out(d_ln, level_n, (size_t)B * nlevels); io.out(d_k, kpts, K * 2); io.out(d_o, octave, K); io.out(d_s, score, K);
    io.out(d_d, desc, K * 256, true);
    io.out_opt(d_v, levels, (size_t)B * P.frame);
    if ((rc = pyr_prepare(c, H, W, B, scale_factor, P, levels == nullptr))) return rc;
    if ((rc = io.upload())) return rc;
    if ((rc = pyr_forward(c, d_img, H, W, W, B, P, thr, d_v ? d_v : (uint8_t*)c->ws_pyr, d_v != nullptr, d_n, d_ln, d_k, d_o, d_s, d_d))) return rc;
    return io.download();
}
