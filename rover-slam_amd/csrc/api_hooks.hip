// api_hooks.hip -- C ABI of librover_fe.so: the kernel-level test hooks (every rfe_k_*), which drive single kernels and stages of the two
// pipelines through the forward passes' own code.
#include <algorithm>
#include "api_internal.h"

using namespace rfe;

// =====================================================================================
// kernel-level test hooks
// =====================================================================================
extern "C" int rfe_k_conv3x3(rfe_ctx* c, const float* in, int B, int H, int W, int Cin, const float* w, const float* bias,
                             int Cout, int relu, int pool, float* out) {
    if (!c) return RFE_ERR_INVALID;
    if ((Cin != 16 && Cin != 32 && Cin != 64 && Cin != 128) || (Cout % 64)) return fail(c, RFE_ERR_INVALID, "k_conv3x3: Cin in {16,32,64,128}, Cout % 64 == 0");
    RFE_HIP(c, hipSetDevice(c->device));
    std::vector<float> packed;
    pack_conv3x3_weights(w, Cin, Cout, pool != 0, packed);
    float *dw, *db;
    int rc = ws_carve(c, &c->ws_tmp, &c->ws_tmp_bytes, [&](Bump& a) { dw = a.take<float>(packed.size()); db = a.take<float>(Cout); });
    if (rc) return rc;
    RFE_HIP(c, hipMemcpyAsync(dw, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, c->stream));
    RFE_HIP(c, hipMemcpyAsync(db, bias, (size_t)Cout * 4, hipMemcpyHostToDevice, c->stream));
    launch_conv3x3(c->stream, in, B, H, W, Cin, dw, db, Cout, relu != 0, pool != 0, out, 0);
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

extern "C" int rfe_k_linear(rfe_ctx* c, const float* a, int M, int K, const float* w, const float* bias, int N, int relu,
                            float* out) {
    if (!c) return RFE_ERR_INVALID;
    if (K % 32) return fail(c, RFE_ERR_INVALID, "k_linear: K % 32 == 0 required");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dw, *db;
    int rc = ws_carve(c, &c->ws_tmp, &c->ws_tmp_bytes, [&](Bump& a) { dw = a.take<float>((size_t)N * K); db = a.take<float>(N); });
    if (rc) return rc;
    RFE_HIP(c, hipMemcpyAsync(dw, w, (size_t)N * K * 4, hipMemcpyHostToDevice, c->stream));
    if (bias) RFE_HIP(c, hipMemcpyAsync(db, bias, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    GemmArgs g = gemm_plain(a, K, dw, K, bias ? db : nullptr, out, N, M, N, K);
    g.relu = relu;
    launch_gemm_nt(c->stream, g);
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

extern "C" int rfe_k_scoremap(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, float* scoremap,
                              float* nms, float* descmap) {
    int rc = sp_check(c, H, W, B, 1);
    if (rc) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    SpBuffers b;
    bool forked;
    if ((rc = sp_forward_maps(c, img, H, W, stride, B, b, true, forked, false, 0, 0.0005f, true))) return rc;   // sp_cnt stays dirty: zeroed before the next forward
    const size_t hw = (size_t)B * (H / 8 * 8) * (W / 8 * 8);   // maps are on the score-map frame: [B, 8*(H/8), 8*(W/8)]
    if (scoremap) RFE_HIP(c, hipMemcpyAsync(scoremap, b.smap, hw * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nms) RFE_HIP(c, hipMemcpyAsync(nms, b.nmap, hw * 4, hipMemcpyDeviceToDevice, c->stream));
    if (descmap) RFE_HIP(c, hipMemcpyAsync(descmap, b.dmap, hw / 64 * 256 * 4, hipMemcpyDeviceToDevice, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

// The sparse descriptor head (sp_desc_rows, the forward's own: cell list, row gather, convDa and convDb on rows, L2 norm) behind the backbone of B frames,
// for CALLER-PROVIDED keypoints n [B], kxy [B,Kmax,2] (device) -- so the tests place footprints on the map's edges and beyond them, whatever B.  poison != 0
// fills the patch buffer, both activation buffers and the row tables with 0xFFFFFFFF words (NaN) between the backbone and the head: nothing past the live
// rows may reach a result.  Outputs (device, each may be null): cell_row [B,Hc*Wc] (row within the frame or -1), count [B], rows [B*cap,256] with
// cap = min(4 Kmax, Hc Wc): the frames' live rows back to back (frame b's from row count[0] + .. + count[b-1] on; only those sum(count) rows are
// meaningful), desc [B,Kmax,256] = desc_sample_kernel through cell_row.
extern "C" int rfe_k_sparse_desc(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int Kmax, const int32_t* n, const int32_t* kxy, int poison,
                                 int32_t* cell_row, int32_t* count, float* rows, float* desc) {
    int rc = sp_check(c, H, W, B, Kmax);
    if (rc) return rc;
    if (!img || !n || !kxy || stride < W) return fail(c, RFE_ERR_INVALID, "k_sparse_desc: null pointer or stride < W");
    RFE_HIP(c, hipSetDevice(c->device));
    SpBuffers b;
    bool forked;
    if ((rc = sp_forward_maps(c, img, H, W, stride, B, b, true, forked, false, 0, 0.0005f, false, false))) return rc;   // sp_cnt stays dirty: zeroed before the next forward
    const int Hc = H / 8, Wc = W / 8, cap = sp_desc_cap(Kmax, Hc, Wc);
    const size_t cells = (size_t)B * Hc * Wc, live = (size_t)B * cap;
    hipStream_t s = c->stream;
    if (poison) {
        const struct { void* p; size_t words; } fill[] = {{b.patch, live * 1152}, {b.da, cells * 256}, {b.dmap, cells * 256}, {b.cell_row, cells},
                                                          {b.row_cell, cells}, {b.cell_cnt, (size_t)2 * B + 1}};
        for (const auto& f : fill) RFE_HIP(c, hipMemsetD32Async((hipDeviceptr_t)f.p, -1, f.words, s));
    }
    if ((rc = sp_desc_rows(c, b, B, Hc, Wc, Kmax, n, kxy))) return rc;
    if (desc) launch_desc_sample(s, b.dmap, B, Hc, Wc, 8 * Hc, 8 * Wc, n, kxy, Kmax, desc, nullptr, b.cell_row, b.cell_cnt + B);
    RFE_HIP(c, hipGetLastError());
    if (cell_row) RFE_HIP(c, hipMemcpyAsync(cell_row, b.cell_row, cells * 4, hipMemcpyDeviceToDevice, s));
    if (count) RFE_HIP(c, hipMemcpyAsync(count, b.cell_cnt, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (rows) RFE_HIP(c, hipMemcpyAsync(rows, b.dmap, live * 256 * 4, hipMemcpyDeviceToDevice, s));
    RFE_HIP(c, hipStreamSynchronize(s));
    return RFE_OK;
}

// keypoint selection alone on a caller-provided post-NMS map [B,H,W] (device): candidates > thr, the top Kmax by (score descending, pixel
// index ascending) or row-major order, through the forward's own launch_select -- so B selects the form (rank-all up to 4 frames, radix
// select + rank sort above).  Lets the tests drive candidate counts and tie patterns no network output produces.
extern "C" int rfe_k_select(rfe_ctx* c, const float* nms, int B, int H, int W, int Kmax, float thr, int topk_always, int32_t* n, int32_t* kxy,
                            float* score) {
    int rc = sp_check(c, H, W, B, Kmax);
    if (rc) return rc;
    if (!nms || !n || !kxy || !score) return fail(c, RFE_ERR_INVALID, "k_select: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    SpBuffers b;
    if ((rc = sp_carve(c, B, H, W, b))) return rc;
    launch_select(c->stream, nms, B, H, W, Kmax, thr, b.cand_score, b.cand_idx, n, kxy, score, (int32_t*)b.ss, topk_always != 0, b.sel_keys, b.sel_n);
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

// the same selection through the latency regime's key form (B <= 4): the map's candidates are appended as 64-bit keys in a scrambled order by a helper
// kernel (one atomic per candidate -- the order sp_tail_lat_kernel's workgroups leave is just as arbitrary), then select_rankall_keys_kernel ranks them
extern "C" int rfe_k_select_keys(rfe_ctx* c, const float* nms, int B, int H, int W, int Kmax, float thr, int topk_always, int32_t* n, int32_t* kxy,
                                 float* score) {
    int rc = sp_check(c, H, W, B, Kmax);
    if (rc) return rc;
    if (!nms || !n || !kxy || !score || B > 4) return fail(c, RFE_ERR_INVALID, "k_select_keys: null pointer or more than four frames");
    RFE_HIP(c, hipSetDevice(c->device));
    SpBuffers b;
    if ((rc = sp_carve(c, B, H, W, b))) return rc;
    if (!c->sp_cnt) RFE_HIP(c, hipMalloc((void**)&c->sp_cnt, 8 * sizeof(int32_t)));
    RFE_HIP(c, hipMemsetAsync(c->sp_cnt, 0, 8 * sizeof(int32_t), c->stream));
    launch_keys_from_map(c->stream, nms, B, H * W, thr, (unsigned long long*)b.cand_score, c->sp_cnt);
    launch_select_keys(c->stream, (const unsigned long long*)b.cand_score, c->sp_cnt, B, H, W, Kmax, topk_always != 0, n, kxy, score);
    c->sp_cnt_dirty = false;
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    int32_t left[8];
    RFE_HIP(c, hipMemcpy(left, c->sp_cnt, sizeof(left), hipMemcpyDeviceToHost));
    for (int q = 0; q < 8; ++q) if (left[q] != 0) return fail(c, RFE_ERR_HIP, "k_select_keys: the ranking kernel did not leave the candidate counters at zero");
    return RFE_OK;
}

// x + ffn([x | second]) of one LightGlue block with the loaded weights (unfolded W1: `second` is the attention message), through
// the same lg_ffn the forward uses -- so `rows` selects the path: >= 32768 rows take the 128x256 tiles with the LayerNorm + GELU
// fused across ffn.0 / ffn.3, a few thousand rows the 64-row tiles with the stand-alone lg_ln_gelu pass.
extern "C" int rfe_k_lightglue_ffn(rfe_ctx* c, int layer, int cross, const float* x, const float* second, int rows, float* out) {
    int rc = lg_check(c, 1, 4, 4);
    if (rc) return rc;
    if (layer < 0 || layer >= LG_LAYERS || rows <= 0 || !x || !second || !out) return fail(c, RFE_ERR_INVALID, "k_lightglue_ffn: bad argument");
    RFE_HIP(c, hipSetDevice(c->device));
    const int L = 1024, P = (rows + 2 * L - 1) / (2 * L);
    LgBuffers b;
    if ((rc = lg_carve(c, P, L, b))) return rc;
    const LgLayerDev& Lw = c->lg.L[layer];
    RFE_HIP(c, hipMemcpyAsync(out, x, (size_t)rows * 1024, hipMemcpyDeviceToDevice, c->stream));
    if (cross) lg_ffn(c, b, out, second, rows, Lw.cw1, Lw.cb1, Lw.clng, Lw.clnb, Lw.cw2, Lw.cb2);
    else lg_ffn(c, b, out, second, rows, Lw.w1, Lw.b1, Lw.lng, Lw.lnb, Lw.w2, Lw.b2);
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

extern "C" int rfe_k_attention(rfe_ctx* c, const float* q, const float* k, const float* v, int ld, float* out, int nseq, int Lq, int Lk,
                               const int32_t* qlen, const int32_t* klen, const int32_t* kv_map, const float* rope) {
    if (!c) return RFE_ERR_INVALID;
    if (!q || !k || !v || !out || nseq <= 0 || Lq <= 0 || Lk <= 0 || ld < 256) return fail(c, RFE_ERR_INVALID, "k_attention: bad argument");
    RFE_HIP(c, hipSetDevice(c->device));
    float* part = nullptr;
    const size_t pb = lg_attention_part_bytes(nseq, Lq);
    if (pb) RFE_HIP(c, hipMalloc((void**)&part, pb));
    launch_lg_attention(c->stream, q, k, v, ld, out, nseq, Lq, Lk, qlen, klen, kv_map, part, rope, c->opt_lg_fp16x2);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (part) (void)hipFree(part);
    RFE_HIP(c, e);
    return RFE_OK;
}

// Both directions of one cross block, through the forward's own lg_cross_attention, on caller-provided [qk | v] rows in the side-major layout.  form 0: what
// the forward would choose at (P, L); 1: the shared-logit form at any shape; 2: the generic form.  The whole LightGlue workspace, the logit scratch included, is filled
// with 0xFFFFFFFF words (NaN) before the launches: nothing but what a call writes itself may reach its result.
extern "C" int rfe_k_cross_attention(rfe_ctx* c, const float* qk_v, int ld, float* out, int P, int L, const int32_t* lens, int form) {
    if (!c) return RFE_ERR_INVALID;
    if (!qk_v || !out || !lens || P <= 0 || L < 4 || L > 4096 || (L % 4) || ld < 512 || (ld % 4) || form < 0 || form > 2)
        return fail(c, RFE_ERR_INVALID, "k_cross_attention: null pointer, P <= 0, L not a multiple of 4 in [4, 4096], ld < 512 or not a multiple of 4, or form outside 0..2");
    RFE_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> hl((size_t)2 * P), map((size_t)2 * P);   // the kernels trust the lengths (lg_stage clamps them for the forward)
    RFE_HIP(c, hipMemcpy(hl.data(), lens, hl.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : hl) if (v < 0 || v > L) return fail(c, RFE_ERR_INVALID, "k_cross_attention: a length outside [0, L]");
    for (int i = 0; i < 2 * P; ++i) map[i] = i < P ? i + P : i - P;
    LgBuffers b;
    int rc = lg_carve_as(c, P, L, b, form == 1 || (form == 0 && lg_cross_shared(c, P, L)), [](Bump&) {});
    if (rc) return rc;
    hipStream_t s = c->stream;
    RFE_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->ws_lg, -1, c->ws_lg_bytes / 4, s));   // the whole LightGlue workspace, the logit scratch included
    RFE_HIP(c, hipMemcpyAsync(b.lens, lens, (size_t)2 * P * 4, hipMemcpyDeviceToDevice, s));
    RFE_HIP(c, hipMemcpyAsync(b.kvmap, map.data(), (size_t)2 * P * 4, hipMemcpyHostToDevice, s));
    lg_cross_attention(c, b, qk_v, ld, out, P, L);
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(s));
    return RFE_OK;
}

extern "C" int rfe_k_set_lightglue_tap(rfe_ctx* c, int pair, float* x0, float* x1, float* scores) {
    if (!c) return RFE_ERR_INVALID;
    if (pair < 0) { c->tap.armed = false; return RFE_OK; }
    c->tap.armed = true; c->tap.pair = pair; c->tap.x0 = x0; c->tap.x1 = x1; c->tap.scores = scores;
    return RFE_OK;
}

// projection + attention of layer `layer`'s self block on caller-provided token rows x [nseq * L, 256] with the rotary table csn [nseq * L, 32] (cos, sin),
// through the forward's own lg_self_qkv_attention -- so nseq * L selects the path (throughput: rotary in gemm.hip's epilogue + lg_attention_dma_kernel;
// one / few pairs: gemm_lat.hip + lg_attention_lat_kernel; shapes neither takes: plain epilogue + rotary on load).  qkv_out [nseq * L, 768], ctx_out [nseq * L, 256];
// *qk_rotated = 1 when qkv_out's q | k columns are rotated.
extern "C" int rfe_k_lightglue_self_attention(rfe_ctx* c, int layer, const float* x, const float* csn, const int32_t* lens, int nseq, int L,
                                              float* qkv_out, float* ctx_out, int32_t* qk_rotated) {
    int rc = lg_check(c, 1, 4, 4);
    if (rc) return rc;
    if (layer < 0 || layer >= LG_LAYERS || nseq <= 0 || L <= 0 || (L % 4) || !x || !csn || !lens) return fail(c, RFE_ERR_INVALID, "k_lightglue_self_attention: bad argument");
    RFE_HIP(c, hipSetDevice(c->device));
    const int P = (nseq + 1) / 2;
    LgBuffers b;
    if ((rc = lg_carve(c, P, L, b))) return rc;
    const bool rot = lg_self_qkv_attention(c, b, c->lg.L[layer], x, csn, lens, nseq, L);
    RFE_HIP(c, hipGetLastError());
    if (qkv_out) RFE_HIP(c, hipMemcpyAsync(qkv_out, b.qkv, (size_t)nseq * L * 768 * 4, hipMemcpyDeviceToDevice, c->stream));
    if (ctx_out) RFE_HIP(c, hipMemcpyAsync(ctx_out, b.ctx, (size_t)nseq * L * 256 * 4, hipMemcpyDeviceToDevice, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    if (qk_rotated) *qk_rotated = rot ? 1 : 0;
    return RFE_OK;
}

// LightGlue's assignment stage alone (lg_assign_stage, the forward's own) on caller-provided similarities, token states and matchability head: needs a
// ctx and no weights.  Every buffer the stage leaves behind, the match list and the score dump are pre-filled with the 32-bit word `sentinel`, so the
// caller sees exactly which words the stage wrote; (P, L) selects the form as inside a match call.
extern "C" int rfe_k_lightglue_assign(rfe_ctx* c, const float* sim, const float* x, const float* wm, const float* bm, const int32_t* lens, int P, int L,
                                      float thr, int cap, int scores_pair, int32_t sentinel, float* z, float* rowlse, float* collse, float* mx0,
                                      int32_t* a0, int32_t* a1, int32_t* S, int32_t* pairs, float* ms, float* scores) {
    if (!c) return RFE_ERR_INVALID;
    if (!sim || !x || !wm || !bm || !lens || P <= 0 || L < 4 || L > 4096 || (L % 4) || cap <= 0 || scores_pair >= P)
        return fail(c, RFE_ERR_INVALID, "k_lightglue_assign: null input, P <= 0, L not a multiple of 4 in [4, 4096], cap <= 0 or scores_pair >= P");
    RFE_HIP(c, hipSetDevice(c->device));
    {   // the kernels trust the lengths (lg_stage clamps them for the forward): refuse what would index past a padded sequence
        std::vector<int32_t> hl((size_t)2 * P);
        RFE_HIP(c, hipMemcpy(hl.data(), lens, hl.size() * 4, hipMemcpyDeviceToHost));
        for (int32_t v : hl) if (v < 0 || v > L) return fail(c, RFE_ERR_INVALID, "k_lightglue_assign: a length outside [0, L]");
    }
    const size_t PL = (size_t)P * L, n_scores = scores ? (scores_pair < 0 ? PL * L : (size_t)L * L) : 0;
    LgBuffers b;
    float *dsc = nullptr, *dms; int32_t *dS, *dp;
    int rc = lg_carve(c, P, L, b, [&](Bump& a) {
        dS = a.take<int32_t>(P); dp = a.take<int32_t>((size_t)P * cap * 2); dms = a.take<float>((size_t)P * cap);
        if (n_scores) dsc = a.take<float>(n_scores);
    });
    if (rc) return rc;
    hipStream_t s = c->stream;
    RFE_HIP(c, hipMemcpyAsync(b.sim, sim, PL * L * 4, hipMemcpyDeviceToDevice, s));
    RFE_HIP(c, hipMemcpyAsync(b.x, x, 2 * PL * 1024, hipMemcpyDeviceToDevice, s));
    RFE_HIP(c, hipMemcpyAsync(b.lens, lens, (size_t)2 * P * 4, hipMemcpyDeviceToDevice, s));
    const struct { void* p; size_t words; } fill[] = {{b.z, 2 * PL}, {b.rowlse, PL}, {b.collse, PL}, {b.mx0, PL}, {b.a0, PL}, {b.a1, PL},
                                                      {dS, (size_t)P}, {dp, (size_t)P * cap * 2}, {dms, (size_t)P * cap}, {dsc, n_scores}};
    for (const auto& f : fill)
        if (f.words) RFE_HIP(c, hipMemsetD32Async((hipDeviceptr_t)f.p, sentinel, f.words, s));
    lg_assign_stage(s, b, P, L, thr, cap, dS, dp, dms, dsc, scores_pair, wm, bm);
    RFE_HIP(c, hipGetLastError());
    const struct { void* dst; const void* src; size_t words; } out[] = {{z, b.z, 2 * PL}, {rowlse, b.rowlse, PL}, {collse, b.collse, PL}, {mx0, b.mx0, PL},
                                                                       {a0, b.a0, PL}, {a1, b.a1, PL}, {S, dS, (size_t)P}, {pairs, dp, (size_t)P * cap * 2},
                                                                       {ms, dms, (size_t)P * cap}, {scores, dsc, n_scores}};
    for (const auto& o : out)
        if (o.dst && o.words) RFE_HIP(c, hipMemcpyAsync(o.dst, o.src, o.words * 4, hipMemcpyDeviceToDevice, s));
    RFE_HIP(c, hipStreamSynchronize(s));
    return RFE_OK;
}

// CheckHomography (model 0; H12 is the cofactor inverse of M) or CheckFundamental (model 1) of ONE model M [9] over pts [n,4] = u1 v1 u2 v2:
// contrib [n] what each match adds to the score, inl [n] its flag.  HOST pointers, synchronous; n <= 4096.
extern "C" int rfe_k_two_view_check(rfe_ctx* c, int model, const float* M, float sigma, const float* pts, int n, float* contrib, uint8_t* inl) {
    if (!c) return RFE_ERR_INVALID;
    if (!M || !pts || !contrib || !inl || n < 0 || n > 4096 || model < 0 || model > 1) return fail(c, RFE_ERR_INVALID, "k_two_view_check: bad argument");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dM, *dp, *dc; uint8_t* di;
    HostIo io(c, HostIo::DIRECT);
    io.in(dM, M, (size_t)9); io.in(dp, pts, (size_t)n * 4); io.out(dc, contrib, (size_t)n); io.out(di, inl, (size_t)n);
    int rc = io.upload();
    if (rc) return rc;
    const float s2 = sigma * sigma;
    launch_two_view_hook_check(c->stream, model, dM, 1.f / s2, dp, n, dc, di);
    RFE_HIP(c, hipGetLastError());
    return io.download();
}

// CheckRT of ONE motion hypothesis Rt [12] = R row-major | t over pts [n,4] with K = (fx, fy, cx, cy) and th2: code [n] (0 not counted, 1
// counted without vbGood, 2 counted and vbGood), cosp [n], p3d [n,3].  HOST pointers, synchronous; n <= 4096.
extern "C" int rfe_k_two_view_check_rt(rfe_ctx* c, const float* Rt, const float* K4, float th2, const float* pts, int n, uint8_t* code, float* cosp,
                                       float* p3d) {
    if (!c) return RFE_ERR_INVALID;
    if (!Rt || !K4 || !pts || !code || !cosp || !p3d || n < 0 || n > 4096) return fail(c, RFE_ERR_INVALID, "k_two_view_check_rt: bad argument");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dR, *dp, *dc, *dx; uint8_t* dk;
    HostIo io(c, HostIo::DIRECT);
    io.in(dR, Rt, (size_t)12); io.in(dp, pts, (size_t)n * 4); io.out(dk, code, (size_t)n); io.out(dc, cosp, (size_t)n); io.out(dx, p3d, (size_t)n * 3);
    int rc = io.upload();
    if (rc) return rc;
    launch_two_view_hook_check_rt(c->stream, dR, K4[0], K4[1], K4[2], K4[3], th2, dp, n, dk, dc, dx);
    RFE_HIP(c, hipGetLastError());
    return io.download();
}

extern "C" int rfe_k_lightglue_taps(rfe_ctx* c, const float* k0n, const float* k1n, const float* d0, const float* d1,
                                    int M, int N, float* x0, float* x1, float* scores) {
    int rc = lg_check(c, 1, M, N);
    if (rc) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    const int L = ((std::max(M, N) + 3) / 4) * 4, cap = std::min(M, N);
    LgBuffers b;
    float *sc, *dms; int32_t *dm, *dn, *dS, *dp;
    if ((rc = lg_carve(c, 1, L, b, [&](Bump& a) {
             sc = a.take<float>((size_t)L * L);
             dm = a.take<int32_t>(1); dn = a.take<int32_t>(1); dS = a.take<int32_t>(1);
             dp = a.take<int32_t>((size_t)cap * 2); dms = a.take<float>(cap);
         }))) return rc;
    RFE_HIP(c, hipMemcpyAsync(dm, &M, 4, hipMemcpyHostToDevice, c->stream));
    RFE_HIP(c, hipMemcpyAsync(dn, &N, 4, hipMemcpyHostToDevice, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    if ((rc = lg_stage(c, b, k0n, k1n, d0, d1, dm, dn, 1, M, N, L))) return rc;
    if ((rc = lg_forward(c, b, 1, L, 0.1f, cap, dS, dp, dms, scores ? sc : nullptr, false, true))) return rc;
    if (x0) RFE_HIP(c, hipMemcpyAsync(x0, b.x, (size_t)M * 1024, hipMemcpyDeviceToDevice, c->stream));
    if (x1) RFE_HIP(c, hipMemcpyAsync(x1, b.x + (size_t)L * 256, (size_t)N * 1024, hipMemcpyDeviceToDevice, c->stream));
    if (scores) RFE_HIP(c, hipMemcpy2DAsync(scores, (size_t)N * 4, sc, (size_t)L * 4, (size_t)N * 4, M, hipMemcpyDeviceToDevice, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

// The float classification of rfe_pose_inertial_optimization behind round `round` (0..3) or its recovery pass (round 4) of n edges at ONE
// camera pose view [12] = Rcw row-major | tcw (doubles), through the device functions the kernel uses.  Every row is an edge;
// outlier_in [n] the flags before (a flagged edge recomputes its error, any other is compared at chi2_in [n]).  code [n]: rounds 0..3 the new
// flag; round 4 bit 0 the flag afterwards, bit 1 the edge counts in nBad.  chi2_out [n] the float compared.  HOST pointers, synchronous.
extern "C" int rfe_k_pose_inertial_classify(rfe_ctx* c, const rfe_pose_inertial_params* P, int mode, int round, const double* view, const float* kpts,
                                            const int32_t* octave, const float* uright, const float* xw, const float* track_depth,
                                            const uint8_t* outlier_in, const float* chi2_in, int n, uint8_t* code, float* chi2_out) {
    if (!c) return RFE_ERR_INVALID;
    if (!P || !view || !kpts || !xw || !track_depth || !outlier_in || !chi2_in || !code || !chi2_out || n < 1 || n > 4096 || round < 0 || round > 4 ||
        (mode != RFE_PIO_LAST_KEYFRAME && mode != RFE_PIO_LAST_FRAME) || P->nlevels < 1 || P->nlevels > RFE_MAX_LEVELS)
        return fail(c, RFE_ERR_INVALID, "k_pose_inertial_classify: bad argument");
    RFE_HIP(c, hipSetDevice(c->device));
    double* dv; float *dk, *du, *dx, *dt, *dci, *dco; int32_t* doct; uint8_t *doi, *dcode;
    HostIo io(c, HostIo::DIRECT);
    io.in(dv, view, (size_t)12); io.in(dk, kpts, (size_t)n * 2); io.in_opt(doct, octave, (size_t)n); io.in_opt(du, uright, (size_t)n);
    io.in(dx, xw, (size_t)n * 3); io.in(dt, track_depth, (size_t)n); io.in(doi, outlier_in, (size_t)n); io.in(dci, chi2_in, (size_t)n);
    io.out(dcode, code, (size_t)n); io.out(dco, chi2_out, (size_t)n);
    int rc = io.upload();
    if (rc) return rc;
    PioArgs a = PioArgs();
    a.kpts = dk; a.octave = doct; a.uright = du; a.xw = dx; a.track_depth = dt; a.chi2 = dco; a.N = n;
    launch_pose_inertial_classify(c->stream, *P, a, dv, mode == RFE_PIO_LAST_FRAME ? 1 : 0, round, doi, dci, dcode);
    RFE_HIP(c, hipGetLastError());
    return io.download();
}
