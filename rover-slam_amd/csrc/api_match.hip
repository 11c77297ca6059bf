// api_match.hip -- C ABI of librover_fe.so: the LightGlue pipeline (forward pass, match entries) and the batched stream mode.
#include <string.h>
#include <algorithm>
#include <vector>
#include "api_internal.h"

using namespace rfe;

// =====================================================================================
// LightGlue pipeline.  Token layout: side-major sequences, seq = side*P + pair, each padded to L.
// =====================================================================================
namespace rfe {

// LightGlue Linears: tolerance-checked, free to use the k-permuted GEMM path (GemmArgs::kperm)
GemmArgs gemm_lg(const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K) {
    GemmArgs g = gemm_plain(A, lda, Bw, ldb, bias, C, ldc, M, N, K);
    g.kperm = 1;
    return g;
}
// A LightGlue Linear whose weight matrix Bw lives in the ctx's weight buffers: with RFE_OPT_LG_FP16X2 on, the fp16 (hi, lo) planes of
// the same matrix ride along and launch_gemm_nt takes the split GEMM for the throughput shapes (gemm_h2.hip)
GemmArgs gemm_lgw(const rfe_ctx* c, const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K) {
    GemmArgs g = gemm_lg(A, lda, Bw, ldb, bias, C, ldc, M, N, K);
    const LgWeightsDev& W = c->lg;
    if (c->opt_lg_fp16x2 && W.h2) {
        if (Bw >= W.blob && Bw < W.blob + LG_COUNT) { g.Bh = W.h2 + (Bw - W.blob); g.Bl = g.Bh + W.n_blob; }
        else if (Bw >= W.extra && Bw < W.extra + W.n_extra) { g.Bh = W.h2 + 2 * W.n_blob + (Bw - W.extra); g.Bl = g.Bh + W.n_extra; }
    }
    return g;
}

void lg_layout(Bump& a, int P, int L, LgBuffers& b, bool shared) {
    const size_t rows = (size_t)2 * P * L;
    b.x = a.take<float>(rows * 256); b.ctx = a.take<float>(rows * 256); b.msg = a.take<float>(rows * 256);
    b.md = a.take<float>(rows * 256);
    b.kn = a.take<float>(rows * 2); b.csn = a.take<float>(rows * 64); b.lnstat = a.take<float>(rows * 32);   // <= 16 partial pairs per row
    b.qkv = a.take<float>(rows * 768); b.h = a.take<float>(rows * 512); b.z = a.take<float>(rows);
    b.slog = shared ? a.take<float>(lg_cross_slog_floats(P, L)) : nullptr;
    b.sim = shared ? b.slog : a.take<float>((size_t)P * L * L);
    b.rowlse = a.take<float>((size_t)P * L); b.collse = a.take<float>((size_t)P * L); b.mx0 = a.take<float>((size_t)P * L);
    b.a0 = a.take<int32_t>((size_t)P * L); b.a1 = a.take<int32_t>((size_t)P * L);
    b.lens = a.take<int32_t>((size_t)2 * P); b.kvmap = a.take<int32_t>((size_t)2 * P);
    { const size_t pb = lg_attention_part_bytes(2 * P, L); b.apart = pb ? a.take<float>(pb / 4) : nullptr; }
}

// scratch of the split-key attention: carved for 2P sequences; a call on fewer sequences (stream mode's per-frame self
// block) may use it whenever its own requirement fits
static float* lg_part(const LgBuffers& b, int nseq, int L) { return (b.apart && lg_attention_part_bytes(nseq, L) > 0) ? b.apart : nullptr; }


void lg_cross_attention(rfe_ctx* c, LgBuffers& b, const float* qk_v, int ld, float* out, int P, int L) {
    if (b.slog) launch_lg_cross_shared(c->stream, qk_v, ld, out, P, L, b.lens, b.slog);
    else launch_lg_attention(c->stream, qk_v, qk_v, qk_v + 256, ld, out, 2 * P, L, L, b.lens, b.lens, b.kvmap, lg_part(b, 2 * P, L), nullptr, c->opt_lg_fp16x2);
}

// x + ffn([x | msg]) in place on x
void lg_ffn(rfe_ctx* c, LgBuffers& b, float* x, const float* second, int rows, const float* w1, const float* b1, const float* g,
            const float* be, const float* w2, const float* b2) {
    hipStream_t s = c->stream;
    // LayerNorm(512) + GELU between the two Linears is fused across them: ffn.0's epilogue leaves per-row partial sums next to the
    // raw h, ffn.3 normalises while it stages its A tiles -- h crosses HBM once in each direction instead of twice (268 MB per block
    // saved, one launch fewer).  Throughput tiles only: launch_gemm_nt returns 0 partials for small problems, which keep the
    // stand-alone lg_ln_gelu pass.
    int P = 0;
    { ProfScope p(c, "lg_ffn1");   // A = [x | second]: second is the message, or the attention context when Wo is folded into W1
      GemmArgs a = gemm_lgw(c, x, 256, w1, 512, b1, b.h, 512, rows, 512, 512);
      a.A2 = second; a.lda2 = 256; a.K1 = 256;
      if (!gemm_latency_regime(a)) a.stats_out = b.lnstat;   // latency regime: the stand-alone pass below (see lg_kernels.hip)
      P = launch_gemm_nt(s, a); }
    if (P == 0 && !c->opt_lg_fp16x2) {
        // one / few pairs per call: LayerNorm + GELU inside ffn.3 (ffn2_lat.hip: the 16 x 512 panel normalised once per workgroup) -- no stand-alone
        // pass, no second round trip of h.  (The fp16x2 option keeps the split form of gemm_lat behind the stand-alone pass.)
        ProfScope p(c, "lg_ffn2");
        if (launch_ffn2_ln_lat(s, b.h, w2, b2, g, be, x, 256, x, 256, rows)) return;
    }
    if (P == 0) { ProfScope p(c, "lg_ln_gelu"); launch_lg_ln_gelu(s, b.h, g, be, rows); }   // small problems: stand-alone pass
    { ProfScope p(c, "lg_ffn2");
      GemmArgs a = gemm_lgw(c, b.h, 512, w2, 512, b2, x, 256, rows, 256, 512);
      a.R = x; a.ldr = 256;
      if (P > 0) { a.stats_in = b.lnstat; a.stats_p = P; a.ln_g = g; a.ln_b = be; }
      launch_gemm_nt(s, a); }
}

// projection + attention of a self block: b.qkv <- [q | k | v] (q | k rotated, unless the fallback named below ran), b.ctx <- softmax(q k^T / 8) v per head.
// Returns whether b.qkv holds ROTATED q | k (false: the plain-epilogue fallback, rotary applied by the attention kernel on load).
bool lg_self_qkv_attention(rfe_ctx* c, LgBuffers& b, const LgLayerDev& Lw, const float* x, const float* csn, const int32_t* lens, int nseq, int L) {
    hipStream_t s = c->stream;
    const int rows = nseq * L;
    // q,k,v = Wqkv x + b, q and k rotated by the projection's epilogue -- gemm_lat.hip at one / few pairs, gemm.hip's ROPE tile at throughput shapes (table
    // rows staged into LDS by DMA under the K loop) -- so that every attention kernel runs without a table and takes its K tiles straight into LDS
    // (self blocks: lg_attention_dma_kernel 523 us against 565 us for the form that rotates every staged K tile; +9 us on the projection).
    // Rotating only K there and q as the attention loads it measured worse on both sides (profiles/r05_ab_notes.md).
    // RFE_OPT_LG_FP16X2: gemm_h2.hip has no rotary epilogue, lg_attention_h2_kernel rotates both on load.
    bool roped = false;
    { ProfScope p(c, "lg_qkv");
      GemmArgs a = gemm_lgw(c, x, 256, Lw.wqkv, 256, Lw.bqkv, b.qkv, 768, rows, 768, 256);
      if (gemm_latency_regime(a) && launch_gemm_lat(s, a, csn, 512)) roped = true;
      else {
          if (csn) {
              a.rope_c0 = 0; a.rope_c1 = 512;
              if (gemm_nt_rope_ok(a)) { a.rope_csn = csn; roped = true; }
          }
          launch_gemm_nt(s, a);
      } }
    { ProfScope p(c, "lg_attention");
      launch_lg_attention(s, b.qkv, b.qkv + 256, b.qkv + 512, 768, b.ctx, nseq, L, L, lens, lens, nullptr, lg_part(b, nseq, L), roped ? nullptr : csn, c->opt_lg_fp16x2); }
    return roped;
}

// self block on `nseq` sequences of L tokens held in x (in place); scratch: b.qkv, b.ctx, b.msg, b.h
void lg_self_block(rfe_ctx* c, LgBuffers& b, const LgLayerDev& Lw, float* x, const float* csn, const int32_t* lens, int nseq, int L) {
    hipStream_t s = c->stream;
    const int rows = nseq * L;
    lg_self_qkv_attention(c, b, Lw, x, csn, lens, nseq, L);
    if (c->opt_lg_fold) {
        lg_ffn(c, b, x, b.ctx, rows, Lw.w1f, Lw.b1f, Lw.lng, Lw.lnb, Lw.w2, Lw.b2);
    } else {
        { ProfScope p(c, "lg_proj"); launch_gemm_nt(s, gemm_lgw(c, b.ctx, 256, Lw.wo, 256, Lw.bo, b.msg, 256, rows, 256, 256)); }
        lg_ffn(c, b, x, b.msg, rows, Lw.w1, Lw.b1, Lw.lng, Lw.lnb, Lw.w2, Lw.b2);
    }
}

// the assignment stage on b.sim / b.x / b.lens: matchability head (z = log sigmoid), row and column log-sum-exp, both argmaxes, mutual check + filter +
// ordered compaction.  Leaves b.z, b.rowlse, b.collse, b.a0, b.mx0, b.a1 behind; (P, L) selects the form (launch_lg_assign).  rfe_k_lightglue_assign runs it alone.
void lg_assign_stage(hipStream_t s, LgBuffers& b, int P, int L, float thr, int cap, int32_t* S, int32_t* pairs, float* ms,
                     float* scores_opt, int scores_pair, const float* wm, const float* bm) {
    if (!lg_assign_few_pairs(P, L)) launch_lg_matchability(s, b.x, wm, bm, (int64_t)2 * P * L, b.z);   // few pairs: inside the row log-sum-exp launch
    launch_lg_assign(s, b.sim, b.z, b.z + (size_t)P * L, P, L, cap, b.lens, b.lens + P, thr, scores_opt, b.rowlse,
                     b.collse, b.a0, b.mx0, b.a1, S, pairs, ms, scores_pair, b.x, wm, bm, b.z);
}

// runs the 9 layers + assignment on already staged b.x / b.kn / b.lens / b.kvmap.
// first_self_done: b.x already holds the output of layer 0's self block and b.csn the rotary table
// (stream mode computes them once per FRAME instead of once per pair side).
int lg_forward(rfe_ctx* c, LgBuffers& b, int P, int L, float thr, int cap, int32_t* S, int32_t* pairs, float* ms,
               float* scores_opt, bool first_self_done, bool posenc_done) {
    hipStream_t s = c->stream;
    const LgWeightsDev& W = c->lg;
    const int rows = 2 * P * L, nseq = 2 * P;
    if (!first_self_done && !posenc_done) { ProfScope p(c, "lg_misc"); launch_lg_posenc(s, b.kn, W.wr, rows, b.csn); }
    for (int l = 0; l < LG_LAYERS; ++l) {
        const LgLayerDev& Lw = W.L[l];
        if (l > 0 || !first_self_done) lg_self_block(c, b, Lw, b.x, b.csn, b.lens, nseq, L);
        // ---- cross block
        { ProfScope p(c, "lg_cross_qkv"); launch_gemm_nt(s, gemm_lgw(c, b.x, 256, Lw.cwqkv, 256, Lw.cbqkv, b.qkv, 512, rows, 512, 256)); }
        { ProfScope p(c, "lg_attention"); lg_cross_attention(c, b, b.qkv, 512, b.ctx, P, L); }
        if (c->opt_lg_fold) {
            lg_ffn(c, b, b.x, b.ctx, rows, Lw.cw1f, Lw.cb1f, Lw.clng, Lw.clnb, Lw.cw2, Lw.cb2);
        } else {
            { ProfScope p(c, "lg_proj"); launch_gemm_nt(s, gemm_lgw(c, b.ctx, 256, Lw.cwo, 256, Lw.cbo, b.msg, 256, rows, 256, 256)); }
            lg_ffn(c, b, b.x, b.msg, rows, Lw.cw1, Lw.cb1, Lw.clng, Lw.clnb, Lw.cw2, Lw.cb2);
        }
    }
    // ---- assignment
    { ProfScope p(c, "lg_proj");
      GemmArgs a = gemm_lgw(c, b.x, 256, W.wp, 256, W.bp, b.md, 256, rows, 256, 256);
      a.alpha = 0.25f;  // / 256^(1/4)
      launch_gemm_nt(s, a); }
    { ProfScope p(c, "lg_sim");
      GemmArgs g = gemm_lg(b.md, 256, b.md + (size_t)P * L * 256, 256, nullptr, b.sim, L, L, L, 256);
      g.batch = P; g.sA = (long long)L * 256; g.sB = (long long)L * 256; g.sC = (long long)L * L;
      g.m_valid = b.lens;
      launch_gemm_nt(s, g); }
    // one-shot test tap (rfe_k_set_lightglue_tap): final token states [L,256] per side and the log-assignment matrix [L,L]
    // of ONE pair of this forward, whatever the entry point and tiling (batched, stream, stereo frame)
    const bool tap = c->tap.armed && c->tap.pair < P;
    c->tap.armed = false;
    int scores_pair = -1;
    if (tap && c->tap.scores && !scores_opt) { scores_opt = c->tap.scores; scores_pair = c->tap.pair; }
    { ProfScope p(c, "lg_assign");
      lg_assign_stage(s, b, P, L, thr, cap, S, pairs, ms, scores_opt, scores_pair, W.wm, W.bm); }
    if (tap) {
        if (c->tap.x0) RFE_HIP(c, hipMemcpyAsync(c->tap.x0, b.x + (size_t)c->tap.pair * L * 256, (size_t)L * 1024, hipMemcpyDeviceToDevice, s));
        if (c->tap.x1) RFE_HIP(c, hipMemcpyAsync(c->tap.x1, b.x + (size_t)(P + c->tap.pair) * L * 256, (size_t)L * 1024, hipMemcpyDeviceToDevice, s));
    }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

// stage device inputs [P,Mmax,*]/[P,Nmax,*] into the padded side-major token layout: descriptors -> x, normalised keypoints -> kn,
// rows past the input capacity zeroed, clamped lengths + cross-attention map -- one launch (it replaced two memsets, four strided
// device-to-device copies and the set-up kernel: eight enqueues per call on the single-pair latency path)
__global__ __launch_bounds__(256) void lg_stage_kernel(const float* __restrict__ k0n, const float* __restrict__ k1n,
                                                       const float* __restrict__ d0, const float* __restrict__ d1,
                                                       const int32_t* __restrict__ m, const int32_t* __restrict__ n, int P, int Mmax,
                                                       int Nmax, int L, float* __restrict__ x, float* __restrict__ kn,
                                                       int32_t* __restrict__ lens, int32_t* __restrict__ kvmap,
                                                       const float* __restrict__ wr, float2* __restrict__ csn) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 2 * P; i += 256) {
            int v = i < P ? m[i] : n[i - P];
            const int cap = i < P ? Mmax : Nmax;
            v = v < 0 ? 0 : (v > cap ? cap : v);
            lens[i] = v;
            kvmap[i] = i < P ? i + P : i - P;
        }
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);     // side-major: row = (side * P + pair) * L + i
    if (row >= (int64_t)2 * P * L) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)(row % L), sp = (int)(row / L), side = sp >= P, pair = side ? sp - P : sp;
    const int cap = side ? Nmax : Mmax;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 kv = make_float2(0.f, 0.f);
    if (i < cap) {
        const size_t src = (size_t)pair * cap + i;
        v = reinterpret_cast<const float4*>((side ? d1 : d0) + src * 256)[lane];
        if (lane == 0) kv = reinterpret_cast<const float2*>(side ? k1n : k0n)[src];
    }
    reinterpret_cast<float4*>(x + row * 256)[lane] = v;
    if (lane == 0) reinterpret_cast<float2*>(kn)[row] = kv;
    if (csn) {   // the rotary table row of this token (lg_posenc_kernel's arithmetic): saves the stand-alone launch in front of every forward
        const float kx = __shfl(kv.x, 0), ky = __shfl(kv.y, 0);
        if (lane < 32) {
            const float th = fmaf(wr[2 * lane + 1], ky, wr[2 * lane] * kx);
            csn[row * 32 + lane] = make_float2(cosf(th), sinf(th));
        }
    }
}

int lg_stage(rfe_ctx* c, LgBuffers& b, const float* k0n, const float* k1n, const float* d0, const float* d1,
             const int32_t* m, const int32_t* n, int P, int Mmax, int Nmax, int L) {
    const int64_t rows = (int64_t)2 * P * L;
    hipLaunchKernelGGL(lg_stage_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, c->stream, k0n, k1n, d0, d1, m, n, P, Mmax, Nmax, L,
                       b.x, b.kn, b.lens, b.kvmap, c->lg.wr, reinterpret_cast<float2*>(b.csn));   // the rotary table too: lg_forward(posenc_done = true)
    return RFE_OK;
}

int lg_check(rfe_ctx* c, int P, int Mmax, int Nmax) {
    if (!c) return RFE_ERR_INVALID;
    if (!c->has_lg) return fail(c, RFE_ERR_NO_WEIGHTS, "LightGlue weights not loaded (rfe_load_weights / rfe_set_weights)");
    if (P <= 0 || Mmax <= 0 || Nmax <= 0 || Mmax > 4096 || Nmax > 4096) return fail(c, RFE_ERR_INVALID, "match: P > 0 and 1 <= Mmax,Nmax <= 4096 required");
    return RFE_OK;
}

}  // namespace rfe

// the argument check of both match entries (the pointers are the caller's, whichever side they live on)
static int match_check(rfe_ctx* c, const void* k0n, const void* k1n, const void* d0, const void* d1, const void* m, const void* n, int P, int Mmax, int Nmax,
                       const void* S, const void* pairs, const void* ms) {
    int rc = lg_check(c, P, Mmax, Nmax);
    if (rc) return rc;
    if (!k0n || !k1n || !d0 || !d1 || !m || !n || !S || !pairs || !ms) return fail(c, RFE_ERR_INVALID, "match: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    return RFE_OK;
}
extern "C" int rfe_match_dev(rfe_ctx* c, const float* k0n, const float* k1n, const float* d0, const float* d1,
                             const int32_t* m, const int32_t* n, int P, int Mmax, int Nmax, float thr, int32_t* S,
                             int32_t* pairs, float* ms) {
    int rc = match_check(c, k0n, k1n, d0, d1, m, n, P, Mmax, Nmax, S, pairs, ms);
    if (rc) return rc;
    const int L = ((std::max(Mmax, Nmax) + 3) / 4) * 4;
    LgBuffers b;
    if ((rc = lg_carve(c, P, L, b))) return rc;
    if ((rc = lg_stage(c, b, k0n, k1n, d0, d1, m, n, P, Mmax, Nmax, L))) return rc;
    return lg_forward(c, b, P, L, thr, std::min(Mmax, Nmax), S, pairs, ms, nullptr, false, true);
}

extern "C" int rfe_match(rfe_ctx* c, const float* k0n, const float* k1n, const float* d0, const float* d1,
                         const int32_t* m, const int32_t* n, int P, int Mmax, int Nmax, float thr, int32_t* S,
                         int32_t* pairs, float* ms) {
    int rc = match_check(c, k0n, k1n, d0, d1, m, n, P, Mmax, Nmax, S, pairs, ms);
    if (rc) return rc;
    const size_t cap = (size_t)std::min(Mmax, Nmax);
    float *dk0, *dk1, *dd0, *dd1, *dms; int32_t *dm, *dn, *dS, *dp;
    // inputs packed into the pinned mirror of the device block, results fetched with one DMA out: see ensure_pin
    HostIo io(c, HostIo::PINNED);
    io.in(dk0, k0n, (size_t)P * Mmax * 2); io.in(dk1, k1n, (size_t)P * Nmax * 2); io.in(dd0, d0, (size_t)P * Mmax * 256);
    io.cut();   // two DMAs, so that the host copy of the second descriptor block (1 MB at K = 1024) runs while the first one is on the bus
    io.in(dd1, d1, (size_t)P * Nmax * 256); io.in(dm, m, P); io.in(dn, n, P);
    io.out(dS, S, P); io.out(dp, pairs, P * cap * 2); io.out(dms, ms, P * cap);
    if ((rc = io.upload())) return rc;
    const int L = ((std::max(Mmax, Nmax) + 3) / 4) * 4;
    if ((rc = ensure_ws(c, &c->ws_lg, &c->ws_lg_bytes, lg_ws_bytes(c, P, L)))) return rc;   // before the key is formed: a capture must not allocate
    int thr_bits; memcpy(&thr_bits, &thr, 4);
    if ((rc = run_host_graph(c, c->g_match, host_graph_key(c, "m", {P, Mmax, Nmax, thr_bits}),
                             [&] { return rfe_match_dev(c, dk0, dk1, dd0, dd1, dm, dn, P, Mmax, Nmax, thr, dS, dp, dms); }))) return rc;
    return io.download();
}

extern "C" int rfe_match_fused(rfe_ctx* c, const float* kp0, int M, const float* kp1, int N, const float* desc0,
                               const float* desc1, int rows, int cols, float filter_thr, float match_thresh,
                               int32_t* vnMatches12) {
    if (!c) return RFE_ERR_INVALID;
    if (M < 0 || N < 0 || !vnMatches12) return fail(c, RFE_ERR_INVALID, "match_fused: bad argument");
    for (int i = 0; i < M; ++i) vnMatches12[i] = -1;   // vnMatches12.resize(M, -1): SPmatcher.cc:375,413,460
    if (M == 0 || N == 0) return 0;
    // NormalizeKeypoints, reference src/Matchers/transform.cpp:19-32
    std::vector<float> k0((size_t)M * 2), k1((size_t)N * 2);
    const float sx = (float)cols / 2, sy = (float)rows / 2, scale = (float)std::max(cols, rows) / 2;
    for (int i = 0; i < M; ++i) { k0[2 * i] = (kp0[2 * i] - sx) / scale; k0[2 * i + 1] = (kp0[2 * i + 1] - sy) / scale; }
    for (int i = 0; i < N; ++i) { k1[2 * i] = (kp1[2 * i] - sx) / scale; k1[2 * i + 1] = (kp1[2 * i + 1] - sy) / scale; }
    const int cap = std::min(M, N);
    std::vector<int32_t> pairs((size_t)cap * 2);
    std::vector<float> ms(cap);
    int32_t S = 0, m = M, n = N;
    int rc = rfe_match(c, k0.data(), k1.data(), desc0, desc1, &m, &n, 1, M, N, filter_thr, &S, pairs.data(), ms.data());
    if (rc) return rc;
    // Matcher_PostProcess_fused, reference src/Matchers/lightglue_onnx.cpp:437-453
    int size = 0;
    for (int i = 0; i < S; ++i)
        if (ms[i] > match_thresh) { ++size; vnMatches12[pairs[2 * i]] = pairs[2 * i + 1]; }
    return size;
}

// =====================================================================================
// batched stream: extract B frames, match (i, i+1)
// =====================================================================================
extern "C" int rfe_extract_match_stream_dev(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, int Kmax,
                                            float thr, float filter_thr, int32_t* n, int32_t* kxy, float* score,
                                            float* desc, int32_t* S, int32_t* pairs, float* ms) {
    int rc = rfe_extract_u8_dev(c, img, H, W, stride, B, Kmax, thr, n, kxy, score, desc);
    if (rc || B < 2) return rc;
    if ((rc = lg_check(c, B - 1, Kmax, Kmax))) return rc;
    if (!S || !pairs || !ms) return fail(c, RFE_ERR_INVALID, "stream: null match output");
    const int P = B - 1, L = ((Kmax + 3) / 4) * 4;
    LgBuffers b;
    float *kn_all, *rot;
    if ((rc = lg_carve(c, P, L, b, [&](Bump& a) {
             kn_all = a.take<float>((size_t)B * Kmax * 2);   // normalised keypoints of all B frames
             rot = a.take<float>((size_t)B * L * 64);        // per-FRAME rotary table (cos, sin pairs)
         }))) return rc;
    hipStream_t s = c->stream;
    if (L != Kmax) {   // Kmax not a multiple of 4: every pair runs its own layer-0 self block
        { ProfScope p(c, "lg_misc");
          launch_normalize_kpts(s, kxy, (int64_t)B * Kmax, H, W, kn_all);
          if ((rc = lg_stage(c, b, kn_all, kn_all + (size_t)Kmax * 2, desc, desc + (size_t)Kmax * 256, n, n + 1, P, Kmax, Kmax, L))) return rc; }
        return lg_forward(c, b, P, L, filter_thr, Kmax, S, pairs, ms, nullptr, false, true);
    }
    // Every interior frame is side 1 of pair i-1 and side 0 of pair i, and layer 0's self block depends on
    // the frame alone: run it (and the positional encoding) once per FRAME, then scatter into the pair layout.
    // B = 2 (one pair): the per-frame layout IS the pair layout, the block runs in place and nothing is scattered
    float* xf = P == 1 ? b.x : b.md;         // [B, L, 256]: md ([2P, L, 256], B <= 2P) is only used by the assignment at the end
    float* csnf = P == 1 ? b.csn : rot;      // [B*L, 32, 2], own scratch (the similarity buffer [P, L, L] is too small for it when L < 64 (P+1)/P)
    { ProfScope p(c, "lg_misc");   // one launch: NormalizeKeypoints + rotary table + descriptors -> token rows + lengths / cross map
      launch_lg_frame_prologue(s, kxy, desc, c->lg.wr, n, B, L, H, W, kn_all, csnf, xf, b.lens, b.kvmap); }
    lg_self_block(c, b, c->lg.L[0], xf, csnf, n, B, L);
    if (P > 1) {
      ProfScope p(c, "lg_misc");
      const size_t half = (size_t)P * L;
      launch_copy_f32(s, xf, b.x, (int64_t)half * 256);
      launch_copy_f32(s, xf + (size_t)L * 256, b.x + half * 256, (int64_t)half * 256);
      launch_copy_f32(s, csnf, b.csn, (int64_t)half * 64);
      launch_copy_f32(s, csnf + (size_t)L * 64, b.csn + half * 64, (int64_t)half * 64); }
    RFE_HIP(c, hipGetLastError());
    return lg_forward(c, b, P, L, filter_thr, Kmax, S, pairs, ms, nullptr, true);
}
