// rfe_internal.h -- shared declarations of librover_fe.so (HIP, gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rover_fe.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace rfe {

// The library never consults the environment: its numerics and kernel choices depend on its arguments and on rfe_set_option alone.

// ---------------------------------------------------------------- SuperPoint layer table
// names follow the reference's dead libtorch header include/SuperPoint.h:24-41
struct SpLayer { int cin, cout, k; bool pool; };   // pool: the fused 2x2 max-pool behind the layer (decides its launch AND which weight images are packed)
static const SpLayer kSpLayers[12] = {
    {1, 64, 3, false}, {64, 64, 3, true}, {64, 64, 3, false}, {64, 64, 3, true}, {64, 128, 3, false}, {128, 128, 3, true},
    {128, 128, 3, false}, {128, 128, 3, false}, {128, 256, 3, false}, {256, 65, 1, false}, {128, 256, 3, false}, {256, 256, 1, false}};
enum { L_1A, L_1B, L_2A, L_2B, L_3A, L_3B, L_4A, L_4B, L_PA, L_PB, L_DA, L_DB };

constexpr int LG_LAYERS = 9;
constexpr int64_t SP_COUNT = 1300865;
constexpr int64_t LG_COUNT = 11321153;

// conv3x3 implicit-GEMM tiling (see sp_conv.hip)
constexpr int CONV_CK = 8;    // input channels per LDS chunk
constexpr int CONV_NT = 64;   // output channels per workgroup

// device-side packed SuperPoint weights
struct SpWeightsDev {
    float* conv1a_w = nullptr;           // [9][64]   (kappa-major)
    float* packed[12] = {nullptr};       // 3x3 layers: [Cout/64][Cin/16][144][64]; 1x1: [N][K] as-is
    float* bias[12] = {nullptr};
    float* da_rows = nullptr;            // convDa's weight as it comes, OIHW = [256][1152] with k = ci*9 + ky*3 + kx: the B operand of the sparse descriptor head's GEMM
};

struct LgLayerDev {
    float *wqkv, *bqkv, *wo, *bo, *w1, *b1, *lng, *lnb, *w2, *b2;
    float *cwqk, *cbqk, *cwv, *cbv, *cwo, *cbo, *cw1, *cb1, *clng, *clnb, *cw2, *cb2;
    float *cwqkv, *cbqkv;   // packed [512][256] = [Wqk ; Wv] and [512] bias (device copy made at load time)
    // attention output projection folded into the first FFN Linear (made at load time, see set_lg):
    // ffn1([x | ctx Wo^T + bo]) == [x | ctx] [W1a | W1b Wo]^T + (b1 + W1b bo)
    float *w1f, *b1f, *cw1f, *cb1f;
};
struct LgWeightsDev {
    float* blob = nullptr;  // whole canonical blob on device; pointers below index into it
    float* extra = nullptr; // packed cross-attention projection weights (cwqkv / cbqkv of every layer)
    float* wr;
    LgLayerDev L[LG_LAYERS];
    float *wp, *bp, *wm, *bm;
    // fp16 (hi, lo) planes of every float of `blob` and `extra`, made at load time for RFE_OPT_LG_FP16X2 (gemm_h2.hip):
    // h2 = [hi blob | lo blob | hi extra | lo extra]; the planes of a weight matrix sit at the matrix' own offset inside its buffer
    uint16_t* h2 = nullptr;
    size_t n_blob = 0, n_extra = 0;
};

// ---------------------------------------------------------------- profiling
struct Stage { std::string name; double ms = 0; int64_t calls = 0; };

struct GemmArgs {
    const float* A; int lda;          // rows of A, K-contiguous
    const float* A2; int lda2; int K1; // optional second A source for k >= K1 (concat [x | msg])
    const float* B; int ldb;          // B[n][k], K-contiguous (PyTorch Linear weight layout)
    const float* bias;                // [N] or null
    const float* R; int ldr;          // optional residual added after alpha/relu
    float* C; int ldc;
    int M, N, K;
    float alpha; int relu;
    long long sA, sA2, sB, sC, sR;    // batch strides (grid.z)
    const int* m_valid;               // optional per-batch valid row count (rows >= m_valid skipped)
    int batch;
    // LayerNorm(N) + GELU fused across two GEMMs (LightGlue ffn.0 -> LN -> GELU -> ffn.3): the producer's epilogue writes per-row
    // partial (mean, sum of squared deviations from it) of what it stores -- one pair per (column tile, wave column) = per 128
    // columns: stats_out [M][P][2], P returned by
    // launch_gemm_nt --, the consumer normalises its A operand while staging it: gelu(((a - mean) * rstd) * ln_g[k] + ln_b[k])
    float* stats_out;
    const float* stats_in; int stats_p; const float* ln_g; const float* ln_b;
    // optional fp16 (hi, lo) planes of B, same [N][K] layout and ldb (RFE_OPT_LG_FP16X2): the shapes that would take the 128 x 256
    // throughput tile run gemm_h2.hip's split GEMM on the f16 matrix pipe instead; everything else ignores them
    const uint16_t* Bh; const uint16_t* Bl;
    // kperm != 0: the caller does not need the k-ascending reduction order (LightGlue: tolerance-checked, not bit-exact).  The 128-row
    // tiles then use the 16-byte-swizzled LDS layout with 128-bit fragment reads, which consume k in the order (s, 16 + s) per K tile.
    int kperm;
    // rope_csn != null: LightGlue's rotary encoding applied by the epilogue to output columns rope_c0 <= n < rope_c1 (the k columns of the qkv projection;
    // multiples of 256): (t0, t1) -> (t0 c - t1 s, t1 c + t0 s) on adjacent column pairs, (c, s) = rope_csn[row][(column & 63) / 2].  Plain projections only.
    const float* rope_csn; int rope_c0, rope_c1;
};

}  // namespace rfe

// the published LightGlue-style export settings (include/rover_fe.h: rfe_hparams defaults)
inline rfe_hparams rfe_default_hparams() { return rfe_hparams{1024, 0.0005f, 4, 4, 0, rfe::LG_LAYERS, 4, 0.1f}; }

struct rfe_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;   // descriptor head of SuperPoint runs here, concurrently with the detector head
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_pyr = nullptr;         // rfe_extract_pyramid_u8*: the level chain (side stream) is done
    std::string err;
    bool has_sp = false, has_lg = false;
    bool opt_lg_fold = true;             // RFE_OPT_LG_FOLD_WO
    bool opt_lg_fp16x2 = false;          // RFE_OPT_LG_FP16X2
    bool opt_host_graph = false;         // RFE_OPT_HOST_GRAPH: the synchronous host entries replay a captured hipGraph of their kernel sequence
    // one instantiated graph per host entry kind (extract / match): `key` names the call shape + every pointer and setting baked into the kernel arguments,
    // `seen` the shape of the last ordinary call (a shape is captured on its SECOND call: the first one allocates workspaces and sets function attributes)
    // RFE_OPT_HOST_GRAPH: a few instantiated graphs per entry (LRU), and a short history of the keys seen lately with their counts -- a shape is captured
    // only once it has come back HOST_GRAPH_REPEATS times, so a caller whose shapes never repeat (per-frame keypoint counts) pays no capture at all
    struct HostGraph {
        struct Slot { std::string key; hipGraphExec_t exec = nullptr; unsigned long long used = 0; };
        struct Seen { std::string key; int count = 0; unsigned long long used = 0; };
        Slot slot[4]; Seen seen[8]; unsigned long long tick = 0;
    };
    HostGraph g_extract, g_match;
    unsigned long long settings_gen = 0; // bumped by everything a captured graph bakes in: weights, hyper-parameters, options
    rfe_hparams hp = rfe_default_hparams();   // graph hyper-parameters (RFEW v2 header / rfe_set_hparams)
    rfe::SpWeightsDev sp;                // views into *sp_hold / *lg_hold
    rfe::LgWeightsDev lg;
    std::shared_ptr<void> sp_hold, lg_hold;   // device copies, shared by every ctx of the process that loaded the same blob on the same device
    // grow-only workspaces
    void* ws_sp = nullptr; size_t ws_sp_bytes = 0;
    void* ws_lg = nullptr; size_t ws_lg_bytes = 0;
    void* ws_io = nullptr; size_t ws_io_bytes = 0;   // staging for host-pointer entry points
    void* h_pin = nullptr; size_t h_pin_bytes = 0;   // pinned host mirror of ws_io for the per-frame host entries (extract / match): one DMA each way
    void* ws_tmp = nullptr; size_t ws_tmp_bytes = 0; // test hooks
    // rfe_extract_pyramid_u8*: level images (when the caller passes none) + per-level SuperPoint staging -- apart from ws_sp, which every
    // SuperPoint pass carves from offset 0 -- and the resampling tables of the last (H, W, nlevels, scale_factor) in ws_ptab
    void* ws_pyr = nullptr; size_t ws_pyr_bytes = 0;
    void* ws_ptab = nullptr; size_t ws_ptab_bytes = 0; std::string ptab_key; std::vector<size_t> ptab_off;
    int32_t* sp_cnt = nullptr;           // [4][2] (count, tickets) of the fused detector tail (sp_post.hip: sp_tail_lat_kernel); zero between calls
    bool sp_cnt_dirty = false;           // the tail ran and its ranking kernel was not enqueued behind it (an error in between): zeroed before the next use
    void* ws_ps = nullptr; size_t ws_ps_bytes = 0;   // rfe_search_by_projection*: grid, segment offsets, (index, distance) slots
    int ps_cap = 0;                                  // rfe_search_by_projection (host form): most slots any call has needed
    void* ws_tri = nullptr; size_t ws_tri_bytes = 0; // rfe_triangulate_neighbours*: per-slot results, claims, per-neighbour counts
    void* ws_bow = nullptr; size_t ws_bow_bytes = 0; // rfe_bow_transform*: per-feature word / node / weight the caller did not ask for
    void* ws_s3 = nullptr; size_t ws_s3_bytes = 0;   // rfe_sim3_ransac*: per-problem records, the front's rows, counts and hypotheses the caller did not ask for
    void* ws_tv = nullptr; size_t ws_tv_bytes = 0;   // rfe_two_view*: per-problem records, match rows, 8-sets, per-iteration models, CheckRT's per-match results
    // rfe_local_ba*: estimates, structure, per-edge terms, the dense reduced system (ws_lba); the Schur blocks' pair lists, sized from a
    // count the first kernels leave, apart (ws_lba_pairs); a pinned block for the one small read per LM trial (h_lba)
    void* ws_lba = nullptr; size_t ws_lba_bytes = 0;
    void* ws_lba_pairs = nullptr; size_t ws_lba_pairs_bytes = 0;
    void* h_lba = nullptr;
    // rfe_essential_graph*: estimates, structure, per-edge terms and the solve's vectors (ws_eg); the dense 7 Nf x 7 Nf matrix, sized from
    // the number of free vertices the front leaves, apart (ws_eg_mat); the pinned block of the small reads (h_eg)
    void* ws_eg = nullptr; size_t ws_eg_bytes = 0;
    void* ws_eg_mat = nullptr; size_t ws_eg_mat_bytes = 0;
    void* h_eg = nullptr;
    // rfe_global_ba*: estimates, structure, per-edge terms and the solve's vectors (ws_gba); the Schur blocks' pair lists with their
    // sorting copy, sized from a count the front leaves (ws_gba_pairs); the dense 6 P x 6 P matrix in tiles, of which only the tiles of
    // the pattern's fill are touched (ws_gba_mat); the pinned block of the small reads (h_gba)
    void* ws_gba = nullptr; size_t ws_gba_bytes = 0;
    void* ws_gba_pairs = nullptr; size_t ws_gba_pairs_bytes = 0;
    void* ws_gba_mat = nullptr; size_t ws_gba_mat_bytes = 0;
    void* h_gba = nullptr;
    int gba_stop_after = 0;              // one-shot test hook (rfe_k_global_ba_stop_after): the next call sets *stop behind this many trials
    void* ws_st = nullptr; size_t ws_st_bytes = 0;   // stereo stream state: staged views, previous left view's features
    int st_H = 0, st_W = 0, st_K = 0; bool st_have_prev = false; int st_flip = 0; std::string st_pyr_key;   // st_flip: which of the two state slots holds the previous left view
    // one-shot test tap (rfe_k_set_lightglue_tap): the next LightGlue forward of this ctx, whatever entry point runs it,
    // copies the final token states / log-assignment matrix of one pair to these device buffers
    struct { bool armed = false; int pair = 0; float *x0 = nullptr, *x1 = nullptr, *scores = nullptr; } tap;
    // profiling
    bool prof = false;
    std::string prof_filter;          // non-empty: only this stage records events
    std::vector<rfe::Stage> stages;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
    std::vector<hipEvent_t> ev_pool;
};

namespace rfe {

int fail(rfe_ctx* c, int code, const std::string& msg);
#define RFE_HIP(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return rfe::fail((ctx), RFE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// profiling scope: records two events around a stage when ctx->prof is on
struct ProfScope {
    rfe_ctx* c; int idx; hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    ProfScope(rfe_ctx* ctx, const char* name, hipStream_t on = nullptr);
    ~ProfScope();
};
void prof_collect(rfe_ctx* c);

int ensure_ws(rfe_ctx* c, void** p, size_t* cur, size_t need);

// ---------------------------------------------------------------- kernel launchers
// sp_conv.hip
// pool: the layer is launched with the fused 2x2 max-pool (decides whether the 16 x 16 x 4 tiles' weight image is emitted: conv3x3_reads_t16)
bool conv3x3_reads_t16(int cin, int cout, bool pool);
void pack_conv3x3_weights(const float* w_oihw, int cin, int cout, bool pool, std::vector<float>& out);
size_t packed_conv3x3_count(int cin, int cout, bool pool);
void launch_conv3x3(hipStream_t s, const float* in, int B, int H, int W, int cin,
                    const float* wpacked, const float* bias, int cout, bool relu, bool pool, float* out,
                    int tag = 0);
// img: u8 pixels (NormalizeImage fused) or, img_f32, already normalised float pixels; stride in pixels
void launch_conv1ab_fused(hipStream_t s, const void* img, bool img_f32, int stride, int B, int H, int W, const float* w1a,
                          const float* b1a, const float* wp, const float* bias, float* out, long long frame_step = 0 /*pixels between frames; 0 = stride * H*/);
// gemm.hip
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the CURRENT device's copy of a kernel: set it once per (kernel, device) -- pools run
// one ctx per device.  `done` is the caller's per-kernel flag array (static bool [64]); races only repeat the idempotent call.
inline void ensure_dynamic_lds(const void* kernel, int bytes, bool* done) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !done[dev]) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
}
int launch_gemm_h2(hipStream_t s, const GemmArgs& g);   // gemm_h2.hip: split GEMM on the f16 matrix pipe (GemmArgs::Bh / Bl), called by launch_gemm_nt
void launch_split_f16(hipStream_t s, const float* x, uint16_t* hi, uint16_t* lo, size_t n);
bool gemm_nt_rope_ok(const GemmArgs& g);                  // may launch_gemm_nt carry GemmArgs::rope_csn for this shape? (set rope_c0 / rope_c1 first)
int launch_gemm_nt(hipStream_t s, const GemmArgs& g);   // returns the number of partial-statistics pairs per row it wrote (0 without stats_out)
// The throughput tiles (128-row) take a problem when they give every CU a workgroup; everything smaller is the LATENCY regime (one or a
// few pairs per call -- what the reference itself runs): gemm_lat.hip / lg_attention_lat.hip serve it, gemm.hip's 64-row tiles what they refuse.
inline bool gemm_latency_regime(const GemmArgs& g) {
    const long long b = g.batch > 0 ? g.batch : 1;
    auto tiles = [&](int bm, int bn) { return (long long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn) * b; };
    const bool big = (g.N % 256 == 0 && tiles(128, 256) >= 256) || tiles(128, 128) >= 256 || g.M > 8192;
    return !big;
}
// gemm_lat.hip: false = shape not served (nothing launched).  rope_csn != null: rotary epilogue on output columns < rope_cols (qkv).
bool launch_gemm_lat(hipStream_t s, const GemmArgs& g, const float* rope_csn, int rope_cols);
// onnx_load.hip (host only): an ONNX graph file -> canonical weight blob of `kind` + that kind's fields of *hp; false + reason when the file cannot be
// read, a tensor cannot be placed, or a hyper-parameter cannot be read from the graph (nothing is guessed)
bool onnx_convert(const std::string& path, int kind, std::vector<float>& blob, rfe_hparams* hp, std::string& err);
// ffn2_lat.hip: ffn.3 of a one- / few-pair forward with LayerNorm(512) + GELU of its activation fused in (h = ffn.0's raw output); false = not served
bool launch_ffn2_ln_lat(hipStream_t s, const float* h, const float* w2, const float* b2, const float* ln_g, const float* ln_b, const float* R, int ldr,
                        float* C, int ldc, int M);
// lg_attention_lat.hip: one-/few-pair attention without rotary (q, k rotated by the projection); false = shape not served.
bool launch_lg_attention_lat(hipStream_t s, const float* q, const float* k, const float* v, int ld, float* out, int nseq, int Lq, int Lk,
                             const int* qlen, const int* klen, const int* kv_map, bool h2 = false /*RFE_OPT_LG_FP16X2: split products*/);
// sp_post.hip
void launch_softmax65_d2s(hipStream_t s, const float* logits, int ld, int B, int Hc, int Wc, float* score);
constexpr int NMS_MAX_RADIUS = 8;
void launch_nms(hipStream_t s, const float* score, int B, int H, int W, int radius /*1..NMS_MAX_RADIUS*/, int border, float* tmp_ss,
                uint8_t* tmp_mask, uint8_t* tmp_supp, float* out);
void launch_select(hipStream_t s, const float* nms, int B, int H, int W, int Kmax, float thr,
                   float* cand_score, int32_t* cand_idx, int32_t* n_out, int32_t* kxy, float* score,
                   int32_t* chunk_cnt /*B * ceil(H*W/4096) ints of scratch*/, bool topk_always /*rfe_hparams::sp_topk_always*/,
                   unsigned long long* sel_keys /*[B,Kmax] scratch*/, int32_t* sel_n /*[B] scratch*/);
// the detector tail of one to four frames in one launch (softmax65 + depth-to-space + simple_nms(4) + border + threshold -> unordered 64-bit candidate keys)
// and the ranking that consumes it; cand_cnt = two ints per frame, zero between calls (the ranking kernel resets them).  false = not served.
bool launch_sp_tail_lat(hipStream_t s, const float* logits, int B, int Hc, int Wc, int radius, int border, float thr, unsigned long long* cand_keys /*[B, 64 Hc Wc]*/,
                        int32_t* cand_cnt /*[B, 2]*/, float* smap_out /*optional [B, 8 Hc, 8 Wc]*/, float* nmap_out /*optional*/);
void launch_select_keys(hipStream_t s, const unsigned long long* cand_keys, int32_t* cand_cnt, int B, int H, int W, int Kmax, bool topk_always,
                        int32_t* n_out, int32_t* kxy, float* score);
void launch_keys_from_map(hipStream_t s, const float* nms, int B, int HW, float thr, unsigned long long* cand_keys, int32_t* cand_cnt);   // test hook
void launch_descmap_norm(hipStream_t s, float* dmap, int64_t cells);
void launch_desc_sample(hipStream_t s, const float* dmap, int B, int Hc, int Wc, int H, int W,
                        const int32_t* n, const int32_t* kxy, int Kmax, float* desc, uint8_t* desc_bin /*optional u8 [B,Kmax,256] = desc > 0*/,
                        const int32_t* cell_row = nullptr /*sparse head: dmap is packed rows, cell_row [B,Hc*Wc] the row of a cell within its frame*/,
                        const int32_t* row_base = nullptr /*sparse head: [B] first row of every frame*/);
// sparse descriptor head: the cells the keypoints' bilinear footprints touch, in ascending cell order per frame (cell_row [B,Hc*Wc] = row within the frame
// or -1, row_cell [B,cap], count [B]) and the frames' rows packed back to back (row_base [B+1], exclusive prefix of count; [B] = rows of the call); their
// 3x3x128 patches of f4 in the conv's reduction order (patch [rows,1152]); the L2 norm of the live rows
void launch_desc_cells(hipStream_t s, int B, int Hc, int Wc, int H, int W, const int32_t* n, const int32_t* kxy, int Kmax, int cap, int32_t* cell_row,
                       int32_t* row_cell, int32_t* count, int32_t* row_base);
void launch_desc_gather(hipStream_t s, const float* f4, int B, int Hc, int Wc, int cap, const int32_t* row_cell, const int32_t* count, const int32_t* row_base,
                        float* patch);
void launch_descrows_norm(hipStream_t s, float* rows, int B, int cap, const int32_t* count, const int32_t* row_base);
// lg_kernels.hip
void launch_lg_posenc(hipStream_t s, const float* kn, const float* wr, int rows, float* csn /*[rows,32] (cos, sin) pairs*/);
void launch_lg_attention(hipStream_t s, const float* q, const float* k, const float* v, int ld /*row stride of q,k,v*/,
                         float* out, int nseq, int Lq, int Lk, const int* qlen, const int* klen,
                         const int* kv_map /*seq -> kv seq index, or null = identity*/,
                         float* part /*lg_attention_part_bytes(nseq, Lq) of scratch for the split-key variant, or null*/,
                         const float* rope_csn = nullptr /*self blocks: rotary table [nseq*Lq, 32] of (cos, sin) pairs, applied to q and k on load*/,
                         bool fp16x2 = false /*RFE_OPT_LG_FP16X2: problems of >= 32 768 query rows take lg_attention_h2.hip's split products on the f16 matrix pipe*/);
void launch_lg_attention_h2(hipStream_t s, const float* q, const float* k, const float* v, int ld, float* out, int nseq, int Lq, int Lk,
                            const int* qlen, const int* klen, const int* kv_map, const float* rope_csn);   // lg_attention_h2.hip
size_t lg_attention_part_bytes(int nseq, int Lq);
// cross blocks, shared-logit form (lg_kernels.hip): side 0 writes each pair's logits to slog while it runs, side 1 reads them back instead of forming them again
bool lg_cross_shared_ok(int P, int L);        // the default fp32 path takes the form at this shape (throughput shapes from the measured crossover up, slog under its cap)
size_t lg_cross_slog_floats(int P, int L);    // 4 P L^2 logits + the padding a tile's loads may run into
void launch_lg_cross_shared(hipStream_t s, const float* qk_v, int ld /*row stride of the [qk | v] rows, % 4 == 0*/, float* out /*[2 P L, 256]*/, int P, int L,
                            const int* lens /*[2 P], side-major*/, float* slog);
void launch_lg_ln_gelu(hipStream_t s, float* h, const float* g, const float* b, int64_t rows);
void launch_lg_assign(hipStream_t s, const float* sim, const float* z0, const float* z1, int P, int L,
                      int cap, const int* m, const int* n, float thr, float* scores_opt, float* rowlse,
                      float* collse, int32_t* a0, float* mx0, int32_t* a1, int32_t* S, int32_t* pairs,
                      float* ms, int scores_pair /*>= 0: scores_opt is [L,L] and receives that pair only; < 0: every pair into [P,L,L]*/,
                      const float* x, const float* wm, const float* bm, float* z /*few-pair shapes: the matchability head rides in the row log-sum-exp launch*/);
bool lg_assign_few_pairs(int P, int L);   // true: launch_lg_assign computes the matchability itself (launch_lg_matchability must not be called)
void launch_lg_frame_prologue(hipStream_t s, const int32_t* kxy, const float* desc, const float* wr, const int32_t* nkp, int B, int L, int rows, int cols,
                              float* kn, float* csn, float* x, int32_t* lens, int32_t* kvmap);
void launch_lg_matchability(hipStream_t s, const float* x, const float* w, const float* b, int64_t rows, float* z);
void launch_copy_f32(hipStream_t s, const float* src, float* dst, int64_t n);
void launch_normalize_kpts(hipStream_t s, const int32_t* kxy, int64_t n, int rows, int cols, float* out);

// stereo.hip
void launch_stereo_match(hipStream_t s, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride,
                         const float* kL, int N, const float* kR, int Nr, const float* dL, const float* dR, float mb,
                         float mbf, float* uRight, float* depth, int32_t* sadv);

void launch_stereo_match_counts(hipStream_t s, const uint8_t* imgL, const uint8_t* imgR, int H, int W, int stride,
                                const int32_t* kL, const int32_t* kR, int Kmax, const int32_t* counts, const float* dL,
                                const float* dR, float mb, float mbf, float* uRight, float* depth, int32_t* sadv);

// pyramid.hip: the scale pyramid of rfe_extract_pyramid_u8
int pyramid_geometry(int H, int W, int nlevels, float scale_factor, int32_t* level_h, int32_t* level_w, float* level_scale);
// coefficient tables of levels 1..nlevels-1, each level's [W_l] column entries then [H_l] row entries (source index, 11-bit weight of index + 1),
// starting at off[l]
void pyramid_tables(int nlevels, const int32_t* level_h, const int32_t* level_w, std::vector<int2>& tab, std::vector<size_t>& off);
// one level of B frames from the level above (cx / cy: that level's table entries); cx == null: copy the Hd x Wd source as it is
void launch_pyr_resample(hipStream_t s, const uint8_t* src, long long src_frame, int src_stride, int Hs, int Ws, uint8_t* dst, long long dst_frame,
                         int Hd, int Wd, int B, const int2* cx, const int2* cy);
struct PyrMergeArgs {
    int L, Ktot;
    const int32_t* n[RFE_MAX_LEVELS];        // per-level staging of the SuperPoint passes ([B] counts, null = level not run: n_l = 0)
    const int32_t* kxy[RFE_MAX_LEVELS];      // [B, kmax_l, 2]
    const float* sc[RFE_MAX_LEVELS];         // [B, kmax_l]
    const float* desc_l[RFE_MAX_LEVELS];     // [B, kmax_l, 256]
    int kmax[RFE_MAX_LEVELS];
    float scale[RFE_MAX_LEVELS];
    int32_t* n_out; int32_t* level_n /*optional [B, L]*/; float* kpts; int32_t* octave; float* score; float* desc;
};
void launch_pyr_merge(hipStream_t s, const PyrMergeArgs& a, int B);

// level table of the octave-aware stereo match (by-value kernel argument): level l is h[l] x w[l] at byte off[l] of one view's level
// buffer, s[l] = mvScaleFactors[l], inv[l] = 1.0f / s[l]
struct StereoPyrTable {
    int L;
    int32_t h[RFE_MAX_LEVELS], w[RFE_MAX_LEVELS];
    uint32_t off[RFE_MAX_LEVELS];
    float s[RFE_MAX_LEVELS], inv[RFE_MAX_LEVELS];
};
void launch_stereo_match_pyr(hipStream_t s, const uint8_t* levL, const uint8_t* levR, const StereoPyrTable& T, const float* kL,
                             const int32_t* octL, int N, const float* kR, const int32_t* octR, int Nr, const int32_t* counts,
                             const float* dL, const float* dR, float mb, float mbf, int sad_level0, float* uRight, float* depth,
                             int32_t* sadv);

void launch_l2_matrix(hipStream_t s, const float* a, int M, const float* b, int N, float* out);
void launch_binarize(hipStream_t s, const float* d, int64_t rows, uint8_t* out);
void launch_search_candidates(hipStream_t s, const float* q, int Nq, const float* f, int Nf, const int32_t* offsets, const int32_t* cand,
                              const uint8_t* skip, int32_t* best_idx, float* best_dist, float* second_dist);
void launch_distinctive(hipStream_t s, const float* desc, const int32_t* offsets, int total /*>= offsets[Np]*/, int Np, int maxn,
                        float* med /*[total] scratch*/, int32_t* best, float* median);

// DescriptorDistance_sp (SPmatcher.cc:2184-2189) of one descriptor pair held as a float4 per lane, in the canonical order of search.hip,
// proj_search.hip and the oracle: float differences, double accumulation, a lane's four elements then an xor butterfly over the wave
__device__ __forceinline__ float desc_dist_wave(const float4 a, const float4 b) {
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    double p = 0.0;
    p += (double)d0 * (double)d0; p += (double)d1 * (double)d1; p += (double)d2 * (double)d2; p += (double)d3 * (double)d3;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
    return (float)sqrt(p);
}

// t[level] of a per-level table that is a kernel argument, as a select chain: no per-lane index into the arguments.  Level 0 is the start
// value, so a level out of range reads level 0.
__device__ __forceinline__ float level_table(const float (&t)[RFE_MAX_LEVELS], int level) {
    float v = t[0];
#pragma unroll
    for (int l = 1; l < RFE_MAX_LEVELS; ++l) v = level == l ? t[l] : v;
    return v;
}
// MapPoint::PredictScale (src/MapPoint.cc:689-707, 716-732): ceil(log(scale_dist / dist) / log_scale_factor), one rounding per written
// operation, clamped to 0..nlevels - 1 as a float; NaN is level 0
__device__ __forceinline__ int predict_scale_level(float scale_dist, float dist, float log_scale_factor, int nlevels) {
    const float c = ceilf(logf(scale_dist / dist) / log_scale_factor);
    if (!(c > 0.f)) return 0;
    if (c >= (float)nlevels) return nlevels - 1;
    return (int)c;
}

// proj_search.hip: SearchByProjection1 on the device.  cell_start [770], cell_items [Nf], fxy [Nf,2], seg_off [Nq+1],
// cand_idx / cand_dist [cand_cap]
void launch_proj_grid(hipStream_t s, const float* kpts, const int32_t* kxy, int Nf, const int32_t* nf_dev, float min_x, float min_y,
                      float inv_w, float inv_h, int32_t* cell_start, int32_t* cell_items, float* fxy);
void launch_proj_count(hipStream_t s, const float* proj, const float* radius, const int32_t* pred_level, int Nq, const int32_t* cell_start,
                       const int32_t* cell_items, const float* fxy, const int32_t* octave, float min_x, float min_y, float inv_w,
                       float inv_h, int cand_cap, int32_t* seg_off, int32_t* cand_idx, int32_t* stats);
void launch_proj_fill(hipStream_t s, const float* q, int Nq, const float* f, int Nf, const int32_t* seg_off, const int32_t* cand_idx,
                      const uint8_t* skip, float* cand_dist);
void launch_proj_fill_trunc(hipStream_t s, const float* q, int Nq, const float* f, int Nf, const int32_t* seg_off, const int32_t* cand_idx,
                            const uint8_t* skip, float* cand_dist);   // every distance truncated toward zero where it is stored
void launch_proj_resolve(hipStream_t s, const int32_t* seg_off, const int32_t* cand_idx, const float* cand_dist, const uint8_t* observed,
                         int Nq, int Nf, float th_high, int32_t* assign, int32_t* best_idx, float* best_dist, float* second_dist,
                         int32_t* stats);

// proj_sim3.hip: the front of the Sim3 SearchByProjection loops; adds the searched map points to stats[4]
void launch_sim3_project(hipStream_t s, const rfe_sim3_params& P, const float* pw, const float* normal, const float* min_dist,
                         const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np, float* proj, float* radius,
                         int32_t* level, int32_t* reject, int32_t* stats);

// proj_frustum.hip: Frame::isInFrustum and the head of SearchByProjection1 for every local map point; adds the points in
// the frustum to stats[4] and the searched ones to stats[5].  proj_xr / depth / view_cos / reject may be NULL
void launch_frustum_project(hipStream_t s, const rfe_frustum_params& P, const float* pw, const float* normal, const float* min_dist,
                            const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np, float* proj, float* radius,
                            int32_t* level, float* proj_xr, float* depth, float* view_cos, int32_t* reject, int32_t* stats);
// triangulate.hip: CreateNewMapPoints behind the matcher for every match slot of every neighbour.  launch_tri_eval leaves
// code (0 = passed every gate) / x3d / bPointStereo per slot in the workspace and atomicMin's claim [N1] (preset to a value above 63);
// launch_tri_resolve gives the losers code 16, writes the per-slot outputs, the list in creation order (room for N1 entries), matches and
// stats (preset to 0; count [64] too).  Every output but stats may be NULL
void launch_tri_eval(hipStream_t s, const rfe_tri_params& P, const rfe_tri_view& V1, const float* kpts1, const float* kraw1, const int32_t* oct1,
                     const float* ur1, const float* dep1, const uint8_t* mp1, int N1, const rfe_tri_view* views2, const float* kpts2,
                     const float* kraw2, const int32_t* oct2, const float* ur2, const float* dep2, const uint8_t* mp2, const int32_t* n2,
                     const uint8_t* nvalid, int Nn, int N2max, const int32_t* S, const int32_t* pairs, int Kmax, int32_t* wcode, float* wx3d,
                     uint8_t* wstereo, int32_t* claim);
void launch_tri_resolve(hipStream_t s, const int32_t* S, const uint8_t* nvalid, const int32_t* pairs, int N1, int Nn, int Kmax, int32_t* wcode,
                        const float* wx3d, const uint8_t* wstereo, const int32_t* claim, int32_t* count, int32_t* code, float* x3d,
                        uint8_t* point_stereo, int32_t* out_n, int32_t* out_idx1, int32_t* out_idx2, float* out_x3d, uint8_t* out_stereo,
                        int32_t* matches, int32_t* stats);

// bow.hip: Vocabulary::transform and the keyframe database's counts and L1 scores
struct BowVocabDev {
    const int32_t* child_off;   // [n_nodes + 1]
    const int32_t* children;    // [n_nodes - 1]
    const uint8_t* desc;        // [n_nodes, Dp], Dp = D rounded up to 16, zero-padded
    const double* weight;       // [n_nodes]
    const int32_t* word_id;     // [n_nodes]
    int D, Dp, L;
};
constexpr int BOW_MAX_N = 4096;
// per feature the descent: word / node / weight [N]
void launch_bow_descend(hipStream_t s, const BowVocabDev& V, const float* desc_f32, const uint8_t* desc_u8, int N, int levelsup, int32_t* word,
                        int32_t* node, double* weight);
// the two sorted results from the per-feature arrays (1 <= N <= BOW_MAX_N); first_only: IDF / BINARY (addIfNotExist)
void launch_bow_build(hipStream_t s, const int32_t* word, const int32_t* node, const double* weight, int N, bool first_only, int32_t* bow_n,
                      int32_t* bow_word, double* bow_value, int32_t* fv_n, int32_t* fv_node, int32_t* fv_offsets, int32_t* fv_feat);
void launch_bow_db_set_entry(hipStream_t s, long long* start, int32_t* len, int e, long long at, int n);
// counts, then scores; stats [4] preset to 0
void launch_bow_db_query(hipStream_t s, const int32_t* words, const double* values, const long long* start, const int32_t* len, int n_entries,
                         const int32_t* q_word, const double* q_value, int nq, const uint8_t* exclude, int32_t* common, uint8_t* scored,
                         double* score, int32_t* stats);

// pose_opt.hip: Optimizer::PoseOptimization, one workgroup per problem.  octave / uright / n / pose_f32 / chi2 / trace may
// be NULL; needs no workspace and presets nothing
void launch_pose_opt(hipStream_t s, const rfe_pose_params& P, const float* pose0, const float* kpts, const int32_t* octave, const float* uright,
                     const float* xw, const uint8_t* has_mp, const int32_t* n, int B, int N, double* pose, float* pose_f32, uint8_t* outlier,
                     float* chi2, double* trace, int32_t* stats);

// pose_inertial.hip: Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame, one workgroup per problem.  The optional
// pointers of PioArgs may be NULL; needs no workspace and presets nothing
struct PioArgs {
    const int32_t *mode, *rec_init, *octave, *n;
    const float *cam, *state, *prev_state, *preint, *cov_rw, *kpts, *uright, *xw, *track_depth;
    const double* prior_in;
    const uint8_t* has_mp;
    double *state_out, *prior_out, *trace;
    float *state_f32, *chi2;
    uint8_t* outlier;
    int32_t* stats;
    int N;
};
void launch_pose_inertial(hipStream_t s, const rfe_pose_inertial_params& P, const PioArgs& a, int B);
// test hook: the float classification behind round rnd (0..3) or the recovery pass (rnd 4) of a.N edges at the camera pose view [12]; reads
// a.kpts / octave / uright / xw / track_depth, writes a.chi2 and code
void launch_pose_inertial_classify(hipStream_t s, const rfe_pose_inertial_params& P, const PioArgs& a, const double* view, int lf, int rnd,
                                   const uint8_t* outlier_in, const float* chi2_in, uint8_t* code);

// optimize_sim3.hip: Optimizer::OptimizeSim3, one workgroup per problem.  params is a HOST array: the kernel takes it by
// value, OS_CHUNK problems per launch.  octave1 / octave2 / s12_f32 / chi2 / trace may be NULL (kpts2 too when N2 = 0); needs no workspace
// and presets nothing
constexpr int OS_CHUNK = 8;
void launch_optimize_sim3(hipStream_t s, const rfe_optimize_sim3_params* params, const double* s12_0, const float* xw1, const float* xw2,
                          const uint8_t* valid, const float* kpts1, const int32_t* octave1, const int32_t* idx2, const float* kpts2,
                          const int32_t* octave2, int B, int N, int N2, double* s12, float* s12_f32, uint8_t* keep, double* chi2, double* trace,
                          int32_t* stats);

// local_ba.hip: Optimizer::LocalBundleAdjustment, one problem per call, the LM loop on the host (api_local_ba.hip).
// LbaDev: the caller's inputs, the shape, the kernel constants and ws_lba's carving.  ctl_d / ctl_i are one block the host reads with a
// single copy: doubles LBA_D_*, then int32 LBA_I_*
enum { LBA_D_CHI = 0, LBA_D_SCALE = 1, LBA_D_MAXDIAG = 2, LBA_CTL_D = 8 };
enum { LBA_I_STATUS = 0, LBA_I_FLAGS = 1, LBA_I_ERASED = 2, LBA_I_SOLVED = 3, LBA_I_NFREE = 4, LBA_I_NPAIRS = 5, LBA_CTL_I = 16 };
enum { LBA_BAD_RANGE = 1, LBA_BAD_ORDER = 2, LBA_BAD_KF = 4 };
constexpr int LBA_LIN = 54;                          // doubles per edge of lba_linearise_kernel
struct LbaDev {
    const float *kf_pose, *kf_cam, *kf_sigma2, *kpts, *uright, *xw;
    const int32_t *kf_nlevels, *kf_feat_off, *octave, *edge_point, *edge_kf, *edge_feat;
    int P, K, L, E, Nf, NB;                          // NB = P (P + 1) / 2 Schur blocks
    double delta_mono, dsqr_mono, delta_stereo, dsqr_stereo, th2_mono, th2_stereo;
    double* ctl_d; int32_t* ctl_i;
    double *pose[2], *pt[2];                         // [K, 7] and [L, 3], the estimate and the trial
    int32_t *pt_start, *pose_start, *pose_cnt, *pose_list, *blk_start, *blk_cnt, *pairs;
    double *lin, *chi2, *rho0, *Hll, *bl, *Dinv, *db, *xl, *Hpp, *bp, *bs, *xp, *BDinv, *Bdb, *S, *sterm;
};
void lba_launch_validate(hipStream_t s, const LbaDev& d);
void lba_launch_structure(hipStream_t s, const LbaDev& d);
void lba_launch_pairs(hipStream_t s, const LbaDev& d);
void lba_launch_errors(hipStream_t s, const LbaDev& d, int cur, bool linearise, bool max_diagonal);
void lba_launch_trial(hipStream_t s, const LbaDev& d, int cur, double lambda);
void lba_launch_finish(hipStream_t s, const LbaDev& d, int cur, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* erase,
                       double* chi2);

// essential_graph.hip: Optimizer::OptimizeEssentialGraph, the Sim3 pose graph, the LM loop on the host (api_essential_graph.hip; DESIGN.md
// 6m).  EgDev: the caller's inputs, the shape and ws_eg's carving.  ctl_d / ctl_i are one block the host reads with a single copy.  The
// factorisation works on square tiles of EG_TILE rows (EG_TILE_V vertices); NT tiles a side, NP = NT EG_TILE padded rows
constexpr int EG_TILE_V = 4, EG_TILE = 28, EG_CON = 119, EG_JAC = 105;
enum { EG_D_CHI = 0, EG_D_SCALE = 1, EG_D_MAXDIAG = 2, EG_CTL_D = 8 };
enum { EG_I_STATUS = 0, EG_I_FLAGS = 1, EG_I_FAIL = 2, EG_I_NFREE = 3, EG_I_TILES = 4, EG_CTL_I = 16 };
enum { EG_BAD_RANGE = 1, EG_BAD_ORDER = 2, EG_BAD_REF = 4 };
struct EgDev {
    const double *s_est, *s_meas;
    const uint8_t *fixed, *edge_src;
    const int32_t *edge_i, *edge_j, *point_ref;
    const float* xw;
    int N, E, L, fix_scale, Nf, NT, NP;              // Nf, NT, NP: known after the front
    double* ctl_d; int32_t* ctl_i;
    double* est[2];                                  // [N, 8], the estimate and the trial
    double *meas, *pert;                             // [E, 8] Sji; [14, 8] Sim3(+-delta e_d)
    int32_t *free_index, *free_list, *inc_start, *inc_list;   // inc_list: edge * 2 + side, ascending inside a vertex
    int32_t *col_start, *col_tiles, *row_start, *row_tiles;   // per tile column: its non-zero tiles, the diagonal first; per tile row likewise
    uint8_t* fill;                                   // [NT, NT]
    double *jac, *con, *chi2;                        // [EG_JAC, E] e | A | B; [EG_CON, E] Hii | bi | Hjj | bj | Hij; [E]
    double *b, *x, *z, *y, *xs, *dvec, *sterm;       // [NP] each
    double* mat;                                     // [NP, NP]: H in the upper triangle with the diagonal, L strictly below
};
void eg_launch_front(hipStream_t s, const EgDev& d);
void eg_launch_structure(hipStream_t s, const EgDev& d);
void eg_launch_errors(hipStream_t s, const EgDev& d, int cur, bool linearise, bool max_diagonal);
void eg_launch_trial(hipStream_t s, const EgDev& d, int cur, double lambda, const int32_t* col_start, const int32_t* row_start);
void eg_launch_finish(hipStream_t s, const EgDev& d, int cur, double* siw, float* tiw_f32, double* swi, float* xw_out, double* chi2);

// global_ba.hip: Optimizer::BundleAdjustment behind GlobalBundleAdjustemnt, one problem per call, the LM loop on the host
// (api_global_ba.hip): 6l's per-edge terms and Schur complement behind a structure front whose work scales with the pairs,
// and 6m's tiled LDLT (tile_ldlt.h) on GBA_TILE rows, GBA_TILE_V poses a tile.  GbaDev: the caller's inputs, the shape and ws_gba's carving
constexpr int GBA_TILE_V = 4, GBA_TILE = 24;
enum { GBA_D_CHI = 0, GBA_D_SCALE = 1, GBA_D_MAXDIAG = 2, GBA_CTL_D = 8 };
enum { GBA_I_STATUS = 0, GBA_I_FLAGS = 1, GBA_I_FAIL = 2, GBA_I_NFREE = 3, GBA_I_NPAIRS = 4, GBA_I_NBLOCKS = 5, GBA_I_TILES = 6, GBA_CTL_I = 16 };
struct GbaDev {
    const float *kf_pose, *kf_cam, *kf_sigma2, *kpts, *uright, *xw;
    const int32_t *kf_nlevels, *kf_feat_off, *octave, *edge_point, *edge_kf, *edge_feat;
    const uint8_t* fixed;
    int K, L, E, Nf, robust;
    int P, NB, NT, NP;                               // known after the front: free poses, non-empty Schur blocks, tiles a side, padded rows
    double delta_mono, dsqr_mono, delta_stereo, dsqr_stereo;
    double* ctl_d; int32_t* ctl_i;
    double *pose[2], *pt[2];                         // [K, 7] and [L, 3], the estimate and the trial
    int32_t *free_index, *free_list;                 // [K] each
    int32_t *pt_start, *pose_start, *pose_cnt, *pose_list, *pose_tmp;   // [L + 1], [K + 1], [K], [E], [E]
    int32_t *key_cnt, *key_start;                    // [K K]: per dense block key i1 P + i2 the pairs still to place, the list's start
    int32_t *blk_key, *blk_start;                    // [K (K + 1) / 2 (+ 1)]: the non-empty blocks in ascending key
    unsigned long long *pairs, *pairs_tmp;           // [NPAIRS]: e1 << 32 | e2, ascending inside a block
    int32_t *col_start, *col_tiles, *row_start, *row_tiles;
    uint8_t* fill;                                   // [NT, NT]
    double *lin, *chi2, *rho0, *Hll, *bl, *Dinv, *db, *xl, *Hpp, *bp, *xp, *BDinv, *Bdb, *sterm;
    double *b, *z, *y, *xs, *dvec;                   // [NP] each
    double* mat;                                     // [NP, NP]: Hschur in the upper triangle with the diagonal, L strictly below
};
void gba_launch_validate(hipStream_t s, const GbaDev& d);
void gba_launch_count(hipStream_t s, const GbaDev& d);
void gba_launch_structure(hipStream_t s, const GbaDev& d);
void gba_launch_errors(hipStream_t s, const GbaDev& d, int cur, bool linearise, bool max_diagonal);
void gba_launch_trial(hipStream_t s, const GbaDev& d, int cur, double lambda, const int32_t* col_start, const int32_t* row_start);
void gba_launch_finish(hipStream_t s, const GbaDev& d, int cur, double* pose, float* pose_f32, double* point, float* point_f32, uint8_t* included,
                       double* chi2);

// sim3_solver.hip: Sim3Solver's RANSAC with every hypothesis at once.  params is a HOST array: the front takes it by value,
// S3_FRONT_CHUNK problems per launch, and leaves prob [B]; front [B, 12, N], counts [B, H] and hyps [B, H, 32] are workspace (or the
// caller's counts / hyps).  R / t / sc / inliers / best_inliers may be NULL; presets nothing
constexpr int S3_FRONT_CHUNK = 16;
struct Sim3Prob { float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; int32_t fix_scale, min_inliers, its, n; };
void launch_sim3_front(hipStream_t s, const rfe_sim3_solver_params* params, const float* xw1, const float* xw2, const float* sg1, const float* sg2,
                       int B, int N, Sim3Prob* prob, float* front);
void launch_sim3_hypotheses(hipStream_t s, const Sim3Prob* prob, const float* front, const int32_t* draws, int B, int N, int H, int32_t* counts,
                            float* hyps);
void launch_sim3_select(hipStream_t s, const Sim3Prob* prob, const float* front, const int32_t* counts, const float* hyps, int B, int N, int H,
                        float* T12, float* R, float* t, float* sc, uint8_t* inliers, uint8_t* best_inliers, int32_t* stats);

// two_view.hip: TwoViewReconstruction with every RANSAC iteration of both models at once.  params is a HOST array: the front
// takes it by value (B <= TV_MAX_B) and leaves prob [B].  Workspace: soa [B, 4, Ks] the matches' u1 | v1 | u2 | v2 rows (Ks = Kmax rounded up
// to 4: 16-byte loads), sets [B, H, 8], hmodels [B, H, 2, 9] every iteration's H21 | F21, sel [B] the selection's record, winl [B, 2, Kmax]
// the winners' flags, rcode / rcos / rp [B, 8, Kmax (, 3)] CheckRT per motion hypothesis and match; scores [B, H, 2] is the caller's or
// workspace.  Every output but R21, t21 and stats may be NULL; presets nothing
constexpr int TV_MAX_B = 16;
struct TvProb { float fx, fy, cx, cy, invs2, th2, rh_threshold, min_parallax, T1[4], T2[4], T2inv[9]; int32_t min_triangulated, N, its, n1, n2, flags; };
struct TvSel { float cand[8][12], SH, SF, RH; int32_t win_h, win_f, cnt_h, cnt_f, ncand, model, exit, flags; };
struct TvBuffers { TvProb* prob; TvSel* sel; float *soa, *hmodels, *scores, *rcos, *rp; int32_t* sets; uint8_t *winl, *rcode; };
inline int tv_soa_stride(int Kmax) { return (Kmax + 3) & ~3; }
void launch_two_view(hipStream_t s, const rfe_two_view_params* params, const float* kpts1, const float* kpts2, const int32_t* S,
                     const int32_t* pairs, const int32_t* draws, int B, int N1max, int N2max, int Kmax, int H, const TvBuffers& w, float* R21,
                     float* t21, float* p3d, uint8_t* triangulated, uint8_t* inliers_h, uint8_t* inliers_f, float* scores, float* models,
                     float* cand, int32_t* stats);
// the test hooks' kernels: CheckHomography / CheckFundamental of one model (0 H, 1 F) and CheckRT of one (R | t) [12] over pts [n,4]
void launch_two_view_hook_check(hipStream_t s, int model, const float* M9, float invs2, const float* pts, int n, float* contrib, uint8_t* inl);
void launch_two_view_hook_check_rt(hipStream_t s, const float* Rt, float fx, float fy, float cx, float cy, float th2, const float* pts, int n,
                                   uint8_t* code, float* cosp, float* p3d);

}  // namespace rfe
