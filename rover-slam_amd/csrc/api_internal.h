// api_internal.h -- what the api_*.hip files (the C ABI of librover_fe.so, split by pipeline) share among themselves: workspace layouts,
// staging of host-pointer entries, the host graph, and the forward passes of the two pipelines.  Kernel files need rfe_internal.h alone.
#pragma once
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include "rfe_internal.h"

namespace rfe {

inline size_t al(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// neither infinite nor NaN: the test the host entries make of their float arguments, over one value, n values, an array or a list
inline bool finite(float v) { return v - v == 0.f; }
inline bool finite(const float* p, size_t n) { for (size_t i = 0; i < n; ++i) if (!finite(p[i])) return false; return true; }
template <size_t N> bool finite(const float (&a)[N]) { return finite(a, N); }
inline bool finite(std::initializer_list<float> v) { return finite(v.begin(), v.size()); }

// Bump allocator over a workspace.  A layout is ONE function that takes a Bump and the shape and fills its pointer struct; run on a Bump
// without a base it only advances `off` (the pointers come back null), and that is the layout's byte count -- so the size a workspace is
// grown to and the walk that carves it cannot differ.
struct Bump {
    char* base; size_t off = 0;
    explicit Bump(void* b) : base((char*)b) {}
    template <typename T> T* take(size_t n) { T* p = base ? (T*)(base + off) : nullptr; off += al(n * sizeof(T)); return p; }
};
template <typename F> size_t layout_bytes(F&& layout) { Bump m(nullptr); layout(m); return m.off; }
// grow the workspace *ws to what `layout` takes (ensure_ws: synchronises and frees when it grows), then carve it
template <typename F> int ws_carve(rfe_ctx* c, void** ws, size_t* cur, F&& layout) {
    const int rc = ensure_ws(c, ws, cur, layout_bytes(layout));
    if (rc) return rc;
    Bump a(*ws);
    layout(a);
    return RFE_OK;
}

int ensure_pin(rfe_ctx* c, size_t need);
bool is_lib_pinned(const void* p, size_t bytes);

// Staging of a host-pointer entry through ws_io.  The entry declares every array once -- device pointer to fill, host pointer, element count -- in the
// order the copies are to be issued; upload() sizes ws_io (and h_pin) from the declarations, fills the device pointers and copies the inputs, download()
// copies the outputs, waits for the ctx stream and collects the profile.  An array of zero elements is carved (one byte at least, so every device pointer
// is distinct) and not copied, and so is an output whose host pointer is null; the *_opt forms leave the device pointer null when the host one is.
//   PINNED (the per-frame entries: extract, match; see ensure_pin): the inputs are copied into h_pin, the pinned mirror of ws_io, and go in with one DMA per
//     run (cut() ends a run); the outputs, contiguous on the device, come back with one DMA and are scattered on the host.  An output declared `to_caller`
//     that lies in rfe_host_malloc memory is written there by the DMA engine instead, which splits the run around it.  A run of several arrays is copied
//     as laid out, padding included; a lone array at its exact size.
//   DIRECT: one hipMemcpyAsync (image(): one hipMemcpy2DAsync) per array on the caller's memory.
struct HostIo {
    enum Transport { PINNED, DIRECT };
    HostIo(rfe_ctx* ctx, Transport transport) : c(ctx), t(transport) {}
    template <typename T> void in(T*& dev, const T* host, size_t n) { add(ins, n_in, (void**)&dev, host, n * sizeof(T), true); }
    template <typename T> void in_opt(T*& dev, const T* host, size_t n) { add(ins, n_in, (void**)&dev, host, n * sizeof(T), host != nullptr); }
    // `rows` rows of row_bytes, `pitch` bytes apart on the host, tight on the device: a cv::Mat ROI has pitch > row_bytes and its last row ends row_bytes
    // into the pitch, so only row_bytes of every row are read (rows * pitch bytes from the first pixel would run past a ROI at the bottom of its parent buffer)
    template <typename T> void image(T*& dev, const T* host, size_t row_bytes, size_t rows, size_t pitch) {
        add(ins, n_in, (void**)&dev, host, row_bytes * rows, true);
        ins[n_in - 1].row_bytes = row_bytes; ins[n_in - 1].pitch = pitch;
    }
    void cut() { ins[n_in - 1].cut = true; }
    template <typename T> void out(T*& dev, T* host, size_t n, bool to_caller = false) {
        add(outs, n_out, (void**)&dev, host, n * sizeof(T), true);
        outs[n_out - 1].to_caller = to_caller && t == PINNED && is_lib_pinned(host, n * sizeof(T));
    }
    template <typename T> void out_opt(T*& dev, T* host, size_t n) { add(outs, n_out, (void**)&dev, host, n * sizeof(T), host != nullptr); }
    template <typename T> void scratch(T*& dev, size_t n) { add(outs, n_out, (void**)&dev, nullptr, n * sizeof(T), true); }   // device only, never copied
    int upload();
    int download();

private:
    struct Item { void** dev; void* host; char* p; size_t bytes, row_bytes, pitch; bool carve, cut, to_caller; };
    static constexpr int MAX_ITEMS = 20;               // rfe_triangulate_neighbours stages 17 inputs
    void add(Item* v, int& n, void** dev, const void* host, size_t bytes, bool carve) {
        if (n >= MAX_ITEMS) abort();
        v[n++] = Item{dev, const_cast<void*>(host), nullptr, bytes, 0, 0, carve, false, false};
    }
    void layout(Bump& a);
    static size_t run_bytes(const Item* first, const Item* last) { return first == last ? first->bytes : (size_t)(last->p - first->p) + al(last->bytes); }
    rfe_ctx* c; Transport t;
    Item ins[MAX_ITEMS], outs[MAX_ITEMS]; int n_in = 0, n_out = 0;
};

// RFE_OPT_HOST_GRAPH: run `enqueue` (the kernel launches of a host entry, on c->stream and -- forked and joined by events -- c->side_stream) as a replayed
// hipGraph.  A key is everything the kernel arguments bake in (shape, thresholds, workspace addresses, settings_gen).  The first HOST_GRAPH_REPEATS - 1
// calls of a key are ordinary launches (workspaces grow, function attributes are set -- neither is legal inside a capture -- and a shape that never
// comes back never pays a capture); the next one runs under hipStreamBeginCapture, is instantiated into one of four LRU slots, and launched; from then on
// one hipGraphLaunch per call.  Alternating shapes (left / right, stereo sizes) keep their graphs; a caller whose keypoint counts differ on every frame
// gets ordinary launches throughout -- the option only helps FIXED-CAPACITY callers (counts saturating Kmax, or padded to it).  Profiling and the test
// tap fall back to ordinary launches, and so does a failed capture or instantiation: the option never changes results, only how the work is submitted.
constexpr int HOST_GRAPH_REPEATS = 3;
template <typename F>
int run_host_graph(rfe_ctx* c, rfe_ctx::HostGraph& g, const std::string& key, F&& enqueue) {
    if (!c->opt_host_graph || c->prof || c->tap.armed) return enqueue();
    ++g.tick;
    for (auto& sl : g.slot)
        if (sl.exec && sl.key == key) { sl.used = g.tick; RFE_HIP(c, hipGraphLaunch(sl.exec, c->stream)); return RFE_OK; }
    rfe_ctx::HostGraph::Seen* sn = nullptr;
    for (auto& q : g.seen) if (q.count > 0 && q.key == key) sn = &q;
    if (!sn) {                                         // a new key takes the least recently used history entry
        sn = &g.seen[0];
        for (auto& q : g.seen) if (q.used < sn->used) sn = &q;
        sn->key = key; sn->count = 0;
    }
    sn->used = g.tick;
    if (++sn->count < HOST_GRAPH_REPEATS) return enqueue();
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); sn->count = 0; return enqueue(); }
    const int rc = enqueue();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc != RFE_OK || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        sn->count = 0;
        return rc != RFE_OK ? rc : enqueue();          // nothing ran during the capture: submit it the ordinary way
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess || !exec) { (void)hipGetLastError(); sn->count = 0; return enqueue(); }
    rfe_ctx::HostGraph::Slot* sl = &g.slot[0];
    for (auto& q : g.slot) { if (!q.exec) { sl = &q; break; } if (q.used < sl->used) sl = &q; }
    if (sl->exec) (void)hipGraphExecDestroy(sl->exec);
    sl->exec = exec; sl->key = key; sl->used = g.tick;
    sn->count = 0; sn->key.clear();                    // the history entry is free again: the slot remembers the key now
    RFE_HIP(c, hipGraphLaunch(sl->exec, c->stream));
    return RFE_OK;
}
std::string host_graph_key(const rfe_ctx* c, const char* kind, std::initializer_list<long long> v);

// ---------------------------------------------------------------- rfe_triangulate_neighbours* (api_triangulate.hip)
// ws_tri: per slot the code, the point and bPointStereo between the kernels; claim [N1] and count [64], which every call presets
struct TriBuffers { int32_t *code, *claim, *count; float* x3d; uint8_t* stereo; };
inline void tri_layout(Bump& a, int N1, int Nn, int Kmax, TriBuffers& b) {
    const size_t slots = std::max<size_t>((size_t)Nn * Kmax, 1);
    b.claim = a.take<int32_t>(std::max(N1, 1)); b.count = a.take<int32_t>(64);
    b.code = a.take<int32_t>(slots); b.x3d = a.take<float>(slots * 3); b.stereo = a.take<uint8_t>(slots);
}

// ---------------------------------------------------------------- GEMM argument builders (api_extract.hip, api_match.hip)
GemmArgs gemm_plain(const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K);
GemmArgs gemm_lg(const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K);
GemmArgs gemm_lgw(const rfe_ctx* c, const float* A, int lda, const float* Bw, int ldb, const float* bias, float* C, int ldc, int M, int N, int K);

// ---------------------------------------------------------------- SuperPoint pipeline (api_extract.hip)
struct SpBuffers {
    float *p1, *a2, *p2, *a3, *p3, *a4, *f4, *pa, *logits, *da, *dmap, *smap, *nmap, *ss;
    uint8_t *mask, *supp;
    float* cand_score; int32_t* cand_idx;
    unsigned long long* sel_keys; int32_t* sel_n;     // selected (score, pixel) keys between select_kernel and select_rank_kernel
    bool tail_fused = false;                          // sp_tail_lat_kernel ran: candidates are 64-bit keys at cand_score (cand_score | cand_idx = 8 B per pixel)
    // sparse descriptor head (sp_desc_rows): cell -> row within its frame, row -> cell, cell_cnt = [B] rows per frame then [B + 1] their prefix sums;
    // patch = the gathered conv input [rows, 1152], rows <= B cap, which ALIASES p1 | a2 (dead once conv2b has run; B cap 1152 <= B (HW / 64) 1152 =
    // 18 HW floats of the 32 HW the two hold)
    int32_t *cell_row, *row_cell, *cell_cnt; float* patch;
};
// rows per frame the sparse descriptor head can need: four cells per keypoint, every cell of the map at most
inline int sp_desc_cap(int Kmax, int Hc, int Wc) { return std::min(4 * Kmax, Hc * Wc); }
size_t sp_ws_bytes(int B, int H, int W);
int sp_carve(rfe_ctx* c, int B, int H, int W, SpBuffers& b);    // grows ws_sp to its layout and carves it
int sp_check(rfe_ctx* c, int H, int W, int B, int Kmax);
int sp_forward_maps(rfe_ctx* c, const void* img, int H, int W, int stride, int B, SpBuffers& b, bool join, bool& forked, bool img_f32 = false,
                    long long frame_step = 0 /*pixels from frame b to b + 1; 0 = stride * H*/, float thr = 0.0005f /*candidate threshold of the fused tail*/,
                    bool want_maps = false /*test hook: the fused tail also writes the score map and the NMS'ed map*/,
                    bool dense_head = true /*false: no descriptor head; the caller runs sp_desc_rows behind its selection*/);
int sp_desc_rows(rfe_ctx* c, SpBuffers& b, int B, int Hc, int Wc, int Kmax, const int32_t* n, const int32_t* kxy);   // sparse descriptor head: b.dmap = the frames' rows back to back
int sp_forward(rfe_ctx* c, const void* img, int H, int W, int stride, int B, int Kmax, float thr,
               int32_t* n, int32_t* kxy, float* score, float* desc, uint8_t* desc_bin = nullptr, bool img_f32 = false, long long frame_step = 0);

struct PyrPlan {
    int L = 0, Ktot = 0;
    int32_t h[RFE_MAX_LEVELS], w[RFE_MAX_LEVELS]; float s[RFE_MAX_LEVELS];
    int kmax[RFE_MAX_LEVELS]; bool run[RFE_MAX_LEVELS];
    size_t off[RFE_MAX_LEVELS];   // level l's plane inside one frame of the level buffer
    size_t frame = 0;             // sum_l H_l * W_l
};
int pyr_check(rfe_ctx* c, int H, int W, int stride, int B, int L, float sf, const int32_t* kmax, PyrPlan& P);
int pyr_prepare(rfe_ctx* c, int H, int W, int B, float sf, const PyrPlan& P, bool own_levels);
int pyr_forward(rfe_ctx* c, const uint8_t* img, int H, int W, int stride, int B, const PyrPlan& P, float thr, uint8_t* lv, bool copy_level0,
                int32_t* n, int32_t* level_n, float* kpts, int32_t* octave, float* score, float* desc, long long img_frame = 0);

// ---------------------------------------------------------------- LightGlue pipeline (api_match.hip)
struct LgBuffers {
    float *x, *kn, *csn, *lnstat, *qkv, *ctx, *msg, *h, *md, *z, *sim, *rowlse, *collse, *mx0, *apart;
    float* slog;   // cross blocks' shared logits (lg_cross_slog_floats), or null: the generic form.  sim is its first quarter (dead until the assignment)
    int32_t *a0, *a1, *lens, *kvmap;
};
// whether a forward on P pairs of L runs its cross blocks in the shared-logit form -- and therefore whether the workspace holds slog
inline bool lg_cross_shared(const rfe_ctx* c, int P, int L) { return !c->opt_lg_fp16x2 && lg_cross_shared_ok(P, L); }
void lg_layout(Bump& a, int P, int L, LgBuffers& b, bool shared);             // ws_lg
inline size_t lg_ws_bytes(const rfe_ctx* c, int P, int L) { LgBuffers b; return layout_bytes([&](Bump& a) { lg_layout(a, P, L, b, lg_cross_shared(c, P, L)); }); }
// grows ws_lg and carves it: the fixed buffers, then whatever `extra` takes from the same Bump (a caller's own scratch)
template <typename X> int lg_carve_as(rfe_ctx* c, int P, int L, LgBuffers& b, bool shared, X&& extra) {
    return ws_carve(c, &c->ws_lg, &c->ws_lg_bytes, [&](Bump& a) { lg_layout(a, P, L, b, shared); extra(a); });
}
template <typename X> int lg_carve(rfe_ctx* c, int P, int L, LgBuffers& b, X&& extra) { return lg_carve_as(c, P, L, b, lg_cross_shared(c, P, L), extra); }
inline int lg_carve(rfe_ctx* c, int P, int L, LgBuffers& b) { return lg_carve(c, P, L, b, [](Bump&) {}); }
int lg_check(rfe_ctx* c, int P, int Mmax, int Nmax);
void lg_ffn(rfe_ctx* c, LgBuffers& b, float* x, const float* second, int rows, const float* w1, const float* b1, const float* g,
            const float* be, const float* w2, const float* b2);
// both directions of a cross block on [qk | v] rows of stride ld in the side-major layout -> out [2 P L, 256]: the shared-logit form when b.slog was carved
void lg_cross_attention(rfe_ctx* c, LgBuffers& b, const float* qk_v, int ld, float* out, int P, int L);
bool lg_self_qkv_attention(rfe_ctx* c, LgBuffers& b, const LgLayerDev& Lw, const float* x, const float* csn, const int32_t* lens, int nseq, int L);
void lg_self_block(rfe_ctx* c, LgBuffers& b, const LgLayerDev& Lw, float* x, const float* csn, const int32_t* lens, int nseq, int L);
int lg_forward(rfe_ctx* c, LgBuffers& b, int P, int L, float thr, int cap, int32_t* S, int32_t* pairs, float* ms,
               float* scores_opt, bool first_self_done = false, bool posenc_done = false);
void lg_assign_stage(hipStream_t s, LgBuffers& b, int P, int L, float thr, int cap, int32_t* S, int32_t* pairs, float* ms,
                     float* scores_opt, int scores_pair /*launch_lg_assign's*/, const float* wm, const float* bm);
int lg_stage(rfe_ctx* c, LgBuffers& b, const float* k0n, const float* k1n, const float* d0, const float* d1,
             const int32_t* m, const int32_t* n, int P, int Mmax, int Nmax, int L);

}  // namespace rfe
