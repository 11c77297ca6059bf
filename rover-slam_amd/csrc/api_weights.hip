// api_weights.hip -- C ABI of librover_fe.so: weight blobs (set / load / hyper-parameters) and the device copies every ctx of the process shares.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <mutex>
#include <tuple>
#include "api_internal.h"

using namespace rfe;

// =====================================================================================
// weights
// =====================================================================================
extern "C" int64_t rfe_weight_count(int kind) {
    return kind == RFE_KIND_SUPERPOINT ? SP_COUNT : kind == RFE_KIND_LIGHTGLUE ? LG_COUNT : -1;
}

// Read-only weights are shared: Rover-SLAM keeps 2-3 extractors and 3 matchers per process, each with a private runner
// (src/Tracking.cc:645-651, :70; LocalMapping.cc:45; LoopClosing.cc:46).  Every ctx that loads the same blob on the same
// device points at ONE device copy (looked up by device, kind and a 64-bit FNV-1a hash of the floats, and CONFIRMED by comparing
// the blob with the host copy the entry keeps: two different blobs with one hash get two entries); the copy is freed when the
// last ctx holding it is destroyed or loads something else.
namespace {
struct SpShared {
    rfe::SpWeightsDev w; int device = 0; std::vector<float> host;
    ~SpShared() {
        (void)hipSetDevice(device);
        if (w.conv1a_w) (void)hipFree(w.conv1a_w);
        if (w.da_rows) (void)hipFree(w.da_rows);
        for (int l = 0; l < 12; ++l) { if (w.packed[l]) (void)hipFree(w.packed[l]); if (w.bias[l]) (void)hipFree(w.bias[l]); }
    }
};
struct LgShared {
    rfe::LgWeightsDev w; int device = 0; std::vector<float> host;
    ~LgShared() { (void)hipSetDevice(device); if (w.blob) (void)hipFree(w.blob); if (w.extra) (void)hipFree(w.extra); if (w.h2) (void)hipFree(w.h2); }
};
std::mutex g_weights_mu;
std::map<std::tuple<int, int, uint64_t, int>, std::weak_ptr<void>> g_weights;   // (device, kind, hash, collision index) -> device copy

uint64_t fnv1a64(const float* p, size_t n) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n * sizeof(float); ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
}  // namespace

static int upload(rfe_ctx* c, float** dst, const float* src, size_t n) {
    if (*dst) { RFE_HIP(c, hipFree(*dst)); *dst = nullptr; }
    RFE_HIP(c, hipMalloc((void**)dst, n * sizeof(float)));
    RFE_HIP(c, hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return RFE_OK;
}

static int set_sp_upload(rfe_ctx* c, const float* blob);
static int set_lg_upload(rfe_ctx* c, const float* blob);

// one device copy per (device, kind, blob): found by hash and confirmed by contents, or uploaded and entered
template <typename Shared, typename Dev>
static int set_shared(rfe_ctx* c, int kind, const float* blob, size_t count, std::shared_ptr<void>& hold, Dev& dev, bool& has, int (*upload_fn)(rfe_ctx*, const float*)) {
    const uint64_t hash = fnv1a64(blob, count);
    std::lock_guard<std::mutex> lk(g_weights_mu);
    auto key = std::make_tuple(c->device, kind, hash, 0);
    for (;; ++std::get<3>(key)) {   // same hash, different contents -> next collision index
        auto it = g_weights.find(key);
        if (it == g_weights.end()) break;
        auto sp = it->second.lock();
        if (!sp) break;             // expired entry: reuse its slot
        if (memcmp(static_cast<Shared*>(sp.get())->host.data(), blob, count * sizeof(float)) != 0) continue;
        hold = sp; dev = static_cast<Shared*>(sp.get())->w; has = true;
        return RFE_OK;
    }
    has = false; hold.reset(); dev = Dev();
    int rc = upload_fn(c, blob);
    auto sp = std::make_shared<Shared>();
    sp->w = dev; sp->device = c->device;      // takes ownership of whatever was allocated, also after a partial failure
    if (rc) { dev = Dev(); return rc; }
    sp->host.assign(blob, blob + count);
    hold = sp; g_weights[key] = sp;
    return RFE_OK;
}
static int set_sp(rfe_ctx* c, const float* blob) {
    return set_shared<SpShared>(c, RFE_KIND_SUPERPOINT, blob, (size_t)SP_COUNT, c->sp_hold, c->sp, c->has_sp, set_sp_upload);
}
static int set_lg(rfe_ctx* c, const float* blob) {
    return set_shared<LgShared>(c, RFE_KIND_LIGHTGLUE, blob, (size_t)LG_COUNT, c->lg_hold, c->lg, c->has_lg, set_lg_upload);
}

static int set_sp_upload(rfe_ctx* c, const float* blob) {
    size_t off = 0;
    for (int l = 0; l < 12; ++l) {
        const SpLayer& L = kSpLayers[l];
        const float* w = blob + off;
        const size_t wn = (size_t)L.cout * L.cin * L.k * L.k;
        const float* b = w + wn;
        off += wn + L.cout;
        int rc;
        if (l == L_1A) {
            std::vector<float> t(9 * 64);
            for (int co = 0; co < 64; ++co) for (int k = 0; k < 9; ++k) t[k * 64 + co] = w[co * 9 + k];
            if ((rc = upload(c, &c->sp.conv1a_w, t.data(), t.size()))) return rc;
        } else if (L.k == 3) {
            std::vector<float> t;
            pack_conv3x3_weights(w, L.cin, L.cout, L.pool, t);
            if ((rc = upload(c, &c->sp.packed[l], t.data(), t.size()))) return rc;
            if (l == L_DA && (rc = upload(c, &c->sp.da_rows, w, wn))) return rc;   // [256][1152] as-is, for the sparse descriptor head
        } else {
            if ((rc = upload(c, &c->sp.packed[l], w, wn))) return rc;  // [N][K] as-is
        }
        if ((rc = upload(c, &c->sp.bias[l], b, L.cout))) return rc;
    }
    c->has_sp = true;
    return RFE_OK;
}

static int set_lg_upload(rfe_ctx* c, const float* blob) {
    int rc = upload(c, &c->lg.blob, blob, (size_t)LG_COUNT);
    if (rc) return rc;
    size_t taken = 0;
    auto take = [&](size_t n) { float* r = c->lg.blob + taken; taken += n; return r; };
    LgWeightsDev& W = c->lg;
    W.wr = take(64);
    for (int l = 0; l < LG_LAYERS; ++l) {
        LgLayerDev& L = W.L[l];
        L.wqkv = take(768 * 256); L.bqkv = take(768); L.wo = take(256 * 256); L.bo = take(256);
        L.w1 = take(512 * 512); L.b1 = take(512); L.lng = take(512); L.lnb = take(512);
        L.w2 = take(256 * 512); L.b2 = take(256);
        L.cwqk = take(256 * 256); L.cbqk = take(256); L.cwv = take(256 * 256); L.cbv = take(256);
        L.cwo = take(256 * 256); L.cbo = take(256);
        L.cw1 = take(512 * 512); L.cb1 = take(512); L.clng = take(512); L.clnb = take(512);
        L.cw2 = take(256 * 512); L.cb2 = take(256);
    }
    W.wp = take(256 * 256); W.bp = take(256); W.wm = take(256); W.bm = take(1);
    if (taken != (size_t)LG_COUNT) return fail(c, RFE_ERR_INVALID, "internal: LightGlue blob layout mismatch");
    // derived weights, built once at load time:
    //  * the two cross-attention input projections of every layer packed into one [512][256] Linear;
    //  * the attention output projection (Wo, bo) folded into the message half of the first FFN Linear:
    //    the message m = ctx Wo^T + bo only ever feeds ffn.0, so  W1 [x | m] + b1 = [W1a | W1b Wo] [x | ctx] + (b1 + W1b bo).
    //    The product is formed in double precision on the host; it removes 18 of the 19 256x256 GEMM launches
    //    per forward (mathematically identical, rounding differs at the 1e-7 level; RFE_LG_NO_FOLD=1 keeps them).
    if (W.extra) { RFE_HIP(c, hipFree(W.extra)); W.extra = nullptr; }
    const size_t per = 512 * 256 + 512 + 2 * (512 * 512 + 512);
    RFE_HIP(c, hipMalloc((void**)&W.extra, per * LG_LAYERS * sizeof(float)));
    {
        std::vector<float> w1f(512 * 512), b1f(512);
        std::vector<double> acc(256);
        size_t off = 64;   // host blob walk, same order as above (Wr first)
        for (int l = 0; l < LG_LAYERS; ++l) {
            LgLayerDev& L = W.L[l];
            float* base = W.extra + per * l + 512 * 256 + 512;
            L.w1f = base; L.b1f = base + 512 * 512; L.cw1f = L.b1f + 512; L.cb1f = L.cw1f + 512 * 512;
            const float* h = blob + off;
            const float* s_wo = h + 768 * 256 + 768; const float* s_bo = s_wo + 256 * 256;
            const float* s_w1 = s_bo + 256; const float* s_b1 = s_w1 + 512 * 512;
            const float* cr = s_b1 + 512 + 512 + 512 + 256 * 512 + 256;           // start of the cross block
            const float* c_wo = cr + 2 * (256 * 256 + 256); const float* c_bo = c_wo + 256 * 256;
            const float* c_w1 = c_bo + 256; const float* c_b1 = c_w1 + 512 * 512;
            off += 1250560;   // floats per layer (self 658176 + cross 592384)
            for (int blk = 0; blk < 2; ++blk) {
                const float* wo = blk ? c_wo : s_wo; const float* bo = blk ? c_bo : s_bo;
                const float* w1 = blk ? c_w1 : s_w1; const float* b1 = blk ? c_b1 : s_b1;
                for (int i = 0; i < 512; ++i) {
                    const float* w1row = w1 + (size_t)i * 512;
                    for (int j = 0; j < 256; ++j) { w1f[(size_t)i * 512 + j] = w1row[j]; acc[j] = 0.0; }
                    double bacc = b1[i];
                    for (int k = 0; k < 256; ++k) {
                        const double wv = w1row[256 + k];
                        const float* worow = wo + (size_t)k * 256;
                        for (int j = 0; j < 256; ++j) acc[j] += wv * (double)worow[j];
                        bacc += wv * (double)bo[k];
                    }
                    for (int j = 0; j < 256; ++j) w1f[(size_t)i * 512 + 256 + j] = (float)acc[j];
                    b1f[i] = (float)bacc;
                }
                RFE_HIP(c, hipMemcpy(blk ? L.cw1f : L.w1f, w1f.data(), w1f.size() * 4, hipMemcpyHostToDevice));
                RFE_HIP(c, hipMemcpy(blk ? L.cb1f : L.b1f, b1f.data(), b1f.size() * 4, hipMemcpyHostToDevice));
            }
        }
    }
    for (int l = 0; l < LG_LAYERS; ++l) {
        LgLayerDev& L = W.L[l];
        L.cwqkv = W.extra + per * l; L.cbqkv = L.cwqkv + 512 * 256;
        RFE_HIP(c, hipMemcpy(L.cwqkv, L.cwqk, 256 * 256 * 4, hipMemcpyDeviceToDevice));
        RFE_HIP(c, hipMemcpy(L.cwqkv + 256 * 256, L.cwv, 256 * 256 * 4, hipMemcpyDeviceToDevice));
        RFE_HIP(c, hipMemcpy(L.cbqkv, L.cbqk, 256 * 4, hipMemcpyDeviceToDevice));
        RFE_HIP(c, hipMemcpy(L.cbqkv + 256, L.cbv, 256 * 4, hipMemcpyDeviceToDevice));
    }
    // fp16 (hi, lo) planes of both weight buffers for RFE_OPT_LG_FP16X2 (gemm_h2.hip): split once here, 2 x 2 bytes per float
    if (W.h2) { RFE_HIP(c, hipFree(W.h2)); W.h2 = nullptr; }
    W.n_blob = ((size_t)LG_COUNT + 63) & ~(size_t)63; W.n_extra = per * LG_LAYERS;     // plane starts stay 128-byte aligned (LG_COUNT is odd)
    RFE_HIP(c, hipMalloc((void**)&W.h2, 2 * (W.n_blob + W.n_extra) * sizeof(uint16_t)));
    launch_split_f16(c->stream, W.blob, W.h2, W.h2 + W.n_blob, (size_t)LG_COUNT);
    launch_split_f16(c->stream, W.extra, W.h2 + 2 * W.n_blob, W.h2 + 2 * W.n_blob + W.n_extra, W.n_extra);
    RFE_HIP(c, hipGetLastError());
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    c->has_lg = true;
    return RFE_OK;
}

// the fields of one model kind, from one set of hyper-parameters to another
static void take_hparams(rfe_hparams& to, const rfe_hparams& from, int kind) {
    if (kind == RFE_KIND_SUPERPOINT) {
        to.sp_max_keypoints = from.sp_max_keypoints; to.sp_detection_threshold = from.sp_detection_threshold; to.sp_nms_radius = from.sp_nms_radius;
        to.sp_remove_borders = from.sp_remove_borders; to.sp_topk_always = from.sp_topk_always;
    } else {
        to.lg_layers = from.lg_layers; to.lg_heads = from.lg_heads; to.lg_filter_threshold = from.lg_filter_threshold;
    }
}

extern "C" int rfe_set_weights(rfe_ctx* c, int kind, const float* blob, int64_t count) {
    if (!c || !blob) return fail(c, RFE_ERR_INVALID, "rfe_set_weights: null argument");
    RFE_HIP(c, hipSetDevice(c->device));
    if (count != rfe_weight_count(kind)) return fail(c, RFE_ERR_INVALID, "rfe_set_weights: wrong float count for this model kind");
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    const int rc = kind == RFE_KIND_SUPERPOINT ? set_sp(c, blob) : set_lg(c, blob);
    ++c->settings_gen;
    if (rc == RFE_OK) {
        // hyper-parameters belong to a weight set: a bare blob (and a version-1 file) carries none, so this kind's values go back to the published
        // defaults -- a v2 load followed by rfe_set_weights must not keep the earlier file's radius / border / top-k rule silently (rover_fe.h)
        take_hparams(c->hp, rfe_default_hparams(), kind);
    }
    return rc;
}

extern "C" uint64_t rfe_weights_id(rfe_ctx* c, int kind) {
    if (!c) return 0;
    const void* p = kind == RFE_KIND_SUPERPOINT ? c->sp_hold.get() : kind == RFE_KIND_LIGHTGLUE ? c->lg_hold.get() : nullptr;
    return (uint64_t)(uintptr_t)p;
}

// RFEW container (rover-slam_amd/weights.py).  Both versions: "RFEW" | u32 version | u32 kind | u64 float count.
//   version 1: the floats follow.
//   version 2: u32 hp_bytes | hp_bytes of graph hyper-parameters | the floats.  Hyper-parameter block (little endian):
//     kind 1 (SuperPoint): i32 max_keypoints, f32 detection_threshold, i32 nms_radius, i32 remove_borders, i32 topk_always   (20 bytes)
//     kind 2 (LightGlue):  i32 layers, i32 heads, f32 filter_threshold                                     (12 bytes)
//   A longer block (a later writer) is accepted, its known prefix used.
static int check_hparams(rfe_ctx* c, const rfe_hparams& h, const char* who) {
    if (h.sp_max_keypoints < 1 || h.sp_max_keypoints > 4096) return fail(c, RFE_ERR_INVALID, std::string(who) + ": sp_max_keypoints must be in 1..4096");
    if (!(h.sp_detection_threshold >= 0.f) || !(h.sp_detection_threshold < 1.f)) return fail(c, RFE_ERR_INVALID, std::string(who) + ": sp_detection_threshold must be in [0, 1)");
    if (h.sp_nms_radius < 1 || h.sp_nms_radius > NMS_MAX_RADIUS) return fail(c, RFE_ERR_INVALID, std::string(who) + ": sp_nms_radius must be in 1.." + std::to_string(NMS_MAX_RADIUS));
    if (h.sp_remove_borders < 0 || h.sp_remove_borders > 64) return fail(c, RFE_ERR_INVALID, std::string(who) + ": sp_remove_borders must be in 0..64");
    if (h.sp_topk_always != 0 && h.sp_topk_always != 1) return fail(c, RFE_ERR_INVALID, std::string(who) + ": sp_topk_always must be 0 or 1");
    if (h.lg_layers != LG_LAYERS || h.lg_heads != 4)
        return fail(c, RFE_ERR_INVALID, std::string(who) + ": the LightGlue kernels are built for 9 layers of 4 heads x 64, the file / caller says " +
                                        std::to_string(h.lg_layers) + " layers of " + std::to_string(h.lg_heads) + " heads");
    if (!(h.lg_filter_threshold >= 0.f) || !(h.lg_filter_threshold < 1.f)) return fail(c, RFE_ERR_INVALID, std::string(who) + ": lg_filter_threshold must be in [0, 1)");
    return RFE_OK;
}

static int load_rfew(rfe_ctx* c, const char* path, int want_kind) {
    FILE* f = fopen(path, "rb");
    if (!f) return fail(c, RFE_ERR_IO, std::string("cannot open weight file ") + path);
    unsigned char head[20];
    if (fread(head, 1, 20, f) != 20 || memcmp(head, "RFEW", 4) != 0) { fclose(f); return fail(c, RFE_ERR_IO, std::string("not an RFEW file: ") + path); }
    uint32_t ver, kind; uint64_t cnt;
    memcpy(&ver, head + 4, 4); memcpy(&kind, head + 8, 4); memcpy(&cnt, head + 12, 8);
    if ((ver != 1 && ver != 2) || (int)kind != want_kind || (int64_t)cnt != rfe_weight_count(want_kind)) { fclose(f); return fail(c, RFE_ERR_IO, std::string("RFEW header mismatch in ") + path); }
    rfe_hparams hp = c->hp;
    if (ver == 2) {
        uint32_t hb = 0;
        unsigned char blk[256];
        const uint32_t need = want_kind == RFE_KIND_SUPERPOINT ? 20u : 12u;
        if (fread(&hb, 4, 1, f) != 1 || hb < need || hb > sizeof(blk) || fread(blk, 1, hb, f) != hb) { fclose(f); return fail(c, RFE_ERR_IO, std::string("RFEW v2 hyper-parameter block damaged in ") + path); }
        if (want_kind == RFE_KIND_SUPERPOINT) {
            memcpy(&hp.sp_max_keypoints, blk, 4); memcpy(&hp.sp_detection_threshold, blk + 4, 4);
            memcpy(&hp.sp_nms_radius, blk + 8, 4); memcpy(&hp.sp_remove_borders, blk + 12, 4); memcpy(&hp.sp_topk_always, blk + 16, 4);
        } else {
            memcpy(&hp.lg_layers, blk, 4); memcpy(&hp.lg_heads, blk + 4, 4); memcpy(&hp.lg_filter_threshold, blk + 8, 4);
        }
        const int rc = check_hparams(c, hp, path);
        if (rc) { fclose(f); c->err = "RFEW v2 hyper-parameters refused: " + c->err; return RFE_ERR_IO; }
    }
    std::vector<float> blob(cnt);
    size_t got = fread(blob.data(), sizeof(float), cnt, f);
    fclose(f);
    if (got != cnt) return fail(c, RFE_ERR_IO, std::string("short read on ") + path);
    const int rc = rfe_set_weights(c, want_kind, blob.data(), (int64_t)cnt);      // resets this kind's hyper-parameters to the defaults
    if (rc == RFE_OK && ver == 2) take_hparams(c->hp, hp, want_kind);             // the file's hyper-parameters travel with its weights
    return rc;
}

extern "C" int rfe_get_hparams(rfe_ctx* c, rfe_hparams* out) {
    if (!c || !out) return RFE_ERR_INVALID;
    *out = c->hp;
    return RFE_OK;
}
extern "C" int rfe_set_hparams(rfe_ctx* c, const rfe_hparams* in) {
    if (!c || !in) return RFE_ERR_INVALID;
    const int rc = check_hparams(c, *in, "rfe_set_hparams");
    if (rc) return rc;
    c->hp = *in;
    ++c->settings_gen;
    return RFE_OK;
}

// An ONNX graph file (the reference's own onnxmodel/superpoint.onnx / lightglue_sim.onnx, src/Extractors/SPextractor.cc:92-94,
// src/Matchers/lightglue_onnx.cpp:38): initializers -> canonical blob, graph constants -> hyper-parameters (onnx_load.hip), then exactly what an RFEW
// v2 file does.  A graph whose hyper-parameters cannot be read is refused with the reason (RFE_ERR_IO).
static int load_onnx(rfe_ctx* c, const char* path, int want_kind) {
    std::vector<float> blob;
    rfe_hparams hp = rfe_default_hparams();
    std::string err;
    if (!rfe::onnx_convert(path, want_kind, blob, &hp, err)) return fail(c, RFE_ERR_IO, err);
    int rc = check_hparams(c, hp, path);
    if (rc) { c->err = "graph hyper-parameters refused: " + c->err; return RFE_ERR_IO; }
    if ((int64_t)blob.size() != rfe_weight_count(want_kind)) return fail(c, RFE_ERR_IO, std::string("converted weight count mismatch for ") + path);
    rc = rfe_set_weights(c, want_kind, blob.data(), (int64_t)blob.size());   // resets this kind's hyper-parameters to the defaults
    if (rc == RFE_OK) take_hparams(c->hp, hp, want_kind);
    return rc;
}

// RFEW container or ONNX graph, told apart by the file's first four bytes
static int load_any(rfe_ctx* c, const char* path, int want_kind) {
    FILE* f = fopen(path, "rb");
    if (!f) return fail(c, RFE_ERR_IO, std::string("cannot open weight file ") + path);
    unsigned char magic[4] = {0, 0, 0, 0};
    const size_t got = fread(magic, 1, 4, f);
    fclose(f);
    if (got == 4 && memcmp(magic, "RFEW", 4) == 0) return load_rfew(c, path, want_kind);
    return load_onnx(c, path, want_kind);
}

static int load_pair(rfe_ctx* c, const char* sp_path, const char* lg_path, int (*load)(rfe_ctx*, const char*, int)) {
    if (!c) return RFE_ERR_INVALID;
    int rc;
    if (sp_path && (rc = load(c, sp_path, RFE_KIND_SUPERPOINT))) return rc;
    if (lg_path && (rc = load(c, lg_path, RFE_KIND_LIGHTGLUE))) return rc;
    return RFE_OK;
}
extern "C" int rfe_load_weights(rfe_ctx* c, const char* sp_path, const char* lg_path) { return load_pair(c, sp_path, lg_path, load_any); }
extern "C" int rfe_load_onnx(rfe_ctx* c, const char* sp_path, const char* lg_path) { return load_pair(c, sp_path, lg_path, load_onnx); }
