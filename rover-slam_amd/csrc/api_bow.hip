// api_bow.hip -- C ABI of librover_fe.so: the DBoW3 vocabulary on the device, ComputeBoW3 and the keyframe database's scores (bow.hip,
// DESIGN.md 6h).  The vocabulary checks and the reader of DBoW3's uncompressed binary stream are host code and need no device.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include "api_internal.h"

using namespace rfe;

struct rfe_bow_vocab {
    rfe_ctx* ctx = nullptr;
    int k = 0, L = 0, weighting = 0, scoring = 0, n_nodes = 0, n_words = 0, D = 0, depth = 0;
    void* dev = nullptr;               // one allocation, carved into V's arrays
    BowVocabDev V{};
};

struct rfe_bow_db {
    rfe_ctx* ctx = nullptr;
    int32_t* words = nullptr; double* values = nullptr; size_t cap_words = 0, used_words = 0;
    long long* start = nullptr; int32_t* len = nullptr; int cap_entries = 0;
    std::vector<int32_t> host_len;     // per entry id: its word count, -1 once erased
};

namespace {

constexpr int BOW_MAX_NODES = 1 << 24;

struct BowTree {
    int32_t k = 0, L = 0, weighting = 0, scoring = 0, n_nodes = 0, D = 0;
    std::vector<int32_t> parent, child_off, children, word_id;
    std::vector<uint8_t> desc;
    std::vector<double> weight;
    rfe_bow_vocab_desc view() const {
        return rfe_bow_vocab_desc{k, L, weighting, scoring, n_nodes, D, parent.data(), child_off.data(), children.data(), desc.data(), weight.data(),
                                  word_id.data()};
    }
};

// rfe_bow_vocab_create's refusals; the depth of the deepest leaf and the number of childless nodes on the way
bool bow_validate(const rfe_bow_vocab_desc& d, std::string& err, int* depth_out, int* words_out) {
    auto no = [&](const std::string& m) { err = "bow vocabulary: " + m; return false; };
    if (d.n_nodes < 1 || d.n_nodes > BOW_MAX_NODES) return no("n_nodes outside 1..2^24");
    if (d.D < 8 || d.D > 256 || d.D % 8) return no("D must be a multiple of 8 within 8..256");
    if (d.scoring != RFE_BOW_L1_NORM) return no("only L1_NORM scoring is built");
    if (d.weighting < RFE_BOW_TF_IDF || d.weighting > RFE_BOW_BINARY) return no("weighting outside 0..3");
    if (d.L < 0 || d.k < 0) return no("negative k or L");
    if (!d.parent || !d.child_offsets || !d.desc || !d.weight || !d.word_id || (d.n_nodes > 1 && !d.children)) return no("null array");
    const int n = d.n_nodes;
    if (d.child_offsets[0] != 0 || d.child_offsets[n] != n - 1) return no("child_offsets must run from 0 to n_nodes - 1");
    for (int i = 0; i < n; ++i)
        if (d.child_offsets[i + 1] < d.child_offsets[i]) return no("child_offsets descend at node " + std::to_string(i));
    std::vector<uint8_t> seen(n, 0);
    for (int i = 0; i < n; ++i)
        for (int c = d.child_offsets[i]; c < d.child_offsets[i + 1]; ++c) {
            const int ch = d.children[c];
            if (ch < 1 || ch >= n) return no("child index " + std::to_string(ch) + " of node " + std::to_string(i) + " out of range");
            if (seen[ch]) return no("node " + std::to_string(ch) + " has two parents");
            seen[ch] = 1;
        }
    for (int i = 0; i < n; ++i)
        for (int c = d.child_offsets[i]; c < d.child_offsets[i + 1]; ++c)
            if (d.parent[d.children[c]] != i) return no("parent[" + std::to_string(d.children[c]) + "] disagrees with children[]");
    // every node but the root is somebody's child exactly once; a cycle apart from the root is what is left to find
    std::vector<int32_t> queue(1, 0), level(n, 0);
    queue.reserve(n);
    int depth = 0, words = 0;
    for (size_t h = 0; h < queue.size(); ++h) {
        const int i = queue[h];
        if (d.child_offsets[i] == d.child_offsets[i + 1]) {
            if (d.word_id[i] < 0) return no("childless node " + std::to_string(i) + " has no word id");
            depth = std::max(depth, level[i]);
            ++words;
        }
        for (int c = d.child_offsets[i]; c < d.child_offsets[i + 1]; ++c) { level[d.children[c]] = level[i] + 1; queue.push_back(d.children[c]); }
    }
    if ((int)queue.size() != n) return no(std::to_string(n - (int)queue.size()) + " nodes cannot be reached from the root");
    *depth_out = depth; *words_out = words;
    return true;
}

// DBoW3's binary stream (Vocabulary::toStream / fromStream, DescManip::toStream), uncompressed.  Every read goes through take(), which
// refuses to pass the end of the file, and every count is held against the bytes that are left before anything is sized by it.
bool bow_parse_stream(const char* path, BowTree& T, std::string& err) {
    auto no = [&](const std::string& m) { err = std::string("bow vocabulary ") + (path ? path : "(null)") + ": " + m; return false; };
    if (!path) return no("no path");
    FILE* f = fopen(path, "rb");
    if (!f) return no("cannot open");
    std::vector<uint8_t> buf;
    if (fseek(f, 0, SEEK_END) == 0) {
        const long sz = ftell(f);
        if (sz > 0 && fseek(f, 0, SEEK_SET) == 0) { buf.resize((size_t)sz); if (fread(buf.data(), 1, buf.size(), f) != buf.size()) buf.clear(); }
    }
    fclose(f);
    if (buf.empty()) return no("cannot read");
    size_t at = 0;
    auto take = [&](void* dst, size_t n) { if (n > buf.size() - at) return false; memcpy(dst, buf.data() + at, n); at += n; return true; };
    uint64_t sig = 0; uint8_t compressed = 0; uint32_t nnodes = 0;
    if (!take(&sig, 8) || sig != 88877711233ull) return no("not a DBoW3 binary vocabulary (magic number)");
    if (!take(&compressed, 1) || !take(&nnodes, 4)) return no("truncated header");
    if (compressed) return no("the stream is quicklz-compressed; save it again uncompressed (Vocabulary::save(file, false) / toStream(str, false))");
    if (nnodes < 1 || nnodes > (uint32_t)BOW_MAX_NODES) return no("nnodes outside 1..2^24");
    int32_t hdr[4];
    if (!take(hdr, 16)) return no("truncated header");
    T.k = hdr[0]; T.L = hdr[1]; T.scoring = hdr[2]; T.weighting = hdr[3]; T.n_nodes = (int32_t)nnodes;
    constexpr size_t NODE_MIN = 4 + 4 + 8 + 12;      // id, parent, weight, cols / rows / type
    if ((size_t)(nnodes - 1) > (buf.size() - at) / NODE_MIN) return no("nnodes = " + std::to_string(nnodes) + " is more than the file can hold");
    const int n = (int)nnodes;
    T.parent.assign(n, -1); T.word_id.assign(n, -1); T.weight.assign(n, 0.0);
    std::vector<int32_t> order;                      // node ids in the order of the file: the order of every node's children
    order.reserve(n);
    std::vector<uint8_t> seen(n, 0);
    std::vector<size_t> desc_at(n, 0);
    T.D = 0;
    for (int i = 1; i < n; ++i) {
        uint32_t id, parent; double w; int32_t crt[3];
        if (!take(&id, 4) || !take(&parent, 4) || !take(&w, 8) || !take(crt, 12)) return no("truncated in node record " + std::to_string(i));
        if (id < 1 || id >= nnodes || parent >= nnodes) return no("node record " + std::to_string(i) + ": id or parent out of range");
        if (seen[id]) return no("node " + std::to_string(id) + " occurs twice");
        seen[id] = 1;
        if (crt[2] != 0) return no("node " + std::to_string(id) + ": descriptor type " + std::to_string(crt[2]) + " is not CV_8U");
        if (crt[1] != 1 || crt[0] < 1 || crt[0] > 256) return no("node " + std::to_string(id) + ": descriptor is not one row of 1..256 bytes");
        if (T.D == 0) T.D = crt[0];
        if (crt[0] != T.D) return no("node " + std::to_string(id) + ": descriptor width differs from the first node's");
        if ((size_t)crt[0] > buf.size() - at) return no("truncated in the descriptor of node " + std::to_string(id));
        desc_at[id] = at; at += (size_t)crt[0];
        T.parent[id] = (int32_t)parent; T.weight[id] = w;
        order.push_back((int32_t)id);
    }
    uint32_t nwords = 0;
    if (!take(&nwords, 4)) return no("truncated before the word table");
    if ((size_t)nwords > (buf.size() - at) / 8) return no("word count " + std::to_string(nwords) + " is more than the file can hold");
    for (uint32_t i = 0; i < nwords; ++i) {
        uint32_t wid, nid;
        if (!take(&wid, 4) || !take(&nid, 4)) return no("truncated in the word table");
        if (wid >= nwords || nid >= nnodes) return no("word table entry " + std::to_string(i) + " out of range");
        T.word_id[nid] = (int32_t)wid;
    }
    if (T.D == 0) T.D = 8;                            // a lone root: no descriptor to take the width from
    T.desc.assign((size_t)n * T.D, 0);
    for (int id = 1; id < n; ++id) memcpy(T.desc.data() + (size_t)id * T.D, buf.data() + desc_at[id], T.D);
    T.child_off.assign(n + 1, 0);
    for (int id : order) ++T.child_off[T.parent[id] + 1];
    for (int i = 0; i < n; ++i) T.child_off[i + 1] += T.child_off[i];
    T.children.assign(std::max(n - 1, 1), 0);
    std::vector<int32_t> fill(T.child_off.begin(), T.child_off.end() - 1);
    for (int id : order) T.children[fill[T.parent[id]]++] = id;
    return true;
}

int bow_vocab_upload(rfe_ctx* c, const rfe_bow_vocab_desc& d, rfe_bow_vocab** out) {
    std::string err; int depth = 0, words = 0;
    if (!bow_validate(d, err, &depth, &words)) return fail(c, RFE_ERR_INVALID, err);
    RFE_HIP(c, hipSetDevice(c->device));
    const int n = d.n_nodes, Dp = (d.D + 15) & ~15;
    int32_t *child_off, *children, *word_id; uint8_t* desc; double* weight;
    auto layout = [&](Bump& a) {
        child_off = a.take<int32_t>(n + 1); children = a.take<int32_t>(std::max(n - 1, 1)); word_id = a.take<int32_t>(n);
        weight = a.take<double>(n); desc = a.take<uint8_t>((size_t)n * Dp);
    };
    void* dev = nullptr;
    hipError_t e = hipMalloc(&dev, layout_bytes(layout));
    if (e != hipSuccess) return fail(c, RFE_ERR_OOM, std::string("hipMalloc vocabulary: ") + hipGetErrorString(e));
    Bump a(dev);
    layout(a);
    std::vector<uint8_t> padded((size_t)n * Dp, 0);   // the root's row stays zero: it is never read
    for (int i = 1; i < n; ++i) memcpy(padded.data() + (size_t)i * Dp, d.desc + (size_t)i * d.D, d.D);
    e = hipMemcpy(child_off, d.child_offsets, sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && n > 1) e = hipMemcpy(children, d.children, sizeof(int32_t) * (n - 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(word_id, d.word_id, sizeof(int32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(weight, d.weight, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(desc, padded.data(), padded.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dev); return fail(c, RFE_ERR_HIP, std::string("hipMemcpy vocabulary: ") + hipGetErrorString(e)); }
    rfe_bow_vocab* v = new rfe_bow_vocab();
    v->ctx = c; v->k = d.k; v->L = d.L; v->weighting = d.weighting; v->scoring = d.scoring; v->n_nodes = n; v->n_words = words; v->D = d.D;
    v->depth = depth; v->dev = dev;
    v->V = BowVocabDev{child_off, children, desc, weight, word_id, d.D, Dp, d.L};
    *out = v;
    return RFE_OK;
}

}  // namespace

extern "C" int rfe_bow_vocab_create(rfe_ctx* c, const rfe_bow_vocab_desc* desc, rfe_bow_vocab** out) {
    if (!c) return RFE_ERR_INVALID;
    if (!desc || !out) return fail(c, RFE_ERR_INVALID, "bow_vocab_create: null pointer");
    *out = nullptr;
    return bow_vocab_upload(c, *desc, out);
}

extern "C" int rfe_bow_vocab_load(rfe_ctx* c, const char* path, rfe_bow_vocab** out) {
    if (!c) return RFE_ERR_INVALID;
    if (!out) return fail(c, RFE_ERR_INVALID, "bow_vocab_load: null pointer");
    *out = nullptr;
    BowTree T; std::string err;
    if (!bow_parse_stream(path, T, err)) return fail(c, RFE_ERR_IO, err);
    return bow_vocab_upload(c, T.view(), out);
}

extern "C" void rfe_bow_vocab_destroy(rfe_bow_vocab* v) {
    if (!v) return;
    (void)hipSetDevice(v->ctx->device);
    (void)hipStreamSynchronize(v->ctx->stream);
    if (v->dev) (void)hipFree(v->dev);
    delete v;
}

extern "C" int rfe_bow_vocab_info(const rfe_bow_vocab* v, int32_t* info) {
    if (!v || !info) return RFE_ERR_INVALID;
    const int32_t a[8] = {v->k, v->L, v->n_nodes, v->n_words, v->D, v->weighting, v->scoring, v->depth};
    memcpy(info, a, sizeof(a));
    return RFE_OK;
}

extern "C" int rfe_k_bow_vocab_read(const char* path, int32_t* hdr, int32_t* parent, int32_t* child_offsets, int32_t* children, uint8_t* desc,
                                    double* weight, int32_t* word_id, char* err, int errlen) {
    auto say = [&](const std::string& m, int code) { if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", m.c_str()); return code; };
    if (!hdr) return say("rfe_k_bow_vocab_read: hdr is NULL", RFE_ERR_INVALID);
    BowTree T; std::string e;
    if (!bow_parse_stream(path, T, e)) return say(e, RFE_ERR_IO);
    const int32_t h[6] = {T.k, T.L, T.weighting, T.scoring, T.n_nodes, T.D};
    memcpy(hdr, h, sizeof(h));
    int depth, words;
    if (!bow_validate(T.view(), e, &depth, &words)) return say(e, RFE_ERR_INVALID);
    const size_t n = (size_t)T.n_nodes;
    if (parent) memcpy(parent, T.parent.data(), 4 * n);
    if (child_offsets) memcpy(child_offsets, T.child_off.data(), 4 * (n + 1));
    if (children) memcpy(children, T.children.data(), 4 * (n - 1));
    if (desc) memcpy(desc, T.desc.data(), n * T.D);
    if (weight) memcpy(weight, T.weight.data(), 8 * n);
    if (word_id) memcpy(word_id, T.word_id.data(), 4 * n);
    return say("", RFE_OK);
}

// ---------------------------------------------------------------- transform
static int bow_transform_check(rfe_ctx* c, const rfe_bow_vocab* v, const void* f32, const void* u8, int N, const void* bow_n, const void* bow_word,
                               const void* bow_value, const void* fv_n, const void* fv_node, const void* fv_offsets, const void* fv_feat) {
    if (!v) return fail(c, RFE_ERR_INVALID, "bow_transform: no vocabulary");
    if (v->ctx->device != c->device) return fail(c, RFE_ERR_INVALID, "bow_transform: the vocabulary lives on another device");
    if (N < 0 || N > BOW_MAX_N) return fail(c, RFE_ERR_INVALID, "bow_transform: N outside 0..4096");
    if (N > 0 && (f32 != nullptr) == (u8 != nullptr)) return fail(c, RFE_ERR_INVALID, "bow_transform: exactly one of desc_f32 / desc_u8");
    if (N > 0 && f32 && v->D != 256) return fail(c, RFE_ERR_INVALID, "bow_transform: desc_f32 needs a vocabulary of D = 256");
    if (!bow_n || !fv_n || !fv_offsets || (N > 0 && (!bow_word || !bow_value || !fv_node || !fv_feat)))
        return fail(c, RFE_ERR_INVALID, "bow_transform: null pointer");
    return RFE_OK;
}

extern "C" int rfe_bow_transform_dev(rfe_ctx* c, const rfe_bow_vocab* v, const float* desc_f32, const uint8_t* desc_u8, int N, int levelsup,
                                     int32_t* word, int32_t* node, double* weight, int32_t* bow_n, int32_t* bow_word, double* bow_value,
                                     int32_t* fv_n, int32_t* fv_node, int32_t* fv_offsets, int32_t* fv_feat) {
    if (!c) return RFE_ERR_INVALID;
    int rc = bow_transform_check(c, v, desc_f32, desc_u8, N, bow_n, bow_word, bow_value, fv_n, fv_node, fv_offsets, fv_feat);
    if (rc) return rc;
    if (N > 0 && (((uintptr_t)desc_f32 & 15) || ((uintptr_t)desc_u8 & 7)))
        return fail(c, RFE_ERR_INVALID, "bow_transform: desc_f32 must be 16-byte and desc_u8 8-byte aligned");
    RFE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (N == 0) {
        RFE_HIP(c, hipMemsetAsync(bow_n, 0, 4, s)); RFE_HIP(c, hipMemsetAsync(fv_n, 0, 4, s)); RFE_HIP(c, hipMemsetAsync(fv_offsets, 0, 4, s));
        return RFE_OK;
    }
    int32_t *w_word = nullptr, *w_node = nullptr; double* w_weight = nullptr;
    rc = ws_carve(c, &c->ws_bow, &c->ws_bow_bytes, [&](Bump& a) {
        w_word = a.take<int32_t>(BOW_MAX_N); w_node = a.take<int32_t>(BOW_MAX_N); w_weight = a.take<double>(BOW_MAX_N);
    });
    if (rc) return rc;
    if (word) w_word = word;
    if (node) w_node = node;
    if (weight) w_weight = weight;
    { ProfScope ps(c, "bow_descend");
      launch_bow_descend(s, v->V, desc_f32, desc_u8, N, levelsup, w_word, w_node, w_weight); }
    { ProfScope ps(c, "bow_build");
      launch_bow_build(s, w_word, w_node, w_weight, N, v->weighting == RFE_BOW_IDF || v->weighting == RFE_BOW_BINARY, bow_n, bow_word, bow_value,
                       fv_n, fv_node, fv_offsets, fv_feat); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_bow_transform(rfe_ctx* c, const rfe_bow_vocab* v, const float* desc_f32, const uint8_t* desc_u8, int N, int levelsup,
                                 int32_t* word, int32_t* node, double* weight, int32_t* bow_n, int32_t* bow_word, double* bow_value, int32_t* fv_n,
                                 int32_t* fv_node, int32_t* fv_offsets, int32_t* fv_feat) {
    if (!c) return RFE_ERR_INVALID;
    int rc = bow_transform_check(c, v, desc_f32, desc_u8, N, bow_n, bow_word, bow_value, fv_n, fv_node, fv_offsets, fv_feat);
    if (rc) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    float* df = nullptr; uint8_t* du = nullptr; int32_t *dword, *dnode, *dcnt, *dbw, *dfn, *dfo, *dff; double *dweight, *dbv;
    HostIo io(c, HostIo::DIRECT);
    if (N > 0 && desc_f32) io.in(df, desc_f32, (size_t)N * 256);
    if (N > 0 && desc_u8) io.in(du, desc_u8, (size_t)N * v->D);
    io.out_opt(dword, word, N); io.out_opt(dnode, node, N); io.out_opt(dweight, weight, N);
    io.scratch(dcnt, 2); io.scratch(dbw, N); io.scratch(dbv, N); io.scratch(dfn, N); io.scratch(dfo, (size_t)N + 1); io.scratch(dff, N);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_bow_transform_dev(c, v, df, du, N, levelsup, dword, dnode, dweight, dcnt, dbw, dbv, dcnt + 1, dfn, dfo, dff))) return rc;
    int32_t cnt[2] = {0, 0};
    RFE_HIP(c, hipMemcpyAsync(cnt, dcnt, 8, hipMemcpyDeviceToHost, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    // only what the counts cover comes back: the caller's arrays stay as they were past them
    const int nb = std::min(std::max(cnt[0], 0), N), nf = std::min(std::max(cnt[1], 0), N);
    *bow_n = nb; *fv_n = nf;
    if (nb) { RFE_HIP(c, hipMemcpyAsync(bow_word, dbw, 4 * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
              RFE_HIP(c, hipMemcpyAsync(bow_value, dbv, 8 * (size_t)nb, hipMemcpyDeviceToHost, c->stream)); }
    RFE_HIP(c, hipMemcpyAsync(fv_offsets, dfo, 4 * ((size_t)nf + 1), hipMemcpyDeviceToHost, c->stream));
    if (nf) RFE_HIP(c, hipMemcpyAsync(fv_node, dfn, 4 * (size_t)nf, hipMemcpyDeviceToHost, c->stream));
    if ((rc = io.download())) return rc;                                // waits for the stream
    const int kept = std::min(std::max(fv_offsets[nf], 0), N);
    if (kept) { RFE_HIP(c, hipMemcpyAsync(fv_feat, dff, 4 * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
                RFE_HIP(c, hipStreamSynchronize(c->stream)); }
    return nb;
}

// ---------------------------------------------------------------- keyframe database
static int db_grow(rfe_bow_db* db, size_t need_words, int need_entries) {
    rfe_ctx* c = db->ctx;
    if (need_words > db->cap_words) {
        size_t cap = std::max<size_t>(db->cap_words * 2, (size_t)1 << 16);
        while (cap < need_words) cap *= 2;
        int32_t* w = nullptr; double* v = nullptr;
        if (hipMalloc((void**)&w, cap * 4) != hipSuccess || hipMalloc((void**)&v, cap * 8) != hipSuccess) {
            if (w) (void)hipFree(w);
            (void)hipGetLastError();
            return fail(c, RFE_ERR_OOM, "bow_db: hipMalloc of the word store failed");
        }
        if (db->used_words) {
            RFE_HIP(c, hipMemcpyAsync(w, db->words, db->used_words * 4, hipMemcpyDeviceToDevice, c->stream));
            RFE_HIP(c, hipMemcpyAsync(v, db->values, db->used_words * 8, hipMemcpyDeviceToDevice, c->stream));
        }
        RFE_HIP(c, hipStreamSynchronize(c->stream));
        if (db->words) (void)hipFree(db->words);
        if (db->values) (void)hipFree(db->values);
        db->words = w; db->values = v; db->cap_words = cap;
    }
    if (need_entries > db->cap_entries) {
        int cap = std::max(db->cap_entries * 2, 256);
        while (cap < need_entries) cap *= 2;
        long long* st = nullptr; int32_t* ln = nullptr;
        if (hipMalloc((void**)&st, (size_t)cap * 8) != hipSuccess || hipMalloc((void**)&ln, (size_t)cap * 4) != hipSuccess) {
            if (st) (void)hipFree(st);
            (void)hipGetLastError();
            return fail(c, RFE_ERR_OOM, "bow_db: hipMalloc of the entry table failed");
        }
        const size_t n = db->host_len.size();
        if (n) {
            RFE_HIP(c, hipMemcpyAsync(st, db->start, n * 8, hipMemcpyDeviceToDevice, c->stream));
            RFE_HIP(c, hipMemcpyAsync(ln, db->len, n * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        RFE_HIP(c, hipStreamSynchronize(c->stream));
        if (db->start) (void)hipFree(db->start);
        if (db->len) (void)hipFree(db->len);
        db->start = st; db->len = ln; db->cap_entries = cap;
    }
    return RFE_OK;
}

extern "C" int rfe_bow_db_create(rfe_ctx* c, rfe_bow_db** out) {
    if (!c) return RFE_ERR_INVALID;
    if (!out) return fail(c, RFE_ERR_INVALID, "bow_db_create: out is NULL");
    rfe_bow_db* db = new rfe_bow_db();
    db->ctx = c;
    *out = db;
    return RFE_OK;
}

extern "C" void rfe_bow_db_destroy(rfe_bow_db* db) {
    if (!db) return;
    (void)hipSetDevice(db->ctx->device);
    (void)hipStreamSynchronize(db->ctx->stream);
    for (void* p : {(void*)db->words, (void*)db->values, (void*)db->start, (void*)db->len}) if (p) (void)hipFree(p);
    delete db;
}

extern "C" int rfe_bow_db_add_dev(rfe_bow_db* db, const int32_t* word, const double* value, int n, int32_t* entry_id) {
    if (!db) return RFE_ERR_INVALID;
    rfe_ctx* c = db->ctx;
    if (n < 0 || n > BOW_MAX_N) return fail(c, RFE_ERR_INVALID, "bow_db_add: n outside 0..4096");
    if (n > 0 && (!word || !value)) return fail(c, RFE_ERR_INVALID, "bow_db_add: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    const int e = (int)db->host_len.size();
    const int rc = db_grow(db, db->used_words + (size_t)n, e + 1);
    if (rc) return rc;
    if (n) {
        RFE_HIP(c, hipMemcpyAsync(db->words + db->used_words, word, 4 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        RFE_HIP(c, hipMemcpyAsync(db->values + db->used_words, value, 8 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    }
    launch_bow_db_set_entry(c->stream, db->start, db->len, e, (long long)db->used_words, n);
    RFE_HIP(c, hipGetLastError());
    db->used_words += (size_t)n;
    db->host_len.push_back(n);
    if (entry_id) *entry_id = e;
    return RFE_OK;
}

extern "C" int rfe_bow_db_add(rfe_bow_db* db, const int32_t* word, const double* value, int n, int32_t* entry_id) {
    if (!db) return RFE_ERR_INVALID;
    rfe_ctx* c = db->ctx;
    if (n < 0 || n > BOW_MAX_N) return fail(c, RFE_ERR_INVALID, "bow_db_add: n outside 0..4096");
    if (n > 0 && (!word || !value)) return fail(c, RFE_ERR_INVALID, "bow_db_add: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    int32_t* dw; double* dv;
    HostIo io(c, HostIo::DIRECT);
    io.in(dw, word, n); io.in(dv, value, n);
    int rc = io.upload();
    if (rc) return rc;
    if ((rc = rfe_bow_db_add_dev(db, dw, dv, n, entry_id))) return rc;
    return io.download();                                               // the staging area is free again when this returns
}

extern "C" int rfe_bow_db_erase(rfe_bow_db* db, int32_t e) {
    if (!db) return RFE_ERR_INVALID;
    rfe_ctx* c = db->ctx;
    if (e < 0 || (size_t)e >= db->host_len.size()) return fail(c, RFE_ERR_INVALID, "bow_db_erase: no such entry");
    if (db->host_len[e] < 0) return RFE_OK;
    RFE_HIP(c, hipSetDevice(c->device));
    launch_bow_db_set_entry(c->stream, db->start, db->len, e, 0, 0);
    RFE_HIP(c, hipGetLastError());
    db->host_len[e] = -1;
    return RFE_OK;
}

extern "C" int rfe_bow_db_clear(rfe_bow_db* db) {
    if (!db) return RFE_ERR_INVALID;
    db->host_len.clear();                                               // the store keeps its size; queries in flight have their own launch arguments
    db->used_words = 0;
    return RFE_OK;
}

extern "C" int rfe_bow_db_size(const rfe_bow_db* db) { return db ? (int)db->host_len.size() : RFE_ERR_INVALID; }

extern "C" int rfe_bow_db_query_dev(rfe_bow_db* db, const int32_t* q_word, const double* q_value, int nq, const uint8_t* exclude, int32_t* common,
                                    uint8_t* scored, double* score, int32_t* stats) {
    if (!db) return RFE_ERR_INVALID;
    rfe_ctx* c = db->ctx;
    const int E = (int)db->host_len.size();
    if (nq < 0 || nq > BOW_MAX_N) return fail(c, RFE_ERR_INVALID, "bow_db_query: nq outside 0..4096");
    if (!stats || (nq > 0 && (!q_word || !q_value)) || (E > 0 && (!common || !scored || !score)))
        return fail(c, RFE_ERR_INVALID, "bow_db_query: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    RFE_HIP(c, hipMemsetAsync(stats, 0, 16, c->stream));
    { ProfScope ps(c, "bow_db_query");
      launch_bow_db_query(c->stream, db->words, db->values, db->start, db->len, E, q_word, q_value, nq, exclude, common, scored, score, stats); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_bow_db_query(rfe_bow_db* db, const int32_t* q_word, const double* q_value, int nq, const uint8_t* exclude, int32_t* common,
                                uint8_t* scored, double* score, int32_t* stats) {
    if (!db) return RFE_ERR_INVALID;
    rfe_ctx* c = db->ctx;
    const size_t E = db->host_len.size();
    if (nq < 0 || nq > BOW_MAX_N) return fail(c, RFE_ERR_INVALID, "bow_db_query: nq outside 0..4096");
    if (!stats || (nq > 0 && (!q_word || !q_value)) || (E > 0 && (!common || !scored || !score)))
        return fail(c, RFE_ERR_INVALID, "bow_db_query: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    int32_t *dqw, *dcommon, *dstats; double *dqv, *dscore; uint8_t *dex, *dscored;
    HostIo io(c, HostIo::DIRECT);
    io.in(dqw, q_word, nq); io.in(dqv, q_value, nq); io.in_opt(dex, exclude, E);
    io.out(dcommon, common, E); io.out(dscored, scored, E); io.out(dstats, stats, 4);
    io.scratch(dscore, E);
    int rc = io.upload();
    if (rc) return rc;
    // the scores go in as the caller has them, so that the ones the query does not write come back unchanged
    if (E) RFE_HIP(c, hipMemcpyAsync(dscore, score, 8 * E, hipMemcpyHostToDevice, c->stream));
    if ((rc = rfe_bow_db_query_dev(db, dqw, dqv, nq, dex, dcommon, dscored, dscore, dstats))) return rc;
    if (E) RFE_HIP(c, hipMemcpyAsync(score, dscore, 8 * E, hipMemcpyDeviceToHost, c->stream));
    if ((rc = io.download())) return rc;
    return stats[3];
}
