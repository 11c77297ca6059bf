// api_ctx.hip -- the part of the C ABI of librover_fe.so (see include/rover_fe.h for the reference interface each entry point replaces) that
// belongs to no pipeline: context lifetime, options, memory, the grow-only workspaces and their pinned mirror, staging of host-pointer
// entries, the host graph, profiling.  Host-side orchestration only, like every api_*.hip; no CPU compute path.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include "api_internal.h"

using namespace rfe;

static std::string g_init_error;
static std::mutex g_mu;

namespace rfe {

int fail(rfe_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else { std::lock_guard<std::mutex> l(g_mu); g_init_error = msg; }
    return code;
}

int ensure_ws(rfe_ctx* c, void** p, size_t* cur, size_t need) {
    if (need <= *cur) return RFE_OK;
    if (*p) { RFE_HIP(c, hipStreamSynchronize(c->stream)); RFE_HIP(c, hipFree(*p)); *p = nullptr; *cur = 0; }
    need = (need + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) return fail(c, RFE_ERR_OOM, std::string("hipMalloc workspace: ") + hipGetErrorString(e));
    *cur = need;
    return RFE_OK;
}

// Pinned host staging (grow-only) for the host-pointer entries a tracking thread calls once per frame: the caller's arrays are pageable
// (std::vector, cv::Mat), and a hipMemcpyAsync on pageable memory is a synchronous, internally staged copy PER CALL -- four to six of them per
// entry.  Packing the inputs into one pinned block (one DMA in) and fetching the contiguous device results with one DMA out, then scattering
// on the host -- together with the runner writing straight into its output tensors -- measured through the drop-in classes (bench.py
// latency.dropin): one frame 0.914 -> 0.793 ms, one pair 3.28 -> 2.99 ms, one stereo frame 3.43 -> 3.25 ms (profiles/r04_ab_notes.md).
int ensure_pin(rfe_ctx* c, size_t need) {
    if (need <= c->h_pin_bytes) return RFE_OK;
    if (c->h_pin) { RFE_HIP(c, hipStreamSynchronize(c->stream)); RFE_HIP(c, hipHostFree(c->h_pin)); c->h_pin = nullptr; c->h_pin_bytes = 0; }
    need = (need + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
    hipError_t e = hipHostMalloc(&c->h_pin, need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, RFE_ERR_OOM, std::string("hipHostMalloc staging: ") + hipGetErrorString(e));
    c->h_pin_bytes = need;
    return RFE_OK;
}

// Host blocks handed out by rfe_host_malloc (pinned, portable): a host entry whose descriptor output lies inside one of them lets the DMA engine write
// the K x 256 floats straight into the caller's memory instead of staging them through h_pin and copying 1 MB on the host afterwards.
static std::mutex g_pin_mu;
static std::vector<std::pair<char*, size_t>> g_pin_blocks;
bool is_lib_pinned(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (const auto& b : g_pin_blocks)
        if ((const char*)p >= b.first && (const char*)p + bytes <= b.first + b.second) return true;
    return false;
}

static void host_graph_release(rfe_ctx::HostGraph& g) {
    for (auto& sl : g.slot) { if (sl.exec) (void)hipGraphExecDestroy(sl.exec); sl.exec = nullptr; sl.key.clear(); }
    for (auto& q : g.seen) { q.key.clear(); q.count = 0; }
}
std::string host_graph_key(const rfe_ctx* c, const char* kind, std::initializer_list<long long> v) {
    std::string k = kind;
    for (long long x : v) { k += '|'; k += std::to_string(x); }
    k += "|g" + std::to_string(c->settings_gen) + "|" + std::to_string((unsigned long long)(uintptr_t)c->ws_sp) + "|" + std::to_string((unsigned long long)(uintptr_t)c->ws_lg) +
         "|" + std::to_string((unsigned long long)(uintptr_t)c->ws_io) + "|" + std::to_string((unsigned long long)(uintptr_t)c->sp_hold.get()) + "|" +
         std::to_string((unsigned long long)(uintptr_t)c->lg_hold.get());
    return k;
}

ProfScope::ProfScope(rfe_ctx* ctx, const char* name, hipStream_t on) : c(ctx), idx(-1), st(on ? on : ctx->stream) {
    if (!c->prof) return;
    if (!c->prof_filter.empty() && c->prof_filter != name) return;
    for (size_t i = 0; i < c->stages.size(); ++i) if (c->stages[i].name == name) idx = (int)i;
    if (idx < 0) { c->stages.push_back(Stage{name, 0, 0}); idx = (int)c->stages.size() - 1; }
    auto get = [&]() { hipEvent_t e; if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
    e0 = get(); e1 = get();
    (void)hipEventRecord(e0, st);
}
ProfScope::~ProfScope() {
    if (idx < 0) return;
    (void)hipEventRecord(e1, st);
    c->pending.push_back({idx, {e0, e1}});
}
void prof_collect(rfe_ctx* c) {
    for (auto& p : c->pending) {
        float ms = 0.f;
        (void)hipEventSynchronize(p.second.second);
        (void)hipEventElapsedTime(&ms, p.second.first, p.second.second);
        c->stages[p.first].ms += ms; c->stages[p.first].calls += 1;
        c->ev_pool.push_back(p.second.first); c->ev_pool.push_back(p.second.second);
    }
    c->pending.clear();
}

void HostIo::layout(Bump& a) {
    for (Item* v : {ins, outs})
        for (Item* it = v; it < v + (v == ins ? n_in : n_out); ++it) {
            it->p = it->carve ? a.take<char>(std::max<size_t>(it->bytes, 1)) : nullptr;
            *it->dev = it->p;
        }
}

int HostIo::upload() {
    int rc;
    if (t == PINNED && (rc = ensure_pin(c, layout_bytes([&](Bump& a) { layout(a); })))) return rc;
    if ((rc = ws_carve(c, &c->ws_io, &c->ws_io_bytes, [&](Bump& a) { layout(a); }))) return rc;
    hipStream_t s = c->stream;
    if (t == DIRECT) {
        for (Item* it = ins; it < ins + n_in; ++it) {
            if (!it->p || !it->bytes) continue;
            if (it->pitch) RFE_HIP(c, hipMemcpy2DAsync(it->p, it->row_bytes, it->host, it->pitch, it->row_bytes, it->bytes / it->row_bytes, hipMemcpyHostToDevice, s));
            else RFE_HIP(c, hipMemcpyAsync(it->p, it->host, it->bytes, hipMemcpyHostToDevice, s));
        }
        return RFE_OK;
    }
    char* dev0 = (char*)c->ws_io; char* hp = (char*)c->h_pin;
    for (Item *first = ins, *it = ins; it < ins + n_in; ++it) {
        char* h = hp + (it->p - dev0);
        if (it->pitch) for (size_t r = 0; r < it->bytes / it->row_bytes; ++r) memcpy(h + r * it->row_bytes, (const char*)it->host + r * it->pitch, it->row_bytes);
        else if (it->p && it->bytes) memcpy(h, it->host, it->bytes);
        if (it->cut || it + 1 == ins + n_in) {
            RFE_HIP(c, hipMemcpyAsync(first->p, hp + (first->p - dev0), run_bytes(first, it), hipMemcpyHostToDevice, s));
            first = it + 1;
        }
    }
    return RFE_OK;
}

int HostIo::download() {
    hipStream_t s = c->stream;
    char* dev0 = (char*)c->ws_io; char* hp = (char*)c->h_pin;
    const Item* end = outs + n_out;
    if (t == DIRECT) {
        for (const Item* it = outs; it < end; ++it)
            if (it->host && it->p && it->bytes) RFE_HIP(c, hipMemcpyAsync(it->host, it->p, it->bytes, hipMemcpyDeviceToHost, s));
    } else {
        for (const Item* it = outs; it < end; ++it) {
            if (!it->p) continue;
            if (it->to_caller) { RFE_HIP(c, hipMemcpyAsync(it->host, it->p, it->bytes, hipMemcpyDeviceToHost, s)); continue; }
            const Item* last = it;                       // the run of staged outputs that starts here: one DMA into the mirror
            while (last + 1 < end && last[1].p && !last[1].to_caller) ++last;
            RFE_HIP(c, hipMemcpyAsync(hp + (it->p - dev0), it->p, run_bytes(it, last), hipMemcpyDeviceToHost, s));
            it = last;
        }
    }
    RFE_HIP(c, hipStreamSynchronize(s));
    if (t == PINNED)
        for (const Item* it = outs; it < end; ++it)
            if (it->host && it->p && it->bytes && !it->to_caller) memcpy(it->host, hp + (it->p - dev0), it->bytes);
    prof_collect(c);
    return RFE_OK;
}

}  // namespace rfe

// =====================================================================================
// lifetime
// =====================================================================================
extern "C" const char* rfe_version(void) { return "rover-fe 0.1 (gfx950)"; }

extern "C" const char* rfe_last_error(rfe_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    return g_init_error.c_str();
}

extern "C" int rfe_init(int device, rfe_ctx** out) {
    if (!out) return fail(nullptr, RFE_ERR_INVALID, "rfe_init: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, RFE_ERR_NO_DEVICE, "rfe_init: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(nullptr, RFE_ERR_INVALID, "rfe_init: device index out of range");
    if ((e = hipSetDevice(device)) != hipSuccess)
        return fail(nullptr, RFE_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return fail(nullptr, RFE_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, RFE_ERR_NO_DEVICE, std::string("rfe_init: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    rfe_ctx* c = new rfe_ctx();
    c->device = device;
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return fail(nullptr, RFE_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    if ((e = hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_pyr, hipEventDisableTiming)) != hipSuccess) {
        rfe_destroy(c);
        return fail(nullptr, RFE_ERR_HIP, std::string("hipStreamCreate/hipEventCreate: ") + hipGetErrorString(e));
    }
    *out = c;
    return RFE_OK;
}

extern "C" void rfe_destroy(rfe_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    host_graph_release(c->g_extract);
    host_graph_release(c->g_match);
    auto fr = [](void* p) { if (p) (void)hipFree(p); };
    c->sp_hold.reset(); c->lg_hold.reset();   // the last ctx holding a device copy frees it
    fr(c->ws_sp); fr(c->ws_lg); fr(c->ws_io); fr(c->ws_tmp); fr(c->ws_st); fr(c->ws_ps); fr(c->ws_tri); fr(c->ws_bow); fr(c->ws_s3); fr(c->ws_tv); fr(c->ws_lba); fr(c->ws_lba_pairs); fr(c->ws_eg); fr(c->ws_eg_mat); fr(c->ws_gba); fr(c->ws_gba_pairs); fr(c->ws_gba_mat); fr(c->sp_cnt); fr(c->ws_pyr); fr(c->ws_ptab);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    if (c->h_lba) (void)hipHostFree(c->h_lba);
    if (c->h_eg) (void)hipHostFree(c->h_eg);
    if (c->h_gba) (void)hipHostFree(c->h_gba);
    if (c->side_stream) { (void)hipStreamSynchronize(c->side_stream); (void)hipStreamDestroy(c->side_stream); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_pyr) (void)hipEventDestroy(c->ev_pyr);
    (void)hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" int rfe_set_option(rfe_ctx* c, int option, int value) {
    if (!c) return RFE_ERR_INVALID;
    switch (option) {
        case RFE_OPT_LG_FOLD_WO: c->opt_lg_fold = value != 0; ++c->settings_gen; return RFE_OK;
        case RFE_OPT_LG_FP16X2: c->opt_lg_fp16x2 = value != 0; ++c->settings_gen; return RFE_OK;
        case RFE_OPT_HOST_GRAPH: c->opt_host_graph = value != 0; return RFE_OK;
        default: return fail(c, RFE_ERR_INVALID, "rfe_set_option: unknown option");
    }
}
extern "C" int rfe_get_option(rfe_ctx* c, int option, int* value) {
    if (!c || !value) return RFE_ERR_INVALID;
    switch (option) {
        case RFE_OPT_LG_FOLD_WO: *value = c->opt_lg_fold ? 1 : 0; return RFE_OK;
        case RFE_OPT_LG_FP16X2: *value = c->opt_lg_fp16x2 ? 1 : 0; return RFE_OK;
        case RFE_OPT_HOST_GRAPH: *value = c->opt_host_graph ? 1 : 0; return RFE_OK;
        default: return fail(c, RFE_ERR_INVALID, "rfe_get_option: unknown option");
    }
}

extern "C" int rfe_set_stream(rfe_ctx* c, void* s) {
    if (!c) return RFE_ERR_INVALID;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return RFE_OK;
}
extern "C" int rfe_synchronize(rfe_ctx* c) {
    if (!c) return RFE_ERR_INVALID;
    RFE_HIP(c, hipSetDevice(c->device));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return RFE_OK;
}
extern "C" int rfe_malloc(rfe_ctx* c, size_t bytes, void** p) {
    if (!c || !p) return RFE_ERR_INVALID;
    RFE_HIP(c, hipSetDevice(c->device));
    hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(c, RFE_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return RFE_OK;
}
extern "C" int rfe_free(rfe_ctx* c, void* p) {
    if (!c) return RFE_ERR_INVALID;
    RFE_HIP(c, hipSetDevice(c->device));
    RFE_HIP(c, hipFree(p));
    return RFE_OK;
}
extern "C" int rfe_memcpy_h2d(rfe_ctx* c, void* d, const void* s, size_t n) {
    if (!c) return RFE_ERR_INVALID;
    RFE_HIP(c, hipSetDevice(c->device));
    RFE_HIP(c, hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}
extern "C" int rfe_memcpy_d2h(rfe_ctx* c, void* d, const void* s, size_t n) {
    if (!c) return RFE_ERR_INVALID;
    RFE_HIP(c, hipSetDevice(c->device));
    RFE_HIP(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, c->stream));
    RFE_HIP(c, hipStreamSynchronize(c->stream));
    return RFE_OK;
}

extern "C" int rfe_host_malloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return RFE_ERR_INVALID;
    *out = nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return RFE_ERR_OOM; }
    { std::lock_guard<std::mutex> lk(g_pin_mu); g_pin_blocks.push_back({(char*)p, bytes}); }
    *out = p;
    return RFE_OK;
}
extern "C" void rfe_host_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = 0; i < g_pin_blocks.size(); ++i)
            if (g_pin_blocks[i].first == (char*)p) { g_pin_blocks.erase(g_pin_blocks.begin() + i); break; }
    }
    (void)hipHostFree(p);
}

extern "C" int64_t rfe_workspace_bytes(rfe_ctx* c) {
    return c ? (int64_t)(c->ws_sp_bytes + c->ws_lg_bytes + c->ws_io_bytes + c->ws_tmp_bytes + c->ws_st_bytes + c->ws_ps_bytes + c->ws_tri_bytes + c->ws_bow_bytes + c->ws_s3_bytes + c->ws_tv_bytes + c->ws_lba_bytes + c->ws_lba_pairs_bytes + c->ws_eg_bytes + c->ws_eg_mat_bytes + c->ws_gba_bytes + c->ws_gba_pairs_bytes + c->ws_gba_mat_bytes + c->ws_pyr_bytes + c->ws_ptab_bytes) : 0;
}

// =====================================================================================
// profiling
// =====================================================================================
extern "C" int rfe_profile_enable(rfe_ctx* c, int on) { if (!c) return RFE_ERR_INVALID; c->prof = on != 0; return RFE_OK; }
extern "C" int rfe_profile_filter(rfe_ctx* c, const char* stage) {
    if (!c) return RFE_ERR_INVALID;
    c->prof_filter = stage ? stage : "";
    return RFE_OK;
}
extern "C" int rfe_profile_reset(rfe_ctx* c) {
    if (!c) return RFE_ERR_INVALID;
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    c->stages.clear();
    return RFE_OK;
}
extern "C" int rfe_profile_read(rfe_ctx* c, char* names, size_t names_cap, double* ms, int64_t* calls, int cap) {
    if (!c) return RFE_ERR_INVALID;
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    std::string all;
    int k = 0;
    for (auto& st : c->stages) {
        if (k >= cap) break;
        if (k) all += ";";
        all += st.name; ms[k] = st.ms; calls[k] = st.calls; ++k;
    }
    if (names && names_cap) { strncpy(names, all.c_str(), names_cap - 1); names[names_cap - 1] = 0; }
    return k;
}
