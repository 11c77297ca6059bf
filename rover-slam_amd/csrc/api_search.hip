// api_search.hip -- C ABI of librover_fe.so: the descriptor helpers of the callers' classic searches (L2 matrix, binarisation, candidate
// scan, SearchByProjection1, the Sim3 SearchByProjection overloads, SearchLocalPoints, distinctive descriptors).
#include <string.h>
#include <algorithm>
#include <type_traits>
#include "api_internal.h"

using namespace rfe;

// =====================================================================================
// descriptor helpers of the callers' classic searches.  The "_dev" forms take device pointers and are
// asynchronous on the ctx stream (descriptors usually ARE device resident: they come out of rfe_extract_u8_dev /
// rfe_stereo_frame_dev); the host-pointer forms validate, stage through ws_io and call them.
// =====================================================================================
// Every pair below: one argument check for both forms (it passes an empty problem without a look at the pointers, which are the caller's,
// whichever side they live on); the host form adds the checks only it can make, stages its arrays and calls the device form.
static int l2_check(rfe_ctx* c, const void* a, int M, const void* b, int N, const void* out) {
    if (!c) return RFE_ERR_INVALID;
    if (M < 0 || N < 0 || (M > 0 && N > 0 && (!a || !b || !out))) return fail(c, RFE_ERR_INVALID, "l2_distance_matrix: bad argument");
    return RFE_OK;
}
extern "C" int rfe_l2_distance_matrix_dev(rfe_ctx* c, const float* a, int M, const float* b, int N, float* out) {
    int rc = l2_check(c, a, M, b, N, out);
    if (rc || M == 0 || N == 0) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    { ProfScope ps(c, "l2_matrix"); launch_l2_matrix(c->stream, a, M, b, N, out); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}
extern "C" int rfe_l2_distance_matrix(rfe_ctx* c, const float* a, int M, const float* b, int N, float* out) {
    int rc = l2_check(c, a, M, b, N, out);
    if (rc || M == 0 || N == 0) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    float *da, *db, *dout;
    HostIo io(c, HostIo::DIRECT);
    io.in(da, a, (size_t)M * 256); io.in(db, b, (size_t)N * 256);
    io.out(dout, out, (size_t)M * N);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_l2_distance_matrix_dev(c, da, M, db, N, dout))) return rc;
    return io.download();
}

static int binarize_check(rfe_ctx* c, const void* desc, int rows, const void* out) {
    if (!c) return RFE_ERR_INVALID;
    if (rows < 0 || (rows > 0 && (!desc || !out))) return fail(c, RFE_ERR_INVALID, "binarize_descriptors: bad argument");
    return RFE_OK;
}
extern "C" int rfe_binarize_descriptors_dev(rfe_ctx* c, const float* desc, int rows, uint8_t* out) {
    int rc = binarize_check(c, desc, rows, out);
    if (rc || rows == 0) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    launch_binarize(c->stream, desc, rows, out);
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}
extern "C" int rfe_binarize_descriptors(rfe_ctx* c, const float* desc, int rows, uint8_t* out) {
    int rc = binarize_check(c, desc, rows, out);
    if (rc || rows == 0) return rc;
    RFE_HIP(c, hipSetDevice(c->device));
    float* dd; uint8_t* dout;
    HostIo io(c, HostIo::DIRECT);
    io.in(dd, desc, (size_t)rows * 256);
    io.out(dout, out, (size_t)rows * 256);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_binarize_descriptors_dev(c, dd, rows, dout))) return rc;
    return io.download();
}

// best / second-best scan of SPmatcher::SearchByProjection1 (src/Matchers/SPmatcher.cc:1218-1248) over device-resident CSR
// candidate lists.  The lists cannot be validated from the host without a synchronisation: the kernel ignores candidate
// indices outside [0, Nf); offsets must be non-decreasing with offsets[0] = 0 (the caller's contract, as for the host form).
static int sc_check(rfe_ctx* c, const void* q, int Nq, int Nf, const void* offsets, const void* best_idx, const void* best_dist, const void* second_dist) {
    if (!c) return RFE_ERR_INVALID;
    if (Nq < 0 || Nf < 0) return fail(c, RFE_ERR_INVALID, "search_candidates: negative count");
    if (Nq == 0) return RFE_OK;
    if (!q || !offsets || !best_idx || !best_dist || !second_dist) return fail(c, RFE_ERR_INVALID, "search_candidates: null pointer");
    return RFE_OK;
}
extern "C" int rfe_search_candidates_dev(rfe_ctx* c, const float* q, int Nq, const float* f, int Nf, const int32_t* offsets,
                                         const int32_t* cand, const uint8_t* skip, int32_t* best_idx, float* best_dist,
                                         float* second_dist) {
    int rc = sc_check(c, q, Nq, Nf, offsets, best_idx, best_dist, second_dist);
    if (rc || Nq == 0) return rc;
    if (Nf > 0 && (!f || !cand)) return fail(c, RFE_ERR_INVALID, "search_candidates: null pointer");
    RFE_HIP(c, hipSetDevice(c->device));
    { ProfScope ps(c, "search_candidates");
      launch_search_candidates(c->stream, q, Nq, f, Nf, offsets, cand, skip, best_idx, best_dist, second_dist); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_search_candidates(rfe_ctx* c, const float* q, int Nq, const float* f, int Nf, const int32_t* offsets,
                                     const int32_t* cand, const uint8_t* skip, int32_t* best_idx, float* best_dist,
                                     float* second_dist) {
    int rc = sc_check(c, q, Nq, Nf, offsets, best_idx, best_dist, second_dist);
    if (rc || Nq == 0) return rc;
    if (offsets[0] != 0) return fail(c, RFE_ERR_INVALID, "search_candidates: offsets[0] must be 0");
    for (int i = 0; i < Nq; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, RFE_ERR_INVALID, "search_candidates: offsets must be non-decreasing");
    const int nnz = offsets[Nq];
    if (nnz > 0 && (!cand || !f)) return fail(c, RFE_ERR_INVALID, "search_candidates: null candidate list");
    for (int k = 0; k < nnz; ++k)
        if (cand[k] < 0 || cand[k] >= Nf) return fail(c, RFE_ERR_INVALID, "search_candidates: candidate index out of range");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dq, *df, *dbd, *dsd; int32_t *doff, *dc, *dbi; uint8_t* dsk;
    HostIo io(c, HostIo::DIRECT);
    io.in(dq, q, (size_t)Nq * 256); io.in(df, f, f ? (size_t)Nf * 256 : 0); io.in(doff, offsets, (size_t)Nq + 1); io.in(dc, cand, nnz);
    io.in_opt(dsk, skip, Nf);
    io.out(dbi, best_idx, Nq); io.out(dbd, best_dist, Nq); io.out(dsd, second_dist, Nq);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_search_candidates_dev(c, dq, Nq, df, Nf, doff, dc, dsk, dbi, dbd, dsd))) return rc;
    return io.download();
}

// =====================================================================================
// The projection searches: SearchByProjection1, the Sim3 SearchByProjection overloads (6e), SearchLocalPoints (6f).  Behind
// its front each of them is the same search, written once here (6d, "The back end"): ps_check holds the shape rules, ps_run the workspace,
// the front and the grid -> count -> fill -> resolve sequence of the device forms, ps_sized the slot sizing of the host forms.  An entry is
// its own checks, its own staging and one call into these.
// =====================================================================================
// ws_ps: the grid (cell starts, items, positions), the segment offsets and cand_cap (index, distance) slots -- one element at least of each
struct PsBuffers { int32_t *cell_start, *cell_items, *seg_off, *cand_idx; float *fxy, *cand_dist; };
static void ps_layout(Bump& a, int Nq, int Nf, int cand_cap, PsBuffers& b) {
    const size_t nf1 = (size_t)std::max(Nf, 1), cap1 = (size_t)std::max(cand_cap, 1);
    b.cell_start = a.take<int32_t>(770); b.cell_items = a.take<int32_t>(nf1); b.fxy = a.take<float>(nf1 * 2);
    b.seg_off = a.take<int32_t>((size_t)Nq + 1); b.cand_idx = a.take<int32_t>(cap1); b.cand_dist = a.take<float>(cap1);
}

// The shape rules of every projection search, in the order the refusals are tested: `count` is what the entry calls its map-point count
// (Nq or Np), `own` the entry's rules that come between the bounds and cand_cap, `null_required` whether a required pointer is null.
template <typename Own>
static int ps_check(rfe_ctx* c, const char* entry, const char* count, int Nq, int Nf, float min_x, float min_y, float max_x, float max_y,
                    int cand_cap, const void* kpts, const void* kxy, bool null_required, Own&& own) {
    const auto refuse = [&](const std::string& what) { return fail(c, RFE_ERR_INVALID, std::string(entry) + ": " + what); };
    if (Nq < 0 || Nq > 16384) return refuse(std::string(count) + " outside 0..16384");
    if (Nf < 0 || Nf > 4096) return refuse("Nf outside 0..4096");
    if (!(max_x > min_x) || !(max_y > min_y)) return refuse("empty image bounds");
    if (int rc = own()) return rc;
    if (cand_cap < 0) return refuse("negative cand_cap");
    if ((kpts != nullptr) == (kxy != nullptr)) return refuse("pass exactly one of kpts and kxy");
    if (null_required) return refuse("null pointer");
    return RFE_OK;
}
// the pyramid rules that the entries with a PredictScale front share
static int ps_check_levels(rfe_ctx* c, const char* entry, int nlevels, float log_scale_factor) {
    if (nlevels < 1 || nlevels > RFE_MAX_LEVELS) return fail(c, RFE_ERR_INVALID, std::string(entry) + ": nlevels outside 1..16");
    if (nlevels > 1 && !(log_scale_factor > 0.f)) return fail(c, RFE_ERR_INVALID, std::string(entry) + ": log_scale_factor must be positive");
    return RFE_OK;
}

// One search, device resident.  Without a front proj / radius / pred_level are the caller's; with one they are ignored, the front writes
// them into ws_ps and proj_out / radius_out / level_out (each may be null) receive copies; level_gate: proj_count reads the front's level.
struct PsProblem {
    const float* q; int Nq;                                                            // map points: descriptors
    const float* proj; const float* radius; const int32_t* pred_level; const uint8_t* observed;
    const float* f; const float* kpts; const int32_t* kxy; const int32_t* octave; const uint8_t* skip; int Nf; const int32_t* nf_dev;   // features
    float min_x, min_y, max_x, max_y;
    float th; bool trunc; int cand_cap;                                                // acceptance threshold, truncated distances (6e), slots
    int32_t *assign, *best_idx; float *best_dist, *second_dist; int32_t* stats;
    bool level_gate; float *proj_out, *radius_out; int32_t* level_out;
};
// Front: nullptr, or a callable (wproj, wradius, wlevel) that launches the front kernel, which runs under the profile stage `front_stage`.
// Workspace: ps_layout, then behind it the front's proj [Nq,2], radius [Nq], level [Nq].  Four or five kernels on the ctx stream, nothing
// read back.
template <typename Front>
static int ps_run(rfe_ctx* c, const PsProblem& p, const char* front_stage, Front&& front) {
    constexpr bool has_front = !std::is_same<typename std::decay<Front>::type, std::nullptr_t>::value;
    RFE_HIP(c, hipSetDevice(c->device));
    PsBuffers b; float *wproj = nullptr, *wradius = nullptr; int32_t* wlevel = nullptr;
    int rc = ws_carve(c, &c->ws_ps, &c->ws_ps_bytes, [&](Bump& a) {
        ps_layout(a, p.Nq, p.Nf, p.cand_cap, b);
        if (has_front) {
            const size_t np1 = (size_t)std::max(p.Nq, 1);
            wproj = a.take<float>(np1 * 2); wradius = a.take<float>(np1); wlevel = a.take<int32_t>(np1);
        }
    });
    if (rc) return rc;
    const float inv_w = 32.f / (p.max_x - p.min_x), inv_h = 24.f / (p.max_y - p.min_y);   // mfGridElementWidthInv / HeightInv of the Frame or KeyFrame
    const float *proj = p.proj, *radius = p.radius; const int32_t* pred_level = p.pred_level;
    hipStream_t s = c->stream;
    if constexpr (has_front) {
        RFE_HIP(c, hipMemsetAsync(p.stats + 4, 0, 16, s));
        { ProfScope ps(c, front_stage); front(wproj, wradius, wlevel); }
        proj = wproj; radius = wradius; pred_level = p.level_gate ? wlevel : nullptr;
    }
    { ProfScope ps(c, "ps_grid");
      launch_proj_grid(s, p.kpts, p.kxy, p.Nf, p.nf_dev, p.min_x, p.min_y, inv_w, inv_h, b.cell_start, b.cell_items, b.fxy); }
    { ProfScope ps(c, "ps_count");
      launch_proj_count(s, proj, radius, pred_level, p.Nq, b.cell_start, b.cell_items, b.fxy, p.octave, p.min_x, p.min_y, inv_w, inv_h, p.cand_cap,
                        b.seg_off, b.cand_idx, p.stats); }
    { ProfScope ps(c, "ps_fill");
      if (p.trunc) launch_proj_fill_trunc(s, p.q, p.Nq, p.f, p.Nf, b.seg_off, b.cand_idx, p.skip, b.cand_dist);
      else launch_proj_fill(s, p.q, p.Nq, p.f, p.Nf, b.seg_off, b.cand_idx, p.skip, b.cand_dist); }
    { ProfScope ps(c, "ps_resolve");
      launch_proj_resolve(s, b.seg_off, b.cand_idx, b.cand_dist, p.observed, p.Nq, p.Nf, p.th, p.assign, p.best_idx, p.best_dist, p.second_dist,
                          p.stats); }
    if (has_front && p.Nq > 0) {
        if (p.proj_out) RFE_HIP(c, hipMemcpyAsync(p.proj_out, wproj, (size_t)p.Nq * 8, hipMemcpyDeviceToDevice, s));
        if (p.radius_out) RFE_HIP(c, hipMemcpyAsync(p.radius_out, wradius, (size_t)p.Nq * 4, hipMemcpyDeviceToDevice, s));
        if (p.level_out) RFE_HIP(c, hipMemcpyAsync(p.level_out, wlevel, (size_t)p.Nq * 4, hipMemcpyDeviceToDevice, s));
    }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

// Slot sizing of the host forms.  The candidate total is known on the device only: `run(cap)` (the entry's device form on the staged arrays,
// stats at dst) goes with the largest slot count used so far (at least 16 per map point) and, when the lists need more, once again with
// exactly what they need.  Then the download, the n_stats ints for the caller, and the number of matches.
template <typename Run>
static int ps_sized(rfe_ctx* c, const char* entry, int Nq, int Nf, HostIo& io, const int32_t* dst, int n_stats, int32_t* stats, Run&& run) {
    int32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc, cap = (int)std::min<long long>(std::max<long long>(c->ps_cap, 16LL * std::max(Nq, 1)), (long long)Nq * Nf);
    for (int attempt = 0; attempt < 2; ++attempt) {
        if ((rc = run(cap))) return rc;
        RFE_HIP(c, hipMemcpyAsync(st, dst, (size_t)n_stats * 4, hipMemcpyDeviceToHost, c->stream));
        RFE_HIP(c, hipStreamSynchronize(c->stream));
        if (!st[3]) break;
        cap = st[1];
    }
    if (st[3]) return fail(c, RFE_ERR_HIP, std::string(entry) + ": candidate lists still overflow");
    c->ps_cap = std::max(c->ps_cap, cap);
    if ((rc = io.download())) return rc;
    if (stats) memcpy(stats, st, (size_t)n_stats * 4);
    return st[0];
}

// SPmatcher::SearchByProjection1, left-camera branch (src/Matchers/SPmatcher.cc:1190-1283): no front, the caller projects.
static int sbp_check(rfe_ctx* c, const void* q, const void* proj, const void* radius, int Nq, const void* f, const void* kpts, const void* kxy,
                    int Nf, float min_x, float min_y, float max_x, float max_y, int cand_cap, const void* assign) {
    return ps_check(c, "search_by_projection", "Nq", Nq, Nf, min_x, min_y, max_x, max_y, cand_cap, kpts, kxy,
                    (Nq > 0 && (!q || !proj || !radius)) || (Nf > 0 && (!f || !assign)), [] { return RFE_OK; });
}

extern "C" int rfe_search_by_projection_dev(rfe_ctx* c, const float* q, const float* proj, const float* radius, const int32_t* pred_level,
                                            const uint8_t* observed, int Nq, const float* f, const float* kpts, const int32_t* kxy,
                                            const int32_t* octave, const uint8_t* skip, int Nf, const int32_t* nf_dev, float min_x,
                                            float min_y, float max_x, float max_y, float th_high, int cand_cap, int32_t* assign,
                                            int32_t* best_idx, float* best_dist, float* second_dist, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = sbp_check(c, q, proj, radius, Nq, f, kpts, kxy, Nf, min_x, min_y, max_x, max_y, cand_cap, assign);
    if (rc) return rc;
    if (!stats) return fail(c, RFE_ERR_INVALID, "search_by_projection: null pointer");
    return ps_run(c, PsProblem{q, Nq, proj, radius, pred_level, observed, f, kpts, kxy, octave, skip, Nf, nf_dev, min_x, min_y, max_x, max_y,
                               th_high, false, cand_cap, assign, best_idx, best_dist, second_dist, stats, false, nullptr, nullptr, nullptr},
                  nullptr, nullptr);
}

extern "C" int rfe_search_by_projection(rfe_ctx* c, const float* q, const float* proj, const float* radius, const int32_t* pred_level,
                                        const uint8_t* observed, int Nq, const float* f, const float* kpts, const int32_t* kxy,
                                        const int32_t* octave, const uint8_t* skip, int Nf, float min_x, float min_y, float max_x,
                                        float max_y, float th_high, int32_t* assign, int32_t* best_idx, float* best_dist,
                                        float* second_dist, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = sbp_check(c, q, proj, radius, Nq, f, kpts, kxy, Nf, min_x, min_y, max_x, max_y, 0, assign);
    if (rc) return rc;
    if (!finite({min_x, min_y, max_x, max_y, th_high})) return fail(c, RFE_ERR_INVALID, "search_by_projection: non-finite argument");
    for (int i = 0; i < Nq; ++i) {
        if (!finite(proj + 2 * i, 2) || !finite(radius[i])) return fail(c, RFE_ERR_INVALID, "search_by_projection: non-finite projection or radius");
        if (pred_level && (pred_level[i] < 0 || pred_level[i] >= RFE_MAX_LEVELS)) return fail(c, RFE_ERR_INVALID, "search_by_projection: pred_level outside 0..15");
    }
    if (kpts && !finite(kpts, 2 * (size_t)Nf)) return fail(c, RFE_ERR_INVALID, "search_by_projection: non-finite keypoint");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dq, *dproj, *drad, *df, *dbd, *dsd; int32_t *dlev, *doct, *dasg, *dbi, *dst; uint8_t *dobs, *dsk; float* dkp; int32_t* dkx;
    HostIo io(c, HostIo::DIRECT);
    io.in(dq, q, (size_t)Nq * 256); io.in(dproj, proj, (size_t)Nq * 2); io.in(drad, radius, Nq); io.in_opt(dlev, pred_level, Nq); io.in_opt(dobs, observed, Nq);
    io.in(df, f, (size_t)Nf * 256); io.in_opt(dkp, kpts, (size_t)Nf * 2); io.in_opt(dkx, kxy, (size_t)Nf * 2); io.in_opt(doct, octave, Nf); io.in_opt(dsk, skip, Nf);
    io.out(dasg, assign, Nf); io.out(dbi, best_idx, Nq); io.out(dbd, best_dist, Nq); io.out(dsd, second_dist, Nq); io.scratch(dst, 4);
    if ((rc = io.upload())) return rc;
    return ps_sized(c, "search_by_projection", Nq, Nf, io, dst, 4, stats, [&](int cap) {
        return rfe_search_by_projection_dev(c, dq, dproj, drad, dlev, dobs, Nq, df, dkp, dkx, doct, dsk, Nf, nullptr, min_x, min_y, max_x, max_y, th_high,
                                            cap, dasg, dbi, dbd, dsd, dst);
    });
}

// The Sim3 SearchByProjection overloads of loop closing (src/Matchers/SPmatcher.cc:1558-1669, 2076-2182): the front is
// sim3_project_kernel (proj_sim3.hip); the search runs with no octave gate and every map point observed.
static int s3_check(rfe_ctx* c, const rfe_sim3_params* P, const void* q, const void* pw, const void* normal, const void* min_dist,
                    const void* max_dist, const void* scale_dist, int Np, const void* f, const void* kpts, const void* kxy, int Nf, int cand_cap,
                    const void* matched) {
    const char* entry = "search_by_projection_sim3";
    if (!P) return fail(c, RFE_ERR_INVALID, "search_by_projection_sim3: null pointer");
    return ps_check(c, entry, "Np", Np, Nf, P->min_x, P->min_y, P->max_x, P->max_y, cand_cap, kpts, kxy,
                    (Np > 0 && (!q || !pw || !normal || !min_dist || !max_dist || !scale_dist)) || (Nf > 0 && (!f || !matched)), [&] {
        if (int rc = ps_check_levels(c, entry, P->nlevels, P->log_scale_factor)) return rc;
        if (P->proj_mode != RFE_PROJ_INVZ && P->proj_mode != RFE_PROJ_DIV) return fail(c, RFE_ERR_INVALID, "search_by_projection_sim3: unknown proj_mode");
        if (P->dist_mode != RFE_DIST_FLOAT && P->dist_mode != RFE_DIST_TRUNC) return fail(c, RFE_ERR_INVALID, "search_by_projection_sim3: unknown dist_mode");
        return (int)RFE_OK;
    });
}

extern "C" int rfe_search_by_projection_sim3_dev(rfe_ctx* c, const rfe_sim3_params* P, const float* q, const float* pw, const float* normal,
                                                 const float* min_dist, const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np,
                                                 const float* f,
                                                 const float* kpts, const int32_t* kxy, const uint8_t* matched_in, int Nf,
                                                 const int32_t* nf_dev, float th_accept, int cand_cap, int32_t* matched, int32_t* best_idx,
                                                 float* best_dist, float* second_dist, float* proj, float* radius, int32_t* level,
                                                 int32_t* reject, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = s3_check(c, P, q, pw, normal, min_dist, max_dist, scale_dist, Np, f, kpts, kxy, Nf, cand_cap, matched);
    if (rc) return rc;
    if (!stats) return fail(c, RFE_ERR_INVALID, "search_by_projection_sim3: null pointer");
    return ps_run(c, PsProblem{q, Np, nullptr, nullptr, nullptr, nullptr, f, kpts, kxy, nullptr, matched_in, Nf, nf_dev, P->min_x, P->min_y, P->max_x,
                               P->max_y, th_accept, P->dist_mode == RFE_DIST_TRUNC, cand_cap, matched, best_idx, best_dist, second_dist, stats, false,
                               proj, radius, level},
                  "s3_project", [&](float* wproj, float* wradius, int32_t* wlevel) {
        launch_sim3_project(c->stream, *P, pw, normal, min_dist, max_dist, scale_dist, valid, Np, wproj, wradius, wlevel, reject, stats);
    });
}

extern "C" int rfe_search_by_projection_sim3(rfe_ctx* c, const rfe_sim3_params* P, const float* q, const float* pw, const float* normal,
                                             const float* min_dist, const float* max_dist, const float* scale_dist, const uint8_t* valid, int Np,
                                                 const float* f,
                                             const float* kpts, const int32_t* kxy, const uint8_t* matched_in, int Nf, float th_accept,
                                             int32_t* matched, int32_t* best_idx, float* best_dist, float* second_dist, float* proj,
                                             float* radius, int32_t* level, int32_t* reject, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = s3_check(c, P, q, pw, normal, min_dist, max_dist, scale_dist, Np, f, kpts, kxy, Nf, 0, matched);
    if (rc) return rc;
    if (!(finite({th_accept, P->log_scale_factor, P->fx, P->fy, P->cx, P->cy, P->min_x, P->min_y, P->max_x, P->max_y}) && finite(P->quat) &&
          finite(P->t) && finite(P->ow) && finite(P->scale_factors, P->nlevels)))
        return fail(c, RFE_ERR_INVALID, "search_by_projection_sim3: non-finite argument");
    if (kpts && !finite(kpts, 2 * (size_t)Nf)) return fail(c, RFE_ERR_INVALID, "search_by_projection_sim3: non-finite keypoint");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dq, *dpw, *dn, *dmin, *dmax, *dsc, *df, *dkp, *dbd, *dsd, *dproj, *drad; int32_t *dkx, *dm, *dbi, *dlev, *drej, *dst; uint8_t *dval, *dmi;
    HostIo io(c, HostIo::DIRECT);
    io.in(dq, q, (size_t)Np * 256); io.in(dpw, pw, (size_t)Np * 3); io.in(dn, normal, (size_t)Np * 3); io.in(dmin, min_dist, Np);
    io.in(dmax, max_dist, Np); io.in(dsc, scale_dist, Np); io.in_opt(dval, valid, Np);
    io.in(df, f, (size_t)Nf * 256); io.in_opt(dkp, kpts, (size_t)Nf * 2); io.in_opt(dkx, kxy, (size_t)Nf * 2); io.in_opt(dmi, matched_in, Nf);
    io.out(dm, matched, Nf); io.out_opt(dbi, best_idx, Np); io.out_opt(dbd, best_dist, Np); io.out_opt(dsd, second_dist, Np);
    io.out_opt(dproj, proj, (size_t)Np * 2); io.out_opt(drad, radius, Np); io.out_opt(dlev, level, Np); io.out_opt(drej, reject, Np);
    io.scratch(dst, 8);
    if ((rc = io.upload())) return rc;
    return ps_sized(c, "search_by_projection_sim3", Np, Nf, io, dst, 8, stats, [&](int cap) {
        return rfe_search_by_projection_sim3_dev(c, P, dq, dpw, dn, dmin, dmax, dsc, dval, Np, df, dkp, dkx, dmi, Nf, nullptr, th_accept, cap, dm, dbi, dbd,
                                                 dsd, dproj, drad, dlev, drej, dst);
    });
}

// Steps 2 and 3 of Tracking::SearchLocalPoints (src/Tracking.cc:4124-4180): the front is frustum_project_kernel
// (proj_frustum.hip), which also writes what else isInFrustum leaves in a map point straight into the caller's arrays; the search runs on
// its proj / radius / level as they are.
static int lp_check(rfe_ctx* c, const rfe_frustum_params* P, const void* q, const void* pw, const void* normal, const void* min_dist,
                    const void* max_dist, const void* scale_dist, int Np, const void* f, const void* kpts, const void* kxy, int Nf, int cand_cap,
                    const void* assign) {
    const char* entry = "search_local_points";
    if (!P) return fail(c, RFE_ERR_INVALID, "search_local_points: null pointer");
    return ps_check(c, entry, "Np", Np, Nf, P->min_x, P->min_y, P->max_x, P->max_y, cand_cap, kpts, kxy,
                    (Np > 0 && (!q || !pw || !normal || !min_dist || !max_dist || !scale_dist)) || (Nf > 0 && (!f || !assign)), [&] {
        if (int rc = ps_check_levels(c, entry, P->nlevels, P->log_scale_factor)) return rc;
        if (P->level_mode != RFE_LEVEL_ZERO && P->level_mode != RFE_LEVEL_PREDICTED) return fail(c, RFE_ERR_INVALID, "search_local_points: unknown level_mode");
        return (int)RFE_OK;
    });
}

extern "C" int rfe_search_local_points_dev(rfe_ctx* c, const rfe_frustum_params* P, const float* q, const float* pw, const float* normal,
                                           const float* min_dist, const float* max_dist, const float* scale_dist, const uint8_t* valid,
                                           const uint8_t* observed, int Np, const float* f, const float* kpts, const int32_t* kxy,
                                           const int32_t* octave, const uint8_t* skip, int Nf, const int32_t* nf_dev, float th_high, int cand_cap,
                                           int32_t* assign, int32_t* best_idx, float* best_dist, float* second_dist, float* proj, float* proj_xr,
                                           float* depth, float* view_cos, int32_t* level, int32_t* reject, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = lp_check(c, P, q, pw, normal, min_dist, max_dist, scale_dist, Np, f, kpts, kxy, Nf, cand_cap, assign);
    if (rc) return rc;
    if (!stats) return fail(c, RFE_ERR_INVALID, "search_local_points: null pointer");
    // level_gate: a rejected point has level -1 and radius 0, an empty list either way
    return ps_run(c, PsProblem{q, Np, nullptr, nullptr, nullptr, observed, f, kpts, kxy, octave, skip, Nf, nf_dev, P->min_x, P->min_y, P->max_x,
                               P->max_y, th_high, false, cand_cap, assign, best_idx, best_dist, second_dist, stats,
                               P->level_mode == RFE_LEVEL_PREDICTED, proj, nullptr, level},
                  "lp_frustum", [&](float* wproj, float* wradius, int32_t* wlevel) {
        launch_frustum_project(c->stream, *P, pw, normal, min_dist, max_dist, scale_dist, valid, Np, wproj, wradius, wlevel, proj_xr, depth, view_cos,
                               reject, stats);
    });
}

extern "C" int rfe_search_local_points(rfe_ctx* c, const rfe_frustum_params* P, const float* q, const float* pw, const float* normal,
                                       const float* min_dist, const float* max_dist, const float* scale_dist, const uint8_t* valid,
                                       const uint8_t* observed, int Np, const float* f, const float* kpts, const int32_t* kxy,
                                       const int32_t* octave, const uint8_t* skip, int Nf, float th_high, int32_t* assign, int32_t* best_idx,
                                       float* best_dist, float* second_dist, float* proj, float* proj_xr, float* depth, float* view_cos,
                                       int32_t* level, int32_t* reject, int32_t* stats) {
    if (!c) return RFE_ERR_INVALID;
    int rc = lp_check(c, P, q, pw, normal, min_dist, max_dist, scale_dist, Np, f, kpts, kxy, Nf, 0, assign);
    if (rc) return rc;
    if (!(finite({th_high, P->log_scale_factor, P->th, P->view_cos_limit, P->fx, P->fy, P->cx, P->cy, P->mbf, P->min_x, P->min_y, P->max_x, P->max_y}) &&
          (!P->far_points || finite(P->th_far)) && finite(P->rcw) && finite(P->tcw) && finite(P->ow) && finite(P->scale_factors, P->nlevels)))
        return fail(c, RFE_ERR_INVALID, "search_local_points: non-finite argument");
    if (kpts && !finite(kpts, 2 * (size_t)Nf)) return fail(c, RFE_ERR_INVALID, "search_local_points: non-finite keypoint");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dq, *dpw, *dn, *dmin, *dmax, *dsc, *df, *dkp, *dbd, *dsd, *dproj, *dxr, *ddep, *dvc; int32_t *dkx, *doct, *dasg, *dbi, *dlev, *drej, *dst;
    uint8_t *dval, *dobs, *dsk;
    HostIo io(c, HostIo::DIRECT);
    io.in(dq, q, (size_t)Np * 256); io.in(dpw, pw, (size_t)Np * 3); io.in(dn, normal, (size_t)Np * 3); io.in(dmin, min_dist, Np);
    io.in(dmax, max_dist, Np); io.in(dsc, scale_dist, Np); io.in_opt(dval, valid, Np); io.in_opt(dobs, observed, Np);
    io.in(df, f, (size_t)Nf * 256); io.in_opt(dkp, kpts, (size_t)Nf * 2); io.in_opt(dkx, kxy, (size_t)Nf * 2); io.in_opt(doct, octave, Nf);
    io.in_opt(dsk, skip, Nf);
    io.out(dasg, assign, Nf); io.out_opt(dbi, best_idx, Np); io.out_opt(dbd, best_dist, Np); io.out_opt(dsd, second_dist, Np);
    io.out_opt(dproj, proj, (size_t)Np * 2); io.out_opt(dxr, proj_xr, Np); io.out_opt(ddep, depth, Np); io.out_opt(dvc, view_cos, Np);
    io.out_opt(dlev, level, Np); io.out_opt(drej, reject, Np);
    io.scratch(dst, 8);
    if ((rc = io.upload())) return rc;
    return ps_sized(c, "search_local_points", Np, Nf, io, dst, 8, stats, [&](int cap) {
        return rfe_search_local_points_dev(c, P, dq, dpw, dn, dmin, dmax, dsc, dval, dobs, Np, df, dkp, dkx, doct, dsk, Nf, nullptr, th_high, cap, dasg, dbi,
                                           dbd, dsd, dproj, dxr, ddep, dvc, dlev, drej, dst);
    });
}

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438-530) for Np map points whose observed descriptors and CSR
// offsets live on the device.  `total` >= offsets[Np] (the number of descriptors, grid size) and `maxn` >= the largest
// observation count (LDS row, <= 8192) come from the caller, who built the lists; a point with more observations than maxn
// rounded up to a power of two is reported as best = -2 instead of computed.
static int dd_check(rfe_ctx* c, const void* offsets, int Np, const void* best, const void* median) {
    if (Np < 0) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: negative count");
    if (Np == 0) return RFE_OK;
    if (!offsets || !best || !median) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: null pointer");
    return RFE_OK;
}
extern "C" int rfe_distinctive_descriptors_dev(rfe_ctx* c, const float* desc, const int32_t* offsets, int Np, int total, int maxn,
                                               int32_t* best, float* median) {
    if (!c) return RFE_ERR_INVALID;
    if (total < 0 || maxn < 0) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: negative count");
    int rc = dd_check(c, offsets, Np, best, median);
    if (rc || Np == 0) return rc;
    if (total > 0 && !desc) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: null pointer");
    if (maxn > 8192) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: more than 8192 observations of one map point");
    RFE_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure_ws(c, &c->ws_tmp, &c->ws_tmp_bytes, al((size_t)std::max(total, 1) * 4)))) return rc;   // per-descriptor medians
    { ProfScope ps(c, "distinctive");
      launch_distinctive(c->stream, desc, offsets, total, Np, std::max(maxn, 1), (float*)c->ws_tmp, best, median); }
    RFE_HIP(c, hipGetLastError());
    return RFE_OK;
}

extern "C" int rfe_distinctive_descriptors(rfe_ctx* c, const float* desc, const int32_t* offsets, int Np, int32_t* best,
                                           float* median) {
    if (!c) return RFE_ERR_INVALID;
    int rc = dd_check(c, offsets, Np, best, median);
    if (rc || Np == 0) return rc;
    if (offsets[0] != 0) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: offsets[0] must be 0");
    int maxn = 0;
    for (int p = 0; p < Np; ++p) {
        const int n = offsets[p + 1] - offsets[p];
        if (n < 0) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: offsets must be non-decreasing");
        maxn = std::max(maxn, n);
    }
    if (maxn > 8192) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: more than 8192 observations of one map point");
    const int total = offsets[Np];
    if (total > 0 && !desc) return fail(c, RFE_ERR_INVALID, "distinctive_descriptors: null descriptors");
    RFE_HIP(c, hipSetDevice(c->device));
    float *dd, *dmedian; int32_t *doff, *dbest;
    HostIo io(c, HostIo::DIRECT);
    io.in(dd, desc, (size_t)total * 256); io.in(doff, offsets, (size_t)Np + 1);
    io.out(dbest, best, Np); io.out(dmedian, median, Np);
    if ((rc = io.upload())) return rc;
    if ((rc = rfe_distinctive_descriptors_dev(c, dd, doff, Np, total, maxn, dbest, dmedian))) return rc;
    return io.download();
}
