// bow.hip -- place recognition on the device: DBoW3::Vocabulary::transform for the features of one frame, and the front of
// KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates: common-word counts and L1 scores against every stored keyframe.
// Every distance is an integer and every float64 sum is taken by ONE thread in the reference's order, so the results do not depend on
// how the work is spread over lanes.  The Makefile compiles with -ffp-contract=off and without any fast-math flag: fp64 add, subtract and
// divide are IEEE, one rounding each.
#include "rfe_internal.h"

namespace rfe {

// ---------------------------------------------------------------- the descent
// Sixteen lanes per feature, four features per wave: lane l holds bytes [16 l, 16 l + 16) of the feature in two 64-bit registers and reads
// the same 16 bytes of every child row with one 16-byte load, so the sixteen lanes read a 256-byte row as one contiguous segment (nothing is
// shared between features, so the rows go straight to registers); the popcounts meet in four xor steps inside the sixteen lanes.
constexpr int BOW_GROUP = 16;
constexpr int BOW_DESCEND_THREADS = 256;

__global__ __launch_bounds__(BOW_DESCEND_THREADS) void bow_descend_kernel(BowVocabDev V, const float* __restrict__ f32,
                                                                          const uint8_t* __restrict__ u8, int N, int nid_level,
                                                                          int32_t* __restrict__ word, int32_t* __restrict__ node,
                                                                          double* __restrict__ weight) {
    const int l = threadIdx.x & (BOW_GROUP - 1);
    const int f = blockIdx.x * (BOW_DESCEND_THREADS / BOW_GROUP) + (threadIdx.x / BOW_GROUP);
    if (f >= N) return;                                // the sixteen lanes of a feature leave together
    unsigned long long a0 = 0, a1 = 0;
    if (f32) {                                         // D == 256: byte = value > 0 (a NaN compares false)
        const float4* p = (const float4*)(f32 + (size_t)f * 256 + l * 16);
        const float4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
        a0 = (unsigned long long)(v0.x > 0.f) | (unsigned long long)(v0.y > 0.f) << 8 | (unsigned long long)(v0.z > 0.f) << 16 |
             (unsigned long long)(v0.w > 0.f) << 24 | (unsigned long long)(v1.x > 0.f) << 32 | (unsigned long long)(v1.y > 0.f) << 40 |
             (unsigned long long)(v1.z > 0.f) << 48 | (unsigned long long)(v1.w > 0.f) << 56;
        a1 = (unsigned long long)(v2.x > 0.f) | (unsigned long long)(v2.y > 0.f) << 8 | (unsigned long long)(v2.z > 0.f) << 16 |
             (unsigned long long)(v2.w > 0.f) << 24 | (unsigned long long)(v3.x > 0.f) << 32 | (unsigned long long)(v3.y > 0.f) << 40 |
             (unsigned long long)(v3.z > 0.f) << 48 | (unsigned long long)(v3.w > 0.f) << 56;
    } else {                                           // rows of D bytes, D % 8 == 0
        const unsigned long long* p = (const unsigned long long*)(u8 + (size_t)f * V.D);
        if (l * 16 < V.D) a0 = p[l * 2];
        if (l * 16 + 8 < V.D) a1 = p[l * 2 + 1];
    }
    const bool live = l * 16 < V.Dp;                   // the padded row has these sixteen bytes
    int cur = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
    for (;;) {
        const int c0 = V.child_off[cur], c1 = V.child_off[cur + 1];
        if (c0 == c1) break;
        ++level;
        int best = 0x7fffffff, best_id = cur;
        // four children at a time, their rows loaded before the first is used; past the last child the last one is read again, which
        // changes nothing: it cannot be strictly nearer than itself
        for (int c = c0; c < c1; c += 4) {
            int id[4];
            uint4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) id[u] = V.children[min(c + u, c1 - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = live ? *(const uint4*)(V.desc + (size_t)id[u] * V.Dp + l * 16) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int d = live ? __popcll(a0 ^ ((unsigned long long)r[u].x | (unsigned long long)r[u].y << 32)) +
                                   __popcll(a1 ^ ((unsigned long long)r[u].z | (unsigned long long)r[u].w << 32))
                             : 0;
                d += __shfl_xor(d, 8, BOW_GROUP); d += __shfl_xor(d, 4, BOW_GROUP);
                d += __shfl_xor(d, 2, BOW_GROUP); d += __shfl_xor(d, 1, BOW_GROUP);
                if (d < best) { best = d; best_id = id[u]; }   // strict: the first of equal children stays
            }
        }
        cur = best_id;
        if (level == nid_level) nid = cur;
    }
    if (l == 0) {
        word[f] = V.word_id[cur];
        node[f] = nid < 0 ? cur : nid;                 // a leaf above depth L - levelsup: the leaf itself
        weight[f] = V.weight[cur];
    }
}

void launch_bow_descend(hipStream_t s, const BowVocabDev& V, const float* desc_f32, const uint8_t* desc_u8, int N, int levelsup, int32_t* word,
                        int32_t* node, double* weight) {
    if (N <= 0) return;
    const int per = BOW_DESCEND_THREADS / BOW_GROUP;
    const long long lvl = (long long)V.L - levelsup;
    const int nid_level = lvl > 0x7fffffff ? 0x7fffffff : lvl < 0 ? 0 : (int)lvl;
    bow_descend_kernel<<<(N + per - 1) / per, BOW_DESCEND_THREADS, 0, s>>>(V, desc_f32, desc_u8, N, nid_level, word, node, weight);
}

// ---------------------------------------------------------------- the two sorted results
// Block 0 builds the BowVector, block 1 the FeatureVector, each from (id << 32 | feature) keys of the features that are not stopped, sorted
// by a bitonic network in LDS (the keys are distinct, so the order is the one a std::map with vectors filled in feature order has).  The
// head of every run of one id owns the run: it adds the run's weights, which lie in sorted order in LDS by then, one after the other in
// feature order, and one thread adds the words' values one after the other in word order for the L1 norm.
constexpr int BOW_BUILD_THREADS = 1024;
constexpr unsigned long long BOW_PAD = ~0ull;

__global__ __launch_bounds__(BOW_BUILD_THREADS) void bow_build_kernel(const int32_t* __restrict__ word, const int32_t* __restrict__ node,
                                                                      const double* __restrict__ weight, int N, int M /*power of two >= N*/,
                                                                      int first_only, int32_t* __restrict__ bow_n, int32_t* __restrict__ bow_word,
                                                                      double* __restrict__ bow_value, int32_t* __restrict__ fv_n,
                                                                      int32_t* __restrict__ fv_node, int32_t* __restrict__ fv_offsets,
                                                                      int32_t* __restrict__ fv_feat) {
    // 48 KiB: the keys while they are sorted; then the sorted ids (u32) in the first third and the sorted weights (f64) behind them
    __shared__ unsigned long long buf[BOW_MAX_N * 3 / 2];
    unsigned long long* key = buf;
    __shared__ int scan[BOW_BUILD_THREADS];
    __shared__ double norm_sh;
    const int t = threadIdx.x;
    const bool is_bow = blockIdx.x == 0;
    const int32_t* id_of = is_bow ? word : node;
    for (int i = t; i < M; i += BOW_BUILD_THREADS)
        key[i] = (i < N && weight[i] > 0.0) ? ((unsigned long long)(uint32_t)id_of[i] << 32 | (uint32_t)i) : BOW_PAD;
    __syncthreads();
    for (int k = 2; k <= M; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < M; i += BOW_BUILD_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = key[i], b = key[x];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[x] = a; }
                }
            }
            __syncthreads();
        }
    // thread t owns the sorted positions [t per, t per + per): it takes their keys and weights into registers, and once everybody has,
    // the ids and the weights in sorted order replace the keys, so that a run is added up from LDS
    const int per = M > BOW_BUILD_THREADS ? M / BOW_BUILD_THREADS : 1;   // <= BOW_MAX_N / BOW_BUILD_THREADS = 4
    const int p0 = t * per;
    unsigned long long mine[4];
    double wmine[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mine[r] = (r < per && p0 + r < M) ? key[p0 + r] : BOW_PAD;
        wmine[r] = mine[r] != BOW_PAD ? weight[(uint32_t)mine[r]] : 0.0;
    }
    __syncthreads();
    uint32_t* ids = (uint32_t*)buf;                    // [M]; 0xffffffff = padding (no word or node id is negative)
    double* wsorted = (double*)(buf + BOW_MAX_N / 2);  // [M]
    constexpr uint32_t NO_ID = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < per && p0 + r < M) { ids[p0 + r] = (uint32_t)(mine[r] >> 32); wsorted[p0 + r] = wmine[r]; }
    __syncthreads();
    int heads = 0;
    unsigned head_mask = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = p0 + r;
        if (r < per && i < M && mine[r] != BOW_PAD && (i == 0 || ids[i - 1] != ids[i])) { ++heads; head_mask |= 1u << r; }
    }
    scan[t] = heads;
    __syncthreads();
    for (int off = 1; off < BOW_BUILD_THREADS; off <<= 1) {
        const int v = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const int n_out = scan[BOW_BUILD_THREADS - 1];
    int o = scan[t] - heads;                           // the first output slot of this thread's heads
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = p0 + r;
        if (mine[r] == BOW_PAD) continue;
        if (!is_bow) fv_feat[i] = (int32_t)(uint32_t)mine[r];
        if (!(head_mask >> r & 1)) continue;
        const uint32_t id = ids[i];
        if (is_bow) {
            double s = wsorted[i];
            if (!first_only)
                for (int j = i + 1; j < M && ids[j] == id; ++j) s += wsorted[j];
            bow_word[o] = (int32_t)id;
            sum[r] = s;
        } else {
            fv_node[o] = (int32_t)id;
            fv_offsets[o] = i;
        }
        ++o;
    }
    if (!is_bow) {
        // the entries that are not stopped end where the padding begins
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = p0 + r;
            if (mine[r] != BOW_PAD && (i == M - 1 || ids[i + 1] == NO_ID)) fv_offsets[n_out] = i + 1;
        }
        if (t == 0) { *fv_n = n_out; if (ids[0] == NO_ID) fv_offsets[0] = 0; }
        return;
    }
    __syncthreads();                                   // every run has been read: the words' values take the weights' place
    double* val = wsorted;
    o = scan[t] - heads;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (head_mask >> r & 1) val[o++] = sum[r];
    __syncthreads();
    if (t == 0) {
        double nrm = 0.0;
        for (int i = 0; i < n_out; ++i) nrm += fabs(val[i]);
        norm_sh = nrm;
        *bow_n = n_out;
    }
    __syncthreads();
    const double nrm = norm_sh;
    for (int i = t; i < n_out; i += BOW_BUILD_THREADS) bow_value[i] = nrm > 0.0 ? val[i] / nrm : val[i];
}

void launch_bow_build(hipStream_t s, const int32_t* word, const int32_t* node, const double* weight, int N, bool first_only, int32_t* bow_n,
                      int32_t* bow_word, double* bow_value, int32_t* fv_n, int32_t* fv_node, int32_t* fv_offsets, int32_t* fv_feat) {
    int M = 2;
    while (M < N) M <<= 1;
    bow_build_kernel<<<2, BOW_BUILD_THREADS, 0, s>>>(word, node, weight, N, M, first_only ? 1 : 0, bow_n, bow_word, bow_value, fv_n, fv_node,
                                                     fv_offsets, fv_feat);
}

// ---------------------------------------------------------------- the keyframe database
__global__ void bow_db_set_entry_kernel(long long* start, int32_t* len, int e, long long at, int n) { start[e] = at; len[e] = n; }
void launch_bow_db_set_entry(hipStream_t s, long long* start, int32_t* len, int e, long long at, int n) {
    bow_db_set_entry_kernel<<<1, 1, 0, s>>>(start, len, e, at, n);
}

constexpr int BOW_DB_THREADS = 256;                    // four waves, one entry per wave at a time
constexpr int BOW_DB_MAX_BLOCKS = 1024;

// index of w in the ascending q [nq], or -1
__device__ __forceinline__ int bow_find(const int32_t* q, int nq, int32_t w) {
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < w) lo = mid + 1; else hi = mid;
    }
    return (lo < nq && q[lo] == w) ? lo : -1;
}

// the query's words go to LDS once per block; a wave walks its entries' words 64 at a time, one binary search per lane
__global__ __launch_bounds__(BOW_DB_THREADS) void bow_db_count_kernel(const int32_t* __restrict__ words, const long long* __restrict__ start,
                                                                      const int32_t* __restrict__ len, int E, const int32_t* __restrict__ q_word,
                                                                      int nq, const uint8_t* __restrict__ exclude, int32_t* __restrict__ common,
                                                                      int32_t* __restrict__ stats) {
    __shared__ int32_t q[BOW_MAX_N];
    for (int i = threadIdx.x; i < nq; i += BOW_DB_THREADS) q[i] = q_word[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, waves = gridDim.x * (BOW_DB_THREADS / 64);
    int wave_max = 0, wave_sharing = 0;
    for (int e = blockIdx.x * (BOW_DB_THREADS / 64) + (threadIdx.x >> 6); e < E; e += waves) {
        const int n = len[e];
        const int32_t* w = words + start[e];
        int cnt = 0;
        for (int i = lane; i < n; i += 64) cnt += bow_find(q, nq, w[i]) >= 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
        if (lane == 0) common[e] = cnt;
        if (cnt > 0 && !(exclude && exclude[e])) { wave_max = max(wave_max, cnt); ++wave_sharing; }
    }
    if (lane == 0 && wave_sharing > 0) { atomicMax(stats + 0, wave_max); atomicAdd(stats + 2, wave_sharing); }
}

__device__ __forceinline__ double bow_readlane(double v, int src /*wave-uniform*/) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(BOW_DB_THREADS) void bow_db_score_kernel(const int32_t* __restrict__ words, const double* __restrict__ values,
                                                                      const long long* __restrict__ start, const int32_t* __restrict__ len, int E,
                                                                      const int32_t* __restrict__ q_word, const double* __restrict__ q_value,
                                                                      int nq, const uint8_t* __restrict__ exclude,
                                                                      const int32_t* __restrict__ common, uint8_t* __restrict__ scored,
                                                                      double* __restrict__ score, int32_t* __restrict__ stats) {
    __shared__ int32_t q[BOW_MAX_N];
    for (int i = threadIdx.x; i < nq; i += BOW_DB_THREADS) q[i] = q_word[i];
    __syncthreads();
    const int min_common = (int)((float)stats[0] * 0.8f);   // int minCommonWords = maxCommonWords * 0.8f
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[1] = min_common;
    const int lane = threadIdx.x & 63, waves = gridDim.x * (BOW_DB_THREADS / 64);
    int wave_scored = 0;
    for (int e = blockIdx.x * (BOW_DB_THREADS / 64) + (threadIdx.x >> 6); e < E; e += waves) {
        const bool take = common[e] > min_common && !(exclude && exclude[e]);
        if (lane == 0) scored[e] = take ? 1 : 0;
        if (!take) continue;
        ++wave_scored;
        const int n = len[e];
        const int32_t* w = words + start[e];
        const double* wv = values + start[e];
        double sum = 0.0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const int at = i < n ? bow_find(q, nq, w[i]) : -1;
            double term = 0.0;
            if (at >= 0) {
                const double vi = q_value[at], wi = wv[i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
            unsigned long long hit = __ballot(at >= 0);
            while (hit) {                              // the terms in ascending word order, one add each
                const int src = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                sum += bow_readlane(term, src);
            }
        }
        if (lane == 0) score[e] = -sum / 2.0;
    }
    if (lane == 0 && wave_scored > 0) atomicAdd(stats + 3, wave_scored);
}

void launch_bow_db_query(hipStream_t s, const int32_t* words, const double* values, const long long* start, const int32_t* len, int n_entries,
                         const int32_t* q_word, const double* q_value, int nq, const uint8_t* exclude, int32_t* common, uint8_t* scored,
                         double* score, int32_t* stats) {
    if (n_entries <= 0) return;
    const int per = BOW_DB_THREADS / 64;
    const int blocks = std::min((n_entries + per - 1) / per, BOW_DB_MAX_BLOCKS);
    bow_db_count_kernel<<<blocks, BOW_DB_THREADS, 0, s>>>(words, start, len, n_entries, q_word, nq, exclude, common, stats);
    bow_db_score_kernel<<<blocks, BOW_DB_THREADS, 0, s>>>(words, values, start, len, n_entries, q_word, q_value, nq, exclude, common, scored, score,
                                                        stats);
}

}  // namespace rfe
