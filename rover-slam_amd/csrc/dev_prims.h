// dev_prims.h -- the device-side primitives every LightGlue tiling (and the LDS-DMA SuperPoint conv) shares, each stated once: the 16-byte
// LDS-DMA copy, the vector register types, the short-erf GELU, the online-softmax step and the XCD block decode with its grid padding.
// Include after rfe_internal.h (f32x16 / f32x4 live there); the fp16 operand split is h2_split.h.
#pragma once
#include "h2_split.h"

namespace rfe {

// ---------------------------------------------------------------- vector register types
typedef h2_f16x8 f16x8;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef h2_f16x2 f16x2;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- LDS-DMA copy
// global_load_lds_dwordx4: lane l of the wave moves 16 bytes from its own address g to lds + 16 l (the LDS side is wave-uniform and lane-linear,
// so a swizzle goes on the SOURCE address).  Counted by vmcnt; the caller places its own s_waitcnt / s_barrier.
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gptr_t;
__device__ __forceinline__ void lds_dma16(const void* g, void* lds) { __builtin_amdgcn_global_load_lds((gptr_t)g, (lds_ptr_t)lds, 16, 0, 0); }

// ---------------------------------------------------------------- GELU
// GELU(erf) with a short branch-free erf: Abramowitz-Stegun 7.1.26, |erf error| <= 1.5e-7 (libm erff: <= 1 ulp = 6e-8), about a
// third of the instructions of the library erff (ffn.3 with the fused LayerNorm + GELU: 3.30 -> 3.13 ms per step).  Over the 20-case
// tolerance study the match-score deviation from the oracle is unchanged (<= 1.9e-4, lists identical): profiles/r02_ab_notes.md.
// The one GELU of every LightGlue tiling (tests/tolerances.py).
__device__ __forceinline__ float gelu_short(float t) {
    const float x = t * 0.70710678118654752f, ax = fabsf(x);
    const float k = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    const float poly = fmaf(fmaf(fmaf(fmaf(1.061405429f, k, -1.453152027f), k, 1.421413741f), k, -0.284496736f), k, 0.254829592f) * k;
    const float er = 1.0f - poly * __builtin_amdgcn_exp2f(-(ax * ax) * 1.44269504088896341f);
    return 0.5f * t * (1.0f + copysignf(er, x));
}

// ---------------------------------------------------------------- online softmax
// Online softmax step on one 32-key x 32-query S^T block, trimmed for VALU count: on gfx950 the fp32 MFMA runs at the vector rate
// (64 FLOP / clk / SIMD) and every VALU instruction of ANY wave of the SIMD measurably costs matrix-pipe time (the softmax removed:
// +12 % with the staging gone, profiles/r01_pmc.md; LayerNorm + GELU on ffn.3's operand path: its full VALU time), so the steady
// state does as little as it can:
//   * the reference maximum is subtracted INSIDE the accumulation -- the accumulator starts at -m_run instead of 0 (softmax_init) --
//     so no subtraction per element;
//   * the tile maximum is a v_max3 tree per lane, compared against the deferred-rescale threshold WITHOUT combining the two half-waves
//     (__any covers both); only the rare branch (always the first tile) combines them, moves the reference and shifts the block;
//   * the row sum stays a per-half-wave partial; the halves are added once after the last tile (softmax_finish).
// st: in = S^T block relative to the reference, out = P^T block.  first: wave-uniform, the first tile of this wave's key range.
// DEFER_LOG2: the deferred-rescale threshold in log2 units, P <= 2^DEFER_LOG2 between two moves of the reference.  The split form
// (RFE_OPT_LG_FP16X2) needs 2^11: P = 2^(S - ref) is split into fp16 operands and must stay below fp16's 65504.
constexpr int SOFTMAX_DEFER_F32 = 16, SOFTMAX_DEFER_H2 = 11;
__device__ __forceinline__ float softmax_init(bool first, float m_run) { return first ? 0.f : -m_run; }
template <int DEFER_LOG2>
__device__ __forceinline__ void softmax_step(f32x16& st, bool first, float& m_run, float& l_run, f32x16& o0, f32x16& o1) {
    float mx = fmaxf(fmaxf(st[0], st[1]), st[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, st[r]), st[r + 1]);
    mx = fmaxf(mx, st[15]);
    if (__any(first || mx > (float)DEFER_LOG2)) {
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float ref = first ? 0.f : m_run;            // what the accumulator already subtracted
        const float m_new = fmaxf(m_run, mx + ref);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // m_run = -inf on the first tile -> 0
        const float d = ref - m_new;
        l_run *= alpha;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] += d; o0[r] *= alpha; o1[r] *= alpha; }
    }
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r]); ps += st[r]; }
    l_run += ps;
}
__device__ __forceinline__ float softmax_finish(float l_run) { return l_run + __shfl_xor(l_run, 32); }

// ---------------------------------------------------------------- XCD block decode and its grid padding
// The hardware deals the workgroups of a grid round-robin over the 8 XCDs (block b runs on XCD b & 7), each with an L2 of its own.  A kernel
// whose `ninner` blocks of one unit share data (the query blocks of a (sequence, head), the column tiles of a row panel) wants them on ONE
// XCD: block b is inner = (b >> 3) % ninner of unit = ((b >> 3) / ninner) * 8 + (b & 7), so eight units run side by side, one per XCD.
// The decode reaches the units in groups of eight, so it maps the grid one-to-one onto (unit, inner) only when the grid covers a multiple
// of 8 units: the launcher sizes the grid ninner * xcd_padded(units) and the kernel returns on unit >= units (checked below).
// xcd_decode_pow2<N>: the same decode for a compile-time power-of-two inner count, as a mask and a shift (the compiler cannot know the block
// index non-negative, so a signed division by a constant 2 would still cost its sign fix-up).
struct XcdBlock { int inner, unit; };
__host__ __device__ constexpr int xcd_padded(int units) { return (units + 7) / 8 * 8; }
__host__ __device__ constexpr XcdBlock xcd_decode(int block, int ninner) {
    const int xcd = block & 7, t_ = block >> 3;
    return {t_ % ninner, (t_ / ninner) * 8 + xcd};
}
template <int N>
__host__ __device__ constexpr XcdBlock xcd_decode_pow2(int block) {
    static_assert(N > 0 && (N & (N - 1)) == 0, "a compile-time inner count must be a power of two");
    const int xcd = block & 7, t_ = block >> 3;
    return {t_ & (N - 1), (t_ >> __builtin_ctz(N)) * 8 + xcd};
}
// every (unit < units, inner) is produced by exactly one block below ninner * xcd_padded(units), every other block decodes to unit >= units
constexpr bool xcd_decode_covers(int units, int ninner) {
    bool seen[132 * 8] = {};
    int live = 0;
    for (int b = 0; b < ninner * xcd_padded(units); ++b) {
        const XcdBlock d = xcd_decode(b, ninner);
        if (ninner == 2 && (d.inner != xcd_decode_pow2<2>(b).inner || d.unit != xcd_decode_pow2<2>(b).unit)) return false;   // the one form in use
        if (d.unit >= units) continue;
        if (d.unit < 0 || d.inner < 0 || d.inner >= ninner || seen[d.unit * ninner + d.inner]) return false;
        seen[d.unit * ninner + d.inner] = true;
        ++live;
    }
    return live == units * ninner;
}
constexpr bool xcd_decode_covers_all() {
    for (int units : {1, 4, 8, 12, 132})
        for (int ninner : {1, 2, 3, 8})
            if (!xcd_decode_covers(units, ninner)) return false;
    return true;
}
static_assert(xcd_decode_covers_all(), "xcd_decode must map ninner * xcd_padded(units) blocks one-to-one onto (unit, inner) plus padding");

}  // namespace rfe
