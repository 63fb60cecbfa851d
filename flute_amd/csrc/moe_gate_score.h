// The score stage of the gating, shared by its forward (moe_gate.hip: gate_token), its backward (router_grad.hip:
// moe_gate_grad_kernel) and the router's auxiliary losses (moe_aux.hip): the logit types, the exchange steps of a wave reduction,
// gate_scores, the device function that turns one token's logits into the scores of its experts, and gate_score_sums, which returns
// the max and the sums gate_scores keeps to itself.  One wave = one token; lane l holds experts l, l + 64, ... in registers.
// A wave reduction is six exchange steps without LDS: DPP quad_perm (lanes ^ 1, ^ 2), row_half_mirror, row_mirror inside a row
// of 16, then v_permlane16_swap and v_permlane32_swap across rows.  Every step combines the same two values in both partners, so
// all 64 lanes hold the same bits afterwards and the order of the additions is fixed.
#pragma once
#include "common.h"
#include "../../include/flute_amd.h"

#include <math.h>

namespace flute_amd {

template <typename L> struct GateLogit;
template <> struct GateLogit<F16> {
    typedef uint16_t type;
    static __device__ __forceinline__ float to_float(uint16_t u) { return Num<F16>::to_float(u); }
    static __device__ __forceinline__ uint16_t from_float(float f) { return Num<F16>::from_float(f); }
};
template <> struct GateLogit<BF16> {
    typedef uint16_t type;
    static __device__ __forceinline__ float to_float(uint16_t u) { return Num<BF16>::to_float(u); }
    static __device__ __forceinline__ uint16_t from_float(float f) { return Num<BF16>::from_float(f); }
};
template <> struct GateLogit<float> {
    typedef float type;
    static __device__ __forceinline__ float to_float(float f) { return f; }
    static __device__ __forceinline__ float from_float(float f) { return f; }
};

// ---- the exchange steps of a wave reduction ---------------------------------------------------------------------------------
// STEP 0 .. 3: the value of the partner lane inside a row of 16 (every lane active: callers keep the wave whole)
template <int STEP>
static __device__ __forceinline__ uint32_t row_partner(uint32_t v) {
    constexpr int ctrl = STEP == 0 ? 0xB1      // quad_perm [1, 0, 3, 2]
                         : STEP == 1 ? 0x4E    // quad_perm [2, 3, 0, 1]
                         : STEP == 2 ? 0x141   // row_half_mirror: quads agree by now, so this pairs the two quads of a half
                                     : 0x140;  // row_mirror: halves agree, this pairs the two halves of the row
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, ctrl, 0xF, 0xF, true);
}

struct OpMaxF {
    static __device__ __forceinline__ float apply(float a, float b) { return fmaxf(a, b); }
};
struct OpAddF {
    static __device__ __forceinline__ float apply(float a, float b) { return a + b; }
};
struct OpMaxU {
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return a > b ? a : b; }
};

template <typename Op>
static __device__ __forceinline__ uint32_t wave_reduce_bits(uint32_t v, auto from, auto to) {
    v = to(Op::apply(from(v), from(row_partner<0>(v))));
    v = to(Op::apply(from(v), from(row_partner<1>(v))));
    v = to(Op::apply(from(v), from(row_partner<2>(v))));
    v = to(Op::apply(from(v), from(row_partner<3>(v))));
    // rows agree inside themselves; with both operands the same register the swap returns (the even row's, the odd row's) value
    // of each pair of rows in every lane of the pair, then (the lower half's, the upper half's) in every lane
    auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = to(Op::apply(from(r[0]), from(r[1])));
    r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return to(Op::apply(from(r[0]), from(r[1])));
}

template <typename Op>
static __device__ __forceinline__ float wave_reduce(float v) {
    return __uint_as_float(wave_reduce_bits<Op>(__float_as_uint(v), [](uint32_t u) { return __uint_as_float(u); },
                                                [](float f) { return __float_as_uint(f); }));
}

static __device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    return wave_reduce_bits<OpMaxU>(v, [](uint32_t u) { return u; }, [](uint32_t u) { return u; });
}

// ---- the scores of one token --------------------------------------------------------------------------------------------------
// Every lane of the wave calls it with the same arguments.  x: the logits in fp32 (-infinity past E).  v: FLUTE_GATE_SIGMOID
// 1 / (1 + exp(-x)); FLUTE_GATE_SOFTMAX u = exp(x - max), with `normalise` divided by the sum of u over all E (the score s; the
// forward leaves the division out where it renormalises the u directly), 0 past E.  The max and the sum are wave reductions.
template <typename L, int NV>
static __device__ __forceinline__ void gate_scores(const typename GateLogit<L>::type* __restrict__ logits, int E, int scoring,
                                                   bool normalise, int lane, float (&x)[NV], float (&v)[NV]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i;
        x[i] = e < E ? GateLogit<L>::to_float(logits[e]) : -INFINITY;
    }
    if (scoring == FLUTE_GATE_SOFTMAX) {
        float m = x[0];
#pragma unroll
        for (int i = 1; i < NV; ++i) m = fmaxf(m, x[i]);
        m = wave_reduce<OpMaxF>(m);
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = lane + 64 * i < E ? expf(x[i] - m) : 0.0f;
            part += v[i];
        }
        if (normalise) {
            const float total = wave_reduce<OpAddF>(part);
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = v[i] / total;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = 1.0f / (1.0f + expf(-x[i]));
    }
}

// ---- what gate_scores does not return (moe_aux.hip: the auxiliary losses and their backward) ------------------------------------
// Every lane calls it with the x and v of gate_scores(..., normalise = false, ...).  m: the max of the logits, by gate_scores' own
// reduction (the same bits).  u: exp(x - m), 0 past E - FLUTE_GATE_SOFTMAX: v itself; FLUTE_GATE_SIGMOID: computed here.  S: the sum
// of u over all E, lane l adding its experts in ascending order from +0, then the exchange tree - gate_scores' `total`, so u / S is
// bit for bit its normalised score.  Z: the sum the score is normalised by - FLUTE_GATE_SOFTMAX: S; FLUTE_GATE_SIGMOID: the sum of
// the sigmoids v over all E in the same order (past E the sigmoid of -infinity is +0).  gate_scores' own arithmetic is untouched.
template <int NV>
static __device__ __forceinline__ void gate_score_sums(const float (&x)[NV], const float (&v)[NV], int E, int scoring, int lane,
                                                       float (&u)[NV], float& m, float& S, float& Z) {
#pragma clang fp contract(off)
    float mx = x[0];
#pragma unroll
    for (int i = 1; i < NV; ++i) mx = fmaxf(mx, x[i]);
    m = wave_reduce<OpMaxF>(mx);
    float part = 0.0f;
    if (scoring == FLUTE_GATE_SOFTMAX) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            u[i] = v[i];
            part += u[i];
        }
        S = wave_reduce<OpAddF>(part);
        Z = S;
    } else {
        float zpart = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            u[i] = lane + 64 * i < E ? expf(x[i] - m) : 0.0f;
            part += u[i];
            zpart += v[i];
        }
        S = wave_reduce<OpAddF>(part);
        Z = wave_reduce<OpAddF>(zpart);
    }
}

}  // namespace flute_amd
