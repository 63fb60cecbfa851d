// The gating of a mixture-of-experts step: from the router's logits [T, E] to the k experts of every token, ids [T, k] int32,
// and their weights [T, k] fp32 (include/flute_amd.h, flute_moe_gate), and in a second form straight on to every array
// moe_route writes (flute_moe_gate_route): one launch from logits to offsets / perm / rows / row_weight / pos.
//
// One wave = one token.  Lane l holds experts l, l + 64, ... in registers: NV = ceil(E / 64) values, a compile-time count per
// class (1, 2, 4, 8, 16), so the arrays are never indexed by a run-time value and nothing spills.
//   score   the max and the sum over all experts are wave reductions; every lane ends with the same bits.
//   key     each expert's key becomes a 32-bit integer whose unsigned order is the order of the floats (NaN as -infinity, -0
//           as +0); 0 is below every key and marks "no expert here" and "already taken".
//   choice  k rounds: the wave's maximum key, then the lowest expert that holds it - one ballot per register, the first
//           register with a hit and the lowest lane in it, which is scalar work: the tie rule is that comparison of indices,
//           not an accident of the reduction.  The winning lane clears its key.  The winner's score reaches every lane
//           through a v_readlane, and lane j keeps round j's expert and score: the stores are coalesced.
//   weight  the sum of the chosen scores is a compensated (Kahan) sum in slot order, made by every lane alike: at k = 64 a plain
//           running sum would carry up to 63 roundings into every weight of the row.
// A wave reduction is six exchange steps without LDS: DPP quad_perm (lanes ^ 1, ^ 2), row_half_mirror, row_mirror inside a
// row of 16, then v_permlane16_swap and v_permlane32_swap across rows.  Every step combines the same two values in both
// partners, so all 64 lanes hold the same bits afterwards and the order of the additions is fixed.  The exchange steps and the
// score stage (gate_scores) live in moe_gate_score.h, which the gate's backward (router_grad.hip) shares.
// The per-token work is ONE device function, gate_token, which both kernels call: their equal bits rest on it (it is compiled
// with floating-point contraction off, so the two inlined copies cannot differ by a fused multiply-add).
//   moe_gate_kernel        4 waves per workgroup, wave w of block b takes token 4 b + w; the grid covers T.
//   moe_gate_route_kernel  one workgroup of 16 waves (moe_route_kernel's design point): wave w takes tokens w, w + 16, ...,
//                          then a barrier, then the count / scan / place phases of moe_route_sort.h on the ids and
//                          weights just written (same CU, workgroup-scope fence before the barrier).
//   moe_gate_count_kernel  the first launch of the multi-workgroup routing (moe_route_wide.hip), grid = its chunks: workgroup c's wave
//                          w takes the chunk's tokens w, w + 16, ..., then the same fence and barrier, then the count of the chunk's
//                          pairs per expert into its row of the workspace - it reads back only what it wrote itself.
// Group-limited selection (flute_moe_gate_limited / flute_moe_gate_route_limited) is the same two kernels with their LIMITED
// parameter set: gate_token then has one more stage between key and choice (without LIMITED it is not compiled in, and the
// kernels' group arguments, the last of their list, are not read):
//   groups  a wave-uniform loop over the n_group groups.  Group g is experts g gs .. (g + 1) gs - 1, a run of lanes that may
//           straddle registers, so each pass is a wave maximum of the keys under the mask lo <= e < hi.  For the top-2 sum a
//           second maximum follows with the lowest holder of the first left out; the two come back from key to float order and
//           are added once.  Lane g keeps group g's key.
//   pick    topk_group rounds of "largest group key, lowest lane by ballot"; each winner's experts are marked allowed, and
//           afterwards the key of every expert not allowed becomes 0, "no expert here": the k rounds run unchanged.
// One host path serves the four entry points (moe_gate_dispatch): LIMITED, the class NV and the logit type are its three choices.
// No atomics on global memory, plain vector stores, nothing read on the host.
#include "kernels.h"
#include "moe_gate_score.h"
#include "moe_route_sort.h"

namespace flute_amd {

constexpr int kGateWaves = 4;                   // waves per workgroup of the standalone form
constexpr int kGateThreads = 64 * kGateWaves;

// a float as an integer of the same (unsigned) order; NaN ranks as -infinity, -0 as +0; the smallest result is 0x007fffff
static __device__ __forceinline__ uint32_t ordered_key(float f) {
    if (!(f == f)) f = -INFINITY;
    if (f == 0.0f) f = 0.0f;
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the float an ordered key stands for (a NaN comes back as -infinity, -0 as +0)
static __device__ __forceinline__ float key_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// The group stage of the group-limited selection: bit i of the result says that this lane's expert lane + 64 i belongs to one of the
// topk_group best groups.  key: the experts' keys (0 past E); c: what FLUTE_GATE_GROUP_TOP2SUM adds up, s (+ bias).  Every lane calls
// it with the same n_group, gs, topk_group, group_score.
template <int NV>
static __device__ __forceinline__ uint32_t allowed_by_group(const uint32_t (&key)[NV], const float (&c)[NV], int n_group, int gs,
                                                            int topk_group, int group_score, int lane) {
#pragma clang fp contract(off)
    uint32_t ckey[NV];                           // what a group is ranked by, per expert, in key order
#pragma unroll
    for (int i = 0; i < NV; ++i) ckey[i] = group_score == FLUTE_GATE_GROUP_TOP2SUM ? ordered_key(c[i]) : key[i];

    uint32_t gkey = 0u;                          // lane g: group g's key; 0: no group here, or taken (a group key is >= 0x007fffff)
    for (int g = 0; g < n_group; ++g) {
        const int lo = g * gs, hi = lo + gs;     // hi <= E: every expert of a group exists
        uint32_t best = 0u;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = lane + 64 * i;
            if (e >= lo && e < hi) best = OpMaxU::apply(best, ckey[i]);
        }
        best = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(best));
        uint32_t gk = best;
        if (group_score == FLUTE_GATE_GROUP_TOP2SUM) {
            // the lowest expert that holds the maximum is left out of the second maximum (an equal value elsewhere stays in)
            int first = 0;
#pragma unroll
            for (int i = NV - 1; i >= 0; --i) {
                const int e = lane + 64 * i;
                const uint64_t hit = __builtin_amdgcn_ballot_w64(e >= lo && e < hi && ckey[i] == best);
                if (hit) first = 64 * i + (int)__builtin_ctzll(hit);
            }
            uint32_t second = 0u;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int e = lane + 64 * i;
                if (e >= lo && e < hi && e != first) second = OpMaxU::apply(second, ckey[i]);
            }
            second = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(second));      // gs >= 2: an expert is left
            gk = ordered_key(key_value(best) + key_value(second));
        }
        if (lane == g) gkey = gk;
    }

    uint32_t allowed = 0u;
    for (int j = 0; j < topk_group; ++j) {
        const uint32_t best = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(gkey));   // topk_group <= n_group: a group is left
        const int g = (int)__builtin_ctzll(__builtin_amdgcn_ballot_w64(gkey == best));
        if (lane == g) gkey = 0u;
        const int lo = g * gs, hi = lo + gs;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = lane + 64 * i;
            if (e >= lo && e < hi) allowed |= 1u << i;
        }
    }
    return allowed;
}

// ---- one token, one wave ----------------------------------------------------------------------------------------------------
// Every lane of the wave calls it with the same arguments (the exchanges need the whole wave).  Writes ids[0 .. k), weights[0 .. k).
// LIMITED: the group stage is compiled in and n_group, gs = E / n_group, topk_group, group_score are read; without it they are not.
template <typename L, int NV, bool LIMITED>
static __device__ __forceinline__ void gate_token(const typename GateLogit<L>::type* __restrict__ logits,
                                                  const float* __restrict__ bias, int E, int k, int scoring, int renormalize,
                                                  float scale, int n_group, int gs, int topk_group, int group_score, int lane,
                                                  int32_t* ids, float* weights) {
#pragma clang fp contract(off)
    // v: what a chosen expert contributes to the weights - u for a renormalised softmax without bias, else the score s
    // (the top-2 sum of a group is a sum of normalised scores: that form always divides)
    float x[NV], v[NV];
    gate_scores<L, NV>(logits, E, scoring, !renormalize || bias || (LIMITED && group_score == FLUTE_GATE_GROUP_TOP2SUM), lane, x, v);

    uint32_t key[NV];                            // 0: no expert in this slot, or taken
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i;
        const float kf = bias ? v[i] + (e < E ? bias[e] : 0.0f) : x[i];
        key[i] = e < E ? ordered_key(kf) : 0u;
    }

    if constexpr (LIMITED) {
        float c[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = lane + 64 * i;
            c[i] = bias ? v[i] + (e < E ? bias[e] : 0.0f) : v[i];
        }
        const uint32_t allowed = allowed_by_group<NV>(key, c, n_group, gs, topk_group, group_score, lane);
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (!((allowed >> i) & 1u)) key[i] = 0u;
    }

    int my_id = 0;
    float my_v = 0.0f, chosen = 0.0f, lost = 0.0f;      // chosen: the compensated (Kahan) sum of the winners' scores, in slot order
    for (int j = 0; j < k; ++j) {
        uint32_t best = key[0];
#pragma unroll
        for (int i = 1; i < NV; ++i) best = OpMaxU::apply(best, key[i]);
        best = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(best));   // k <= E (LIMITED: k <= topk_group gs): some expert is left, best > 0
        // the lowest index that holds it: the first register with a hit (its experts come before the next register's), the
        // lowest lane in it - scalar work on one ballot per register
        int e = 0;
#pragma unroll
        for (int i = NV - 1; i >= 0; --i) {
            const uint64_t hit = __builtin_amdgcn_ballot_w64(key[i] == best);
            if (hit) e = 64 * i + (int)__builtin_ctzll(hit);
        }
        float mine = 0.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (lane + 64 * i == e) {
                mine = v[i];
                key[i] = 0u;
            }
        }
        const float won = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(mine), e & 63));
        const float term = won - lost;
        const float next = chosen + term;
        lost = (next - chosen) - term;
        chosen = next;
        if (lane == j) {
            my_id = e;
            my_v = won;
        }
    }
    if (lane < k) {
        float w = renormalize ? my_v / chosen : my_v;
        w = w * scale;
        ids[lane] = my_id;
        weights[lane] = w;
    }
}

// ---- the kernels --------------------------------------------------------------------------------------------------------------
// LIMITED picks gate_token's instantiation.  The group arguments come last: every other argument sits where it sits without them,
// and an instantiation without LIMITED does not read them.
template <typename L, int NV, bool LIMITED>
__global__ __launch_bounds__(kGateThreads) void moe_gate_kernel(const typename GateLogit<L>::type* __restrict__ logits,
                                                                const float* __restrict__ bias, int T, int E, int k,
                                                                int scoring, int renormalize, float scale,
                                                                int32_t* __restrict__ ids, float* __restrict__ weights,
                                                                GateGroups g) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * kGateWaves + w;          // T k < 2^27, k >= 1: the grid is below 2^25 and t fits an int
    if (t >= T) return;                                 // the whole wave leaves
    gate_token<L, NV, LIMITED>(logits + (size_t)t * E, bias, E, k, scoring, renormalize, scale, g.n_group,
                               LIMITED ? E / g.n_group : 0, g.topk_group, g.group_score, lane, ids + (size_t)t * k,
                               weights + (size_t)t * k);
}

template <typename L, int NV, bool LIMITED>
__global__ __launch_bounds__(kRouteThreads) void moe_gate_route_kernel(const typename GateLogit<L>::type* __restrict__ logits,
                                                                       const float* __restrict__ bias, int T, int E, int k,
                                                                       int scoring, int renormalize, float scale, int nbits,
                                                                       int32_t* ids, float* weights,
                                                                       int32_t* __restrict__ offsets, int32_t* __restrict__ perm,
                                                                       int32_t* __restrict__ rows, float* __restrict__ row_weight,
                                                                       int32_t* __restrict__ pos, GateGroups g) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gs = LIMITED ? E / g.n_group : 0;
    for (int t = w; t < T; t += kRouteWaves)
        gate_token<L, NV, LIMITED>(logits + (size_t)t * E, bias, E, k, scoring, renormalize, scale, g.n_group, gs, g.topk_group,
                                   g.group_score, lane, ids + (size_t)t * k, weights + (size_t)t * k);
    __threadfence_block();
    __syncthreads();                                    // every wave's ids and weights are written and visible in the workgroup
    route_sort_phases<int32_t, float>(ids, weights, T * k, k, E, nbits, offsets, perm, rows, row_weight, pos);
}

template <typename L, int NV, bool LIMITED>
__global__ __launch_bounds__(kRouteThreads) void moe_gate_count_kernel(const typename GateLogit<L>::type* __restrict__ logits,
                                                                       const float* __restrict__ bias, int T, int E, int k,
                                                                       int scoring, int renormalize, float scale, int chunk_tokens,
                                                                       int32_t* ids, float* weights, int32_t* __restrict__ hist,
                                                                       GateGroups g) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gs = LIMITED ? E / g.n_group : 0;
    int lo, hi;
    route_chunk_pairs(blockIdx.x, chunk_tokens, T, k, &lo, &hi);
    for (int t = lo / k + w; t < hi / k; t += kRouteWaves)      // lo, hi: multiples of k, the chunk's tokens
        gate_token<L, NV, LIMITED>(logits + (size_t)t * E, bias, E, k, scoring, renormalize, scale, g.n_group, gs, g.topk_group,
                                   g.group_score, lane, ids + (size_t)t * k, weights + (size_t)t * k);
    __threadfence_block();
    __syncthreads();                                    // the chunk's ids are written and visible in the workgroup
    route_count_chunk<int32_t>(ids, lo, hi, E, hist + (size_t)blockIdx.x * (E + 1));
}

// ---- the host side: one call, one launch, the ladder of classes and the ladder of logit types ---------------------------------
struct GateCall {
    int T, E, k, scoring, renormalize;
    float scale;
    GateGroups groups;
    const void* logits;
    const float* bias;
    int32_t* ids;
    float* weights;
    int32_t *offsets, *perm, *rows;                     // offsets null: the standalone form, and the four after it are not used
    float* row_weight;
    int32_t* pos;
    hipStream_t stream;
    int chunk_tokens;                                   // hist non-null: the counting form, grid ceil(T / chunk_tokens), and of the
    int32_t* hist;                                      // routing arrays none is used
};

template <typename L, int NV, bool LIMITED>
static int gate_launch(const GateCall& c) {
    const typename GateLogit<L>::type* x = reinterpret_cast<const typename GateLogit<L>::type*>(c.logits);
    if (c.hist) {
        auto kern = moe_gate_count_kernel<L, NV, LIMITED>;
        const size_t lds = route_lds_bytes(c.E);
        if (lds > 65536 &&
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return FLUTE_ERR_LAUNCH;
        const unsigned grid = (unsigned)((c.T + c.chunk_tokens - 1) / c.chunk_tokens);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kRouteThreads), lds, c.stream, x, c.bias, c.T, c.E, c.k, c.scoring, c.renormalize,
                           c.scale, c.chunk_tokens, c.ids, c.weights, c.hist, c.groups);
    } else if (!c.offsets) {
        const unsigned grid = (unsigned)((c.T + kGateWaves - 1) / kGateWaves);
        hipLaunchKernelGGL((moe_gate_kernel<L, NV, LIMITED>), dim3(grid), dim3(kGateThreads), 0, c.stream, x, c.bias, c.T, c.E, c.k,
                           c.scoring, c.renormalize, c.scale, c.ids, c.weights, c.groups);
    } else {
        auto kern = moe_gate_route_kernel<L, NV, LIMITED>;
        const size_t lds = route_lds_bytes(c.E);
        if (lds > 65536 &&
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return FLUTE_ERR_LAUNCH;
        hipLaunchKernelGGL(kern, dim3(1), dim3(kRouteThreads), lds, c.stream, x, c.bias, c.T, c.E, c.k, c.scoring, c.renormalize,
                           c.scale, route_bucket_bits(c.E), c.ids, c.weights, c.offsets, c.perm, c.rows, c.row_weight, c.pos,
                           c.groups);
    }
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

template <typename L, bool LIMITED>
static int gate_by_class(const GateCall& c) {
    if (c.E <= 64) return gate_launch<L, 1, LIMITED>(c);
    if (c.E <= 128) return gate_launch<L, 2, LIMITED>(c);
    if (c.E <= 256) return gate_launch<L, 4, LIMITED>(c);
    if (c.E <= 512) return gate_launch<L, 8, LIMITED>(c);
    return gate_launch<L, 16, LIMITED>(c);
}

template <bool LIMITED>
static int gate_by_type(int logit_dtype, const GateCall& c) {
    if (logit_dtype == FLUTE_F16) return gate_by_class<F16, LIMITED>(c);
    if (logit_dtype == FLUTE_BF16) return gate_by_class<BF16, LIMITED>(c);
    return gate_by_class<float, LIMITED>(c);
}

static int gate_dispatch(int logit_dtype, const GateGroups* groups, GateCall c) {
    // every group allowed: every expert is, and the unlimited kernels serve the call - bit for bit by construction.  T == 0 (the
    // routed form's E + 1 zeros) gates nothing and goes the same way.
    const bool limited = groups && groups->topk_group != groups->n_group && c.T != 0;
    c.groups = limited ? *groups : GateGroups{};
    return limited ? gate_by_type<true>(logit_dtype, c) : gate_by_type<false>(logit_dtype, c);
}

int moe_gate_dispatch(int logit_dtype, int T, int E, int k, const GateGroups* groups, int scoring, int renormalize, float scale,
                      const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* offsets, int32_t* perm,
                      int32_t* rows, float* row_weight, int32_t* pos, hipStream_t stream) {
    return gate_dispatch(logit_dtype, groups, {T, E, k, scoring, renormalize != 0, scale, GateGroups{}, logits, bias, ids, weights,
                                               offsets, perm, rows, row_weight, pos, stream, 0, nullptr});
}

int moe_gate_count_dispatch(int logit_dtype, int T, int E, int k, const GateGroups* groups, int scoring, int renormalize, float scale,
                            int chunk_tokens, const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* hist,
                            hipStream_t stream) {
    return gate_dispatch(logit_dtype, groups, {T, E, k, scoring, renormalize != 0, scale, GateGroups{}, logits, bias, ids, weights,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, stream, chunk_tokens, hist});
}

}  // namespace flute_amd
