// The router's backward, the two pieces that are not GEMMs (include/flute_amd.h, flute_moe_weight_grad and flute_moe_gate_grad
// state the contracts, the summation order and the error account):
//
//   moe_weight_grad_kernel   d_row_weight[r] = sum_k (float) dHp[r, k] (float) H[r, k],  dH[r, k] = round_T(row_weight[r] (float) dHp[r, k])
//   moe_gate_grad_kernel     d_logits [T, E] from the gradients of the gate's weights [T, k] and / or of row_weight through pos
//
// moe_weight_grad_kernel: one workgroup of 256 lanes = one row, so the row and its `served` test are uniform in the workgroup and
// the grid follows from R alone.  A lane takes 8 consecutive columns - one 16-byte load from each operand, one 16-byte store - per
// step of 2048 columns, and adds its products in column order across its steps (acc = acc + p, one rounding each, no fma; the
// products of two fp16 or two bf16 values are exact in fp32).  The 64 lanes of a wave combine in moe_gate_score.h's exchange tree
// (lanes ^ 1, ^ 2, the quads of a half, the halves of a row of 16, the rows of a pair, the halves of the wave), the four waves in
// wave order through 16 bytes of LDS: ((w0 + w1) + w2) + w3.  No atomics: a row's results depend neither on R nor on its position.
// The rows at or past served = clamp(offsets[E], 0, R) are written as +0 and none of their operands is read.
//
// moe_gate_grad_kernel: one wave = one token, as the forward; the scores come from the forward's own gate_scores.  Lane j < k holds
// slot j (its id, its incoming gradient, its score); everything over the slots is a wave-uniform loop in slot order on values
// fetched by v_readlane, so every lane forms the same sums in the same order.  No LDS, no atomics, plain vector stores.
#include "kernels.h"
#include "grouped_rows.h"
#include "moe_gate_score.h"

namespace flute_amd {

constexpr int kWeightGradThreads = 256;
constexpr int kWeightGradWaves = kWeightGradThreads / 64;
constexpr int kWeightGradStep = 8 * kWeightGradThreads;            // columns per step

template <typename T>
__global__ __launch_bounds__(kWeightGradThreads) void moe_weight_grad_kernel(const uint16_t* __restrict__ DHP,
                                                                             const uint16_t* __restrict__ H,
                                                                             const float* __restrict__ row_weight,
                                                                             const int32_t* __restrict__ offsets,
                                                                             float* __restrict__ d_row_weight,
                                                                             uint16_t* __restrict__ DH, int E, int R, int K) {
#pragma clang fp contract(off)
    __shared__ float wave_sum[kWeightGradWaves];
    const int r = blockIdx.x;
    const size_t base = (size_t)r * K;
    const int served = offsets ? grouped_served(offsets, E, R) : R;
    if (r >= served) {                                             // uniform: the whole workgroup takes this branch
        if (DH)
            for (int col = 8 * threadIdx.x; col < K; col += kWeightGradStep)
                *reinterpret_cast<uint4*>(DH + base + col) = make_uint4(0, 0, 0, 0);
        if (threadIdx.x == 0) d_row_weight[r] = 0.0f;
        return;
    }
    const float w = DH ? row_weight[r] : 0.0f;
    float acc = 0.0f;
    for (int col = 8 * threadIdx.x; col < K; col += kWeightGradStep) {
        const uint4 dv = *reinterpret_cast<const uint4*>(DHP + base + col);
        const uint4 hv = *reinterpret_cast<const uint4*>(H + base + col);
        const uint32_t dw[4] = {dv.x, dv.y, dv.z, dv.w}, hw[4] = {hv.x, hv.y, hv.z, hv.w};
        uint32_t ow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d0 = Num<T>::to_float((uint16_t)(dw[i] & 0xffffu)), d1 = Num<T>::to_float((uint16_t)(dw[i] >> 16));
            const float h0 = Num<T>::to_float((uint16_t)(hw[i] & 0xffffu)), h1 = Num<T>::to_float((uint16_t)(hw[i] >> 16));
            acc = acc + d0 * h0;
            acc = acc + d1 * h1;
            ow[i] = (uint32_t)Num<T>::from_float(w * d0) | ((uint32_t)Num<T>::from_float(w * d1) << 16);
        }
        if (DH) *reinterpret_cast<uint4*>(DH + base + col) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
    acc = wave_reduce<OpAddF>(acc);                                // every lane of the wave holds the wave's sum
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = wave_sum[0];
#pragma unroll
        for (int i = 1; i < kWeightGradWaves; ++i) s = s + wave_sum[i];
        d_row_weight[r] = s;
    }
}

int moe_weight_grad_dispatch(int dtype, int R, int K, int E, const void* dHp, const void* H, const float* row_weight,
                             const int32_t* offsets, float* d_row_weight, void* dH, hipStream_t stream) {
    const uint16_t* d16 = reinterpret_cast<const uint16_t*>(dHp);
    const uint16_t* h16 = reinterpret_cast<const uint16_t*>(H);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(dH);
    if (dtype == FLUTE_F16)
        hipLaunchKernelGGL(moe_weight_grad_kernel<F16>, dim3((unsigned)R), dim3(kWeightGradThreads), 0, stream, d16, h16, row_weight,
                           offsets, d_row_weight, o16, E, R, K);
    else
        hipLaunchKernelGGL(moe_weight_grad_kernel<BF16>, dim3((unsigned)R), dim3(kWeightGradThreads), 0, stream, d16, h16, row_weight,
                           offsets, d_row_weight, o16, E, R, K);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

// ---- the gate's backward ------------------------------------------------------------------------------------------------------
constexpr int kGateGradWaves = 4;                                  // waves per workgroup, the forward's standalone form
constexpr int kGateGradThreads = 64 * kGateGradWaves;

static __device__ __forceinline__ float lane_value(float v, int lane) {       // lane: wave-uniform
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}

template <typename L, int NV>
__global__ __launch_bounds__(kGateGradThreads) void moe_gate_grad_kernel(const typename GateLogit<L>::type* __restrict__ logits,
                                                                         const int32_t* __restrict__ ids,
                                                                         const float* __restrict__ d_weights,
                                                                         const float* __restrict__ d_row_weight,
                                                                         const int32_t* __restrict__ pos,
                                                                         typename GateLogit<L>::type* __restrict__ d_logits, int T,
                                                                         int E, int k, int scoring, int renormalize, float scale) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * kGateGradWaves + wv;                // T k < 2^27, k >= 1: t fits an int
    if (t >= T) return;                                            // the whole wave leaves

    float x[NV], s[NV];
    gate_scores<L, NV>(logits + (size_t)t * E, E, scoring, true, lane, x, s);

    // lane j < k: slot j's expert, whether it names one, and its incoming gradient q_j
    int my_id = -1;
    float my_q = 0.0f;
    if (lane < k) {
        const size_t at = (size_t)t * k + lane;
        my_id = ids[at];
        if (d_weights) my_q = d_weights[at];
        if (pos) {
            const int p = pos[at];
            if (p >= 0 && p < T * k) my_q = my_q + d_row_weight[p];
        }
    }

    float my_ds;
    if (renormalize) {
        // pass 1, slot order: s_j of every slot into lane j, and S = the sum of the s_j
        float my_s = 0.0f, S = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int id = __builtin_amdgcn_readlane(my_id, j);
            if (id < 0 || id >= E) continue;                       // uniform
            float cand = 0.0f;
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if ((id >> 6) == i) cand = s[i];
            const float sj = lane_value(cand, id & 63);
            S = S + sj;
            if (lane == j) my_s = sj;
        }
        // pass 2, slot order: B = the sum of q_j w_j
        const float my_term = my_q * (my_s / S);
        float B = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int id = __builtin_amdgcn_readlane(my_id, j);
            if (id < 0 || id >= E) continue;
            B = B + lane_value(my_term, j);
        }
        my_ds = (scale * (my_q - B)) / S;
    } else {
        my_ds = scale * my_q;
    }

    // pass 3, slot order: ds_e = the sum of the ds_j of the slots that name expert e
    float ds[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) ds[i] = 0.0f;
    for (int j = 0; j < k; ++j) {
        const int id = __builtin_amdgcn_readlane(my_id, j);
        if (id < 0 || id >= E) continue;
        const float d = lane_value(my_ds, j);
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (lane + 64 * i == id) ds[i] = ds[i] + d;
    }

    float dx[NV];
    if (scoring == FLUTE_GATE_SOFTMAX) {
        float part = 0.0f;                                         // register order, then the exchange tree
#pragma unroll
        for (int i = 0; i < NV; ++i) part = part + ds[i] * s[i];
        const float dot = wave_reduce<OpAddF>(part);
#pragma unroll
        for (int i = 0; i < NV; ++i) dx[i] = s[i] * (ds[i] - dot);
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) dx[i] = (ds[i] * s[i]) * (1.0f - s[i]);
    }
    typename GateLogit<L>::type* out = d_logits + (size_t)t * E;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i;
        if (e < E) out[e] = GateLogit<L>::from_float(dx[i]);
    }
}

struct GateGradCall {
    int T, E, k, scoring, renormalize;
    float scale;
    const void* logits;
    const int32_t* ids;
    const float *d_weights, *d_row_weight;
    const int32_t* pos;
    void* d_logits;
    hipStream_t stream;
};

template <typename L, int NV>
static int gate_grad_launch(const GateGradCall& c) {
    typedef typename GateLogit<L>::type X;
    const unsigned grid = (unsigned)((c.T + kGateGradWaves - 1) / kGateGradWaves);
    hipLaunchKernelGGL((moe_gate_grad_kernel<L, NV>), dim3(grid), dim3(kGateGradThreads), 0, c.stream,
                       reinterpret_cast<const X*>(c.logits), c.ids, c.d_weights, c.d_row_weight, c.pos,
                       reinterpret_cast<X*>(c.d_logits), c.T, c.E, c.k, c.scoring, c.renormalize, c.scale);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

template <typename L>
static int gate_grad_by_class(const GateGradCall& c) {             // the forward's ladder of classes
    if (c.E <= 64) return gate_grad_launch<L, 1>(c);
    if (c.E <= 128) return gate_grad_launch<L, 2>(c);
    if (c.E <= 256) return gate_grad_launch<L, 4>(c);
    if (c.E <= 512) return gate_grad_launch<L, 8>(c);
    return gate_grad_launch<L, 16>(c);
}

int moe_gate_grad_dispatch(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale, const void* logits,
                           const int32_t* ids, const float* d_weights, const float* d_row_weight, const int32_t* pos,
                           void* d_logits, hipStream_t stream) {
    const GateGradCall c = {T, E, k, scoring, renormalize != 0, scale, logits, ids, d_weights, d_row_weight, pos, d_logits, stream};
    if (logit_dtype == FLUTE_F16) return gate_grad_by_class<F16>(c);
    if (logit_dtype == FLUTE_BF16) return gate_grad_by_class<BF16>(c);
    return gate_grad_by_class<float>(c);
}

}  // namespace flute_amd
