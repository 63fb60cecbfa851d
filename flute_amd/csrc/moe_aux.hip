// The router's auxiliary losses and their backward (include/flute_amd.h, flute_moe_aux_loss and flute_moe_aux_loss_grad state the
// definitions, the summation order and the refusals):
//
//   moe_aux_partial_kernel   grid C: chunk c's partial sums of p per expert, its slot counts per expert and its sum of lse^2
//   moe_aux_finish_kernel    one workgroup: the chunks in ascending order in fp64 -> load, importance, balance, z
//   moe_aux_grad_kernel      one wave = one token: d_logits from the logits, load [E] and grads [2] on the device
//
// moe_aux_partial_kernel: one workgroup of 4 waves per chunk of chunk_tokens tokens.  Wave w walks the chunk's tokens w, w + 4, ... in
// ascending order; the scores of a token are gate_scores' (moe_gate_score.h), gate_score_sums adds the max, the sum of the
// exponentials and the sigmoid's normalisation.  Lane l keeps the running sums of p of its experts l, l + 64, ... in NV registers, the
// wave its running sum of lse^2 (wave-uniform).  The waves meet in LDS and are added in wave order, ((w0 + w1) + w2) + w3; a wave
// without a token adds +0.  The chunk's slots are counted by all 256 lanes with integer atomics in LDS (integers: any order gives the
// same count).  The chunk then writes its whole row - E sums, E counts, zeros included, and one sum of lse^2 - with plain stores.
// moe_aux_finish_kernel: 1024 lanes.  The chunks' rows pass through LDS a tile at a time, loaded by all lanes; lane e < E adds
// expert e's column of the tile in ascending chunk order in fp64.  Lane 0 then forms balance and z in fp64 from LDS, in ascending
// order.  No float atomics, no workgroup waits on another: the kernel boundary is the only ordering between workgroups, and every
// word of the workspace the finish reads was written by the first launch of the same call.
// moe_aux_grad_kernel: the shape of moe_gate_grad_kernel (router_grad.hip).  No LDS, no atomics, plain vector stores.
#include "kernels.h"
#include "moe_gate_score.h"

namespace flute_amd {

constexpr int kAuxWaves = 4;                                       // waves per workgroup of the partials and of the backward
constexpr int kAuxThreads = 64 * kAuxWaves;
constexpr int kAuxFinishThreads = 1024;                            // >= FLUTE_MOE_ROUTE_MAX_EXPERTS: one lane per expert
constexpr int kAuxTileWords = 8192;                                // the finish's LDS tile: 32 KB, at least 8 chunks of 1024 experts

template <typename L, int NV>
__global__ __launch_bounds__(kAuxThreads) void moe_aux_partial_kernel(const typename GateLogit<L>::type* __restrict__ logits,
                                                                      const int32_t* __restrict__ ids, int T, int E, int k,
                                                                      int scoring, int chunk_tokens, float* __restrict__ psum,
                                                                      int32_t* __restrict__ pcnt, float* __restrict__ pz) {
#pragma clang fp contract(off)
    __shared__ float part[kAuxWaves][64 * NV];
    __shared__ int cnt[64 * NV];
    __shared__ float zpart[kAuxWaves];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x;
    const int t0 = c * chunk_tokens;                               // c < C: c chunk_tokens < T
    const int t1 = T - t0 < chunk_tokens ? T : t0 + chunk_tokens;

    for (int e = threadIdx.x; e < 64 * NV; e += kAuxThreads) cnt[e] = 0;
    __syncthreads();
    const size_t p1 = (size_t)t1 * k;
    for (size_t i = (size_t)t0 * k + threadIdx.x; i < p1; i += kAuxThreads) {
        const int id = ids[i];
        if (id >= 0 && id < E) atomicAdd(&cnt[id], 1);
    }

    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0f;
    float zsum = 0.0f;
    for (int t = t0 + wv; t < t1; t += kAuxWaves) {                // uniform in the wave: every lane stays
        float x[NV], v[NV], u[NV], m, S, Z;
        gate_scores<L, NV>(logits + (size_t)t * E, E, scoring, false, lane, x, v);
        gate_score_sums<NV>(x, v, E, scoring, lane, u, m, S, Z);
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = acc[i] + v[i] / Z;
        const float lse = m + logf(S);
        zsum = zsum + lse * lse;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) part[wv][lane + 64 * i] = acc[i];
    if (lane == 0) zpart[wv] = zsum;
    __syncthreads();

    const size_t row = (size_t)c * E;
    for (int e = threadIdx.x; e < E; e += kAuxThreads) {
        float s = part[0][e];
#pragma unroll
        for (int w = 1; w < kAuxWaves; ++w) s = s + part[w][e];
        psum[row + e] = s;
        pcnt[row + e] = cnt[e];
    }
    if (threadIdx.x == 0) {
        float s = zpart[0];
#pragma unroll
        for (int w = 1; w < kAuxWaves; ++w) s = s + zpart[w];
        pz[c] = s;
    }
}

__global__ __launch_bounds__(kAuxFinishThreads) void moe_aux_finish_kernel(const float* __restrict__ psum,
                                                                           const int32_t* __restrict__ pcnt,
                                                                           const float* __restrict__ pz, int T, int E, int C,
                                                                           int32_t* __restrict__ load,
                                                                           float* __restrict__ importance,
                                                                           float* __restrict__ losses) {
#pragma clang fp contract(off)
    __shared__ uint32_t tile[kAuxTileWords];
    __shared__ double term[kAuxFinishThreads];
    const int e = threadIdx.x;
    const int rows = kAuxTileWords / E;                            // chunks per tile: E <= 1024, so at least 8

    double sum = 0.0;
    for (int c0 = 0; c0 < C; c0 += rows) {
        const int n = min(rows, C - c0) * E;
        const size_t base = (size_t)c0 * E;
        for (int i = threadIdx.x; i < n; i += kAuxFinishThreads) tile[i] = __float_as_uint(psum[base + i]);
        __syncthreads();
        if (e < E) {
#pragma unroll 8
            for (int i = e; i < n; i += E) sum = sum + (double)__uint_as_float(tile[i]);
        }
        __syncthreads();
    }
    int count = 0;
    for (int c0 = 0; c0 < C; c0 += rows) {
        const int n = min(rows, C - c0) * E;
        const size_t base = (size_t)c0 * E;
        for (int i = threadIdx.x; i < n; i += kAuxFinishThreads) tile[i] = (uint32_t)pcnt[base + i];
        __syncthreads();
        if (e < E) {
#pragma unroll 8
            for (int i = e; i < n; i += E) count += (int)tile[i];
        }
        __syncthreads();
    }
    if (e < E) {
        load[e] = count;
        importance[e] = (float)sum;
        term[e] = (double)count * sum;
    }
    // the chunks' sums of lse^2 pass through the same tile, C <= FLUTE_MOE_ROUTE_MAX_CHUNKS = kAuxTileWords words
    for (int i = threadIdx.x; i < C; i += kAuxFinishThreads) tile[i] = __float_as_uint(pz[i]);
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0;
        for (int i = 0; i < E; ++i) b = b + term[i];
        const double tt = (double)T;
        losses[0] = (float)(((double)E * b) / (tt * tt));
    }
    if (threadIdx.x == 64) {                                       // another wave: the two serial sums run side by side
        double z = 0.0;
        for (int i = 0; i < C; ++i) z = z + (double)__uint_as_float(tile[i]);
        losses[1] = (float)(z / (double)T);
    }
}

template <typename L, int NV>
__global__ __launch_bounds__(kAuxThreads) void moe_aux_grad_kernel(const typename GateLogit<L>::type* __restrict__ logits,
                                                                   const int32_t* __restrict__ load,
                                                                   const float* __restrict__ grads,
                                                                   typename GateLogit<L>::type* __restrict__ d_logits, int T, int E,
                                                                   int scoring) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * kAuxWaves + wv;                     // T < 2^27: t fits an int
    if (t >= T) return;                                            // the whole wave leaves

    float x[NV], v[NV], u[NV], m, S, Z;
    gate_scores<L, NV>(logits + (size_t)t * E, E, scoring, false, lane, x, v);
    gate_score_sums<NV>(x, v, E, scoring, lane, u, m, S, Z);

    const float tf = (float)T;
    const float ab = grads[0] * ((float)E / (tf * tf));
    const float zc = (grads[1] * (2.0f / tf)) * (m + logf(S));
    float a[NV], p[NV];
    float dpart = 0.0f;                                            // register order, then the exchange tree
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i;
        a[i] = e < E ? ab * (float)load[e] : 0.0f;
        p[i] = v[i] / Z;
        dpart = dpart + a[i] * p[i];
    }
    const float D = wave_reduce<OpAddF>(dpart);

    typename GateLogit<L>::type* out = d_logits + (size_t)t * E;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int e = lane + 64 * i;
        float dx;
        if (scoring == FLUTE_GATE_SOFTMAX)
            dx = p[i] * (a[i] - D) + zc * p[i];
        else
            dx = (v[i] * (1.0f - v[i])) * ((a[i] - D) / Z) + zc * (u[i] / S);
        if (e < E) out[e] = GateLogit<L>::from_float(dx + 0.0f);   // -0 + +0 = +0: a zero is written as +0
    }
}

struct AuxCall {
    int T, E, k, scoring, chunk_tokens, C;
    const void* logits;
    const int32_t* ids;
    float* psum;
    int32_t* pcnt;
    float* pz;
    const int32_t* load;
    const float* grads;
    void* d_logits;
    hipStream_t stream;
};

template <typename L, int NV>
static int aux_launch(const AuxCall& c) {
    typedef typename GateLogit<L>::type X;
    if (c.d_logits) {
        const unsigned grid = (unsigned)((c.T + kAuxWaves - 1) / kAuxWaves);
        hipLaunchKernelGGL((moe_aux_grad_kernel<L, NV>), dim3(grid), dim3(kAuxThreads), 0, c.stream,
                           reinterpret_cast<const X*>(c.logits), c.load, c.grads, reinterpret_cast<X*>(c.d_logits), c.T, c.E,
                           c.scoring);
    } else {
        hipLaunchKernelGGL((moe_aux_partial_kernel<L, NV>), dim3((unsigned)c.C), dim3(kAuxThreads), 0, c.stream,
                           reinterpret_cast<const X*>(c.logits), c.ids, c.T, c.E, c.k, c.scoring, c.chunk_tokens, c.psum, c.pcnt,
                           c.pz);
    }
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

template <typename L>
static int aux_by_class(const AuxCall& c) {                        // the gate's ladder of classes
    if (c.E <= 64) return aux_launch<L, 1>(c);
    if (c.E <= 128) return aux_launch<L, 2>(c);
    if (c.E <= 256) return aux_launch<L, 4>(c);
    if (c.E <= 512) return aux_launch<L, 8>(c);
    return aux_launch<L, 16>(c);
}

static int aux_by_type(int logit_dtype, const AuxCall& c) {
    if (logit_dtype == FLUTE_F16) return aux_by_class<F16>(c);
    if (logit_dtype == FLUTE_BF16) return aux_by_class<BF16>(c);
    return aux_by_class<float>(c);
}

int moe_aux_loss_dispatch(int logit_dtype, int T, int E, int k, int scoring, int chunk_tokens, const void* logits,
                          const int32_t* ids, void* workspace, int32_t* load, float* importance, float* losses,
                          hipStream_t stream) {
    const int C = (int)(((long long)T + chunk_tokens - 1) / chunk_tokens);
    float* psum = reinterpret_cast<float*>(workspace);
    int32_t* pcnt = reinterpret_cast<int32_t*>(psum + (size_t)C * E);
    float* pz = reinterpret_cast<float*>(pcnt + (size_t)C * E);
    const AuxCall c = {T, E, k, scoring, chunk_tokens, C, logits, ids, psum, pcnt, pz, nullptr, nullptr, nullptr, stream};
    const int rc = aux_by_type(logit_dtype, c);
    if (rc) return rc;
    hipLaunchKernelGGL(moe_aux_finish_kernel, dim3(1), dim3(kAuxFinishThreads), 0, stream, psum, pcnt, pz, T, E, C, load, importance,
                       losses);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

int moe_aux_loss_grad_dispatch(int logit_dtype, int T, int E, int scoring, const void* logits, const int32_t* load,
                               const float* grads, void* d_logits, hipStream_t stream) {
    const AuxCall c = {T, E, 0, scoring, 0, 0, logits, nullptr, nullptr, nullptr, nullptr, load, grads, d_logits, stream};
    return aux_by_type(logit_dtype, c);
}

}  // namespace flute_amd
