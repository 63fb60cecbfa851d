// The counting sort of moe_route.hip as device code two kernels share: moe_route_kernel (moe_route.hip), which is nothing else,
// and moe_gate_route_kernel (moe_gate.hip), which first writes the ids and weights it sorts.  The description of the phases is at
// the top of moe_route.hip.
#pragma once
#include "common.h"

namespace flute_amd {

constexpr int kRouteWaves = 16;
constexpr int kRouteThreads = 64 * kRouteWaves;

template <typename W> struct RouteWeight;
template <> struct RouteWeight<F16> {
    typedef uint16_t type;
    static __device__ __forceinline__ float to_float(uint16_t u) { return Num<F16>::to_float(u); }
};
template <> struct RouteWeight<BF16> {
    typedef uint16_t type;
    static __device__ __forceinline__ float to_float(uint16_t u) { return Num<BF16>::to_float(u); }
};
template <> struct RouteWeight<float> {
    typedef float type;
    static __device__ __forceinline__ float to_float(float f) { return f; }
};

// the comparison is made at the ids' own width: an int64 id of 2^32 + 1 is outside, not expert 1
template <typename IdT>
static __device__ __forceinline__ int route_bucket(const IdT* ids, int p, int E) {
    const IdT v = ids[p];
    return (v >= 0 && v < (IdT)E) ? (int)v : E;
}

// count / scan / place on the whole workgroup (kRouteThreads threads, every one of them calls it; route_lds_bytes(E) of dynamic
// LDS).  ids and weights carry no __restrict__ here: the gating kernel (moe_gate.hip) writes them in the same launch, before a barrier.
template <typename IdT, typename W>
static __device__ __forceinline__ void route_sort_phases(const IdT* ids, const typename RouteWeight<W>::type* weights, int P,
                                                         int k, int E, int nbits, int32_t* __restrict__ offsets,
                                                         int32_t* __restrict__ perm, int32_t* __restrict__ rows,
                                                         float* __restrict__ row_weight, int32_t* __restrict__ pos) {
    extern __shared__ int route_lds[];
    const int B = E + 1;
    int* cnt = route_lds;                      // [16][B]
    int* tot = route_lds + kRouteWaves * B;    // [B]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per = (((P + kRouteWaves - 1) / kRouteWaves + 63) / 64) * 64;      // P < 2^27: 16 per fits an int
    const int begin = w * per;
    const int end = min(P, begin + per);                                        // begin >= P: an empty range
    int* mine = cnt + w * B;

    const int b_first = (begin + lane < end) ? route_bucket(ids, begin + lane, E) : 0;
    for (int i = tid; i < kRouteWaves * B; i += kRouteThreads) cnt[i] = 0;
    __syncthreads();

    for (int c = begin; c < end; c += 64) {
        const int p = c + lane;
        if (p < end) atomicAdd(&mine[c == begin ? b_first : route_bucket(ids, p, E)], 1);
    }
    __syncthreads();

    for (int b = tid; b < B; b += kRouteThreads) {
        int run = 0;
#pragma unroll
        for (int v = 0; v < kRouteWaves; ++v) {
            const int c = cnt[v * B + b];
            cnt[v * B + b] = run;
            run += c;
        }
        tot[b] = run;
    }
    __syncthreads();
    if (w == 0) {
        const int chunk = (B + 63) / 64;
        const int b0 = min(lane * chunk, B), b1 = min(b0 + chunk, B);
        int sum = 0;
        for (int b = b0; b < b1; ++b) sum += tot[b];
        int incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        int run = incl - sum;
        for (int b = b0; b < b1; ++b) {
            const int c = tot[b];
            tot[b] = run;
            offsets[b] = run;                  // B = E + 1 entries: offsets[E] = the pairs some expert serves
            run += c;
        }
    }
    __syncthreads();

    for (int c = begin; c < end; c += 64) {
        const int p = c + lane;
        const bool valid = p < end;
        const int b = c == begin ? b_first : (valid ? route_bucket(ids, p, E) : 0);
        uint64_t group = __builtin_amdgcn_ballot_w64(valid);
        for (int bit = 0; bit < nbits; ++bit) {
            const bool one = (b >> bit) & 1;
            const uint64_t set = __builtin_amdgcn_ballot_w64(valid && one);
            group &= one ? set : ~set;
        }
        if (valid) {
            const int base = mine[b];
            const int i = tot[b] + base + __popcll(group & ((1ull << lane) - 1));
            if ((group >> lane) == 1) mine[b] = base + __popcll(group);     // the group's highest lane
            perm[i] = p;
            rows[i] = p / k;
            if (weights) row_weight[i] = RouteWeight<W>::to_float(weights[p]);
            pos[p] = i;
        }
    }
}

// dynamic LDS of a launch that runs route_sort_phases: cnt [16][E + 1] and tot [E + 1]
static inline size_t route_lds_bytes(int E) { return (size_t)(kRouteWaves + 1) * (size_t)(E + 1) * sizeof(int); }
// bits of the largest bucket number, E
static inline int route_bucket_bits(int E) {
    int nbits = 0;
    while ((E >> nbits) != 0) ++nbits;
    return nbits;
}

}  // namespace flute_amd
