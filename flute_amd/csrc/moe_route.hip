// The routing of a mixture-of-experts step in ONE launch: from the router's choice ids [T, k] (and weights [T, k]) to
// everything the grouped launches and moe_combine read - offsets [E + 1], perm [P], rows [P], row_weight [P], pos [T, k],
// P = T k (include/flute_amd.h, flute_moe_route; the arrays are integrations/moe.py sort_by_expert's, value for value).
//
// A stable counting sort inside ONE workgroup of 16 waves; bucket e < E = expert e, bucket E = every id outside [0, E).
//   count   wave w owns the contiguous pairs [w per, (w + 1) per) and counts them into its own row of cnt[16][E + 1] in
//           LDS (ds_add; integer counts, so their order does not matter).
//   scan    one thread per bucket turns its column of cnt into the waves' exclusive prefix and leaves the bucket's total
//           in tot; wave 0 turns tot into the buckets' exclusive prefix, which is `offsets`.
//   place   every wave walks its range again in order, 64 pairs at a time.  The lanes of one bucket are found with one
//           ballot per bit of the bucket number; a lane's rank is the popcount of its group below it, its row is
//           tot[b] + cnt[w][b] + rank, and the highest lane of the group adds the group's size to cnt[w][b].  The new
//           value is computed from the one every lane of the group has read (a data dependence: the read of all lanes
//           precedes the leader's write), and a wave's DS operations execute in program order.
// Waves never touch another wave's row after the scan and the ranges are ordered by wave, so the result does not
// depend on scheduling: pairs of one bucket keep their original order.  No atomics on global memory; all five outputs
// are plain vector stores.  The ids are read twice from global memory except a wave's first 64, which stay in a
// register (at decode sizes, P <= 1024, that is all of them and the load overlaps the clearing of the table).
// One workgroup is the design point: decode-sized P.  It is correct for every P the ABI accepts (each wave loops over
// its range), but a prefill-sized P is sorted by 1024 threads; a multi-workgroup form does not exist.
#include "kernels.h"
#include "../../include/flute_amd.h"

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
static __device__ __forceinline__ int route_bucket(const IdT* __restrict__ ids, int p, int E) {
    const IdT v = ids[p];
    return (v >= 0 && v < (IdT)E) ? (int)v : E;
}

template <typename IdT, typename W>
__global__ __launch_bounds__(kRouteThreads) void moe_route_kernel(const IdT* __restrict__ ids,
                                                                  const typename RouteWeight<W>::type* __restrict__ weights,
                                                                  int P, int k, int E, int nbits,
                                                                  int32_t* __restrict__ offsets, int32_t* __restrict__ perm,
                                                                  int32_t* __restrict__ rows, float* __restrict__ row_weight,
                                                                  int32_t* __restrict__ pos) {
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

int moe_route_dispatch(int id_dtype, int weight_dtype, int P, int k, int E, const void* ids, const void* weights,
                       int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos,
                       hipStream_t stream) {
    const size_t lds = (size_t)(kRouteWaves + 1) * (size_t)(E + 1) * sizeof(int);      // cnt [16][E + 1] and tot [E + 1]
    int nbits = 0;
    while ((E >> nbits) != 0) ++nbits;             // bits of the largest bucket number, E
    const void* fn = nullptr;
#define FLUTE_ROUTE(ID, WT)                                                                                            \
    {                                                                                                                  \
        auto kern = moe_route_kernel<ID, WT>;                                                                          \
        fn = (const void*)kern;                                                                                        \
        if (lds > 65536 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) \
            return FLUTE_ERR_LAUNCH;                                                                                   \
        hipLaunchKernelGGL(kern, dim3(1), dim3(kRouteThreads), lds, stream, reinterpret_cast<const ID*>(ids),          \
                           reinterpret_cast<const typename RouteWeight<WT>::type*>(weights), P, k, E, nbits, offsets,  \
                           perm, rows, row_weight, pos);                                                               \
    }
#define FLUTE_ROUTE_W(ID)                              \
    if (weight_dtype == FLUTE_F16) FLUTE_ROUTE(ID, F16) \
    else if (weight_dtype == FLUTE_BF16) FLUTE_ROUTE(ID, BF16) \
    else FLUTE_ROUTE(ID, float)
    if (id_dtype == FLUTE_I32) { FLUTE_ROUTE_W(int32_t) }
    else { FLUTE_ROUTE_W(int64_t) }
#undef FLUTE_ROUTE_W
#undef FLUTE_ROUTE
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
