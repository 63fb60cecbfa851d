// The counting sort of moe_route.hip as device code every routing kernel shares: moe_route_kernel (moe_route.hip) and
// moe_gate_route_kernel (moe_gate.hip), one workgroup each, and the three launches of the multi-workgroup form
// (moe_route_wide.hip; moe_gate_count_kernel, its gated first launch, in moe_gate.hip).  The description of the phases is at the top
// of moe_route.hip, that of the multi-workgroup form at the top of moe_route_wide.hip.
//
// A workgroup sorts one CHUNK, the contiguous pairs [lo, hi): its 16 waves own contiguous sub-ranges of it rounded up to 64 pairs
// (route_wave_range).  The one-workgroup kernels are the case "one chunk, [0, P), base 0" (route_sort_phases); a chunk of the
// multi-workgroup form differs in two loads only - where the buckets' totals come from and what a bucket's count starts at
// (route_sort_chunk) - and in nothing that decides an order.
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

// wave w's share of the chunk [lo, hi): [begin, end), and the bucket of this lane's pair among its first 64 (0 where it has none), which
// stays in a register over both walks
struct RouteWave {
    int begin, end, b_first;
};
template <typename IdT>
static __device__ __forceinline__ RouteWave route_wave_range(const IdT* ids, int lo, int hi, int E, int w, int lane) {
    const int n = hi - lo;
    const int per = (((n + kRouteWaves - 1) / kRouteWaves + 63) / 64) * 64;      // hi <= P < 2^27: lo + 16 per fits an int
    RouteWave r;
    r.begin = lo + w * per;
    r.end = min(hi, r.begin + per);                                             // begin >= hi: an empty range
    r.b_first = (r.begin + lane < r.end) ? route_bucket(ids, r.begin + lane, E) : 0;
    return r;
}

// count: cnt [16][B] cleared, then wave w counts its range into row w (ds_add; integer counts, so their order does not matter).  Ends
// behind a barrier.
template <typename IdT>
static __device__ __forceinline__ void route_count(const IdT* ids, const RouteWave& r, int E, int* cnt) {
    const int B = E + 1;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    int* mine = cnt + __builtin_amdgcn_readfirstlane(tid >> 6) * B;
    for (int i = tid; i < kRouteWaves * B; i += kRouteThreads) cnt[i] = 0;
    __syncthreads();
    for (int c = r.begin; c < r.end; c += 64) {
        const int p = c + lane;
        if (p < r.end) atomicAdd(&mine[c == r.begin ? r.b_first : route_bucket(ids, p, E)], 1);
    }
    __syncthreads();
}

// scan over the waves: one thread per bucket turns its column of cnt into the waves' exclusive prefix, starting at base[b] (null: 0),
// and leaves in tot[b] the bucket's count over the workgroup, or total[b] where that is given.  Ends behind a barrier.
static __device__ __forceinline__ void route_wave_prefix(int* cnt, int* tot, int B, const int* __restrict__ base,
                                                         const int* __restrict__ total) {
    for (int b = threadIdx.x; b < B; b += kRouteThreads) {
        int run = base ? base[b] : 0;
        const int first = run;
#pragma unroll
        for (int v = 0; v < kRouteWaves; ++v) {
            const int c = cnt[v * B + b];
            cnt[v * B + b] = run;
            run += c;
        }
        tot[b] = total ? total[b] : run - first;
    }
    __syncthreads();
}

// scan over the buckets, by ONE wave: tot [B] becomes its exclusive prefix, which is `offsets` (stored where the pointer is given)
static __device__ __forceinline__ void route_bucket_scan(int* tot, int B, int lane, int32_t* __restrict__ offsets) {
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
        if (offsets) offsets[b] = run;         // B = E + 1 entries: offsets[E] = the pairs some expert serves
        run += c;
    }
}

// place: the wave walks its range again in order, 64 pairs at a time; the sorted row of a pair is tot[b] + cnt[w][b] + its rank in its
// group, the lanes of the step with its bucket
template <typename IdT, typename W>
static __device__ __forceinline__ void route_place(const IdT* ids, const typename RouteWeight<W>::type* weights, const RouteWave& r,
                                                   int k, int E, int nbits, int* cnt, const int* tot, int32_t* __restrict__ perm,
                                                   int32_t* __restrict__ rows, float* __restrict__ row_weight,
                                                   int32_t* __restrict__ pos) {
    const int lane = threadIdx.x & 63;
    int* mine = cnt + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (E + 1);
    for (int c = r.begin; c < r.end; c += 64) {
        const int p = c + lane;
        const bool valid = p < r.end;
        const int b = c == r.begin ? r.b_first : (valid ? route_bucket(ids, p, E) : 0);
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

// count / scan / place of the chunk [lo, hi) on the whole workgroup (kRouteThreads threads, every one of them calls it;
// route_lds_bytes(E) of dynamic LDS).  ids and weights carry no __restrict__ here: the gating kernels (moe_gate.hip) write them, in the
// same launch before a barrier or in an earlier one.
//   total null   the chunk is all there is: the buckets' totals are the workgroup's own counts, `offsets` is stored.
//   total given  the multi-workgroup form: total [B] holds every bucket's count over ALL chunks and before [B] the bucket's count over
//                the chunks in front of this one (moe_route_wide.hip's second launch wrote both).  The sorted row of a pair is then
//                tot[b] + before[b] + cnt[w][b] + rank; `before` is what the waves' prefix starts at.  `offsets` is stored by the
//                workgroup that is given the pointer: every workgroup computes the same values from `total`, one writes them.
template <typename IdT, typename W>
static __device__ __forceinline__ void route_sort_chunk(const IdT* ids, const typename RouteWeight<W>::type* weights, int lo, int hi,
                                                        int k, int E, int nbits, const int* __restrict__ total,
                                                        const int* __restrict__ before, int32_t* __restrict__ offsets,
                                                        int32_t* __restrict__ perm, int32_t* __restrict__ rows,
                                                        float* __restrict__ row_weight, int32_t* __restrict__ pos) {
    extern __shared__ int route_lds[];
    const int B = E + 1;
    int* cnt = route_lds;                      // [16][B]
    int* tot = route_lds + kRouteWaves * B;    // [B]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RouteWave r = route_wave_range(ids, lo, hi, E, w, lane);

    route_count(ids, r, E, cnt);
    route_wave_prefix(cnt, tot, B, before, total);
    if (w == 0) route_bucket_scan(tot, B, lane, offsets);
    __syncthreads();
    route_place<IdT, W>(ids, weights, r, k, E, nbits, cnt, tot, perm, rows, row_weight, pos);
}

// the one-workgroup kernels: one chunk, all P pairs, base 0
template <typename IdT, typename W>
static __device__ __forceinline__ void route_sort_phases(const IdT* ids, const typename RouteWeight<W>::type* weights, int P,
                                                         int k, int E, int nbits, int32_t* __restrict__ offsets,
                                                         int32_t* __restrict__ perm, int32_t* __restrict__ rows,
                                                         float* __restrict__ row_weight, int32_t* __restrict__ pos) {
    route_sort_chunk<IdT, W>(ids, weights, 0, P, k, E, nbits, nullptr, nullptr, offsets, perm, rows, row_weight, pos);
}

// the first launch of the multi-workgroup form on one chunk: its pairs counted per bucket, all B counts to hist_row [B] (plain vector
// stores; every word is written, a bucket without a pair as 0)
template <typename IdT>
static __device__ __forceinline__ void route_count_chunk(const IdT* ids, int lo, int hi, int E, int* __restrict__ hist_row) {
    extern __shared__ int route_lds[];
    const int B = E + 1;
    int* cnt = route_lds;
    int* tot = route_lds + kRouteWaves * B;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RouteWave r = route_wave_range(ids, lo, hi, E, w, lane);
    route_count(ids, r, E, cnt);
    route_wave_prefix(cnt, tot, B, nullptr, nullptr);
    for (int b = threadIdx.x; b < B; b += kRouteThreads) hist_row[b] = tot[b];      // the thread that wrote tot[b] reads it
}

// the pairs of chunk c, chunk_tokens tokens each: [lo, hi) (T k < 2^27, and the tokens are clipped before they are multiplied)
static __device__ __forceinline__ void route_chunk_pairs(int c, int chunk_tokens, int T, int k, int* lo, int* hi) {
    const int t0 = c * chunk_tokens;                                            // c < C = ceil(T / chunk_tokens): t0 < T
    *lo = t0 * k;
    *hi = (chunk_tokens < T - t0 ? t0 + chunk_tokens : T) * k;
}

// dynamic LDS of a launch that runs route_sort_chunk or route_count_chunk: cnt [16][E + 1] and tot [E + 1]
static inline size_t route_lds_bytes(int E) { return (size_t)(kRouteWaves + 1) * (size_t)(E + 1) * sizeof(int); }
// bits of the largest bucket number, E
static inline int route_bucket_bits(int E) {
    int nbits = 0;
    while ((E >> nbits) != 0) ++nbits;
    return nbits;
}

}  // namespace flute_amd
