// The routing of a mixture-of-experts step over MANY workgroups, for prefill and training token counts: the stable counting sort of
// moe_route.hip in three plain launches (include/flute_amd.h, flute_moe_route_wide / flute_moe_gate_route_wide).  Every output is bit
// for bit the one-workgroup kernels': a stable sort by bucket has one answer, and the device code is theirs (moe_route_sort.h).
//
// Chunk c owns chunk_tokens consecutive tokens, [c chunk_tokens, (c + 1) chunk_tokens) cut at T: one contiguous range of pairs.
// C = ceil(T / chunk_tokens) chunks, one workgroup of 16 waves per chunk; inside the chunk the waves own contiguous sub-ranges rounded
// up to 64 pairs, as in the one-workgroup sort.  B = E + 1 buckets, bucket E = every id outside [0, E).
//   count  grid C   moe_route_count_kernel: the workgroup counts its chunk's pairs per bucket in LDS and writes all B counts to
//                   hist[c][0 .. B).  Gated (moe_gate_count_kernel, moe_gate.hip, next to gate_token): wave w first gates the chunk's
//                   tokens w, w + 16, ... and writes ids / weights, then a workgroup fence and a barrier, then the same count - the
//                   workgroup reads back only what it wrote itself.
//   scan   grid ceil(B / 64)   moe_route_scan_kernel: each bucket's column of hist becomes its exclusive prefix over the chunks, in
//                   place, and the bucket's total goes to total[b].  A workgroup takes 64 neighbouring buckets, lane = bucket, and its
//                   16 waves split the chunks: each sums its stretch, the 16 partial sums meet in LDS, each walks its stretch again.
//   place  grid C   moe_route_place_kernel: every workgroup loads total into LDS and scans it over the buckets (wave 0; workgroup 0
//                   stores `offsets`), counts its chunk per wave again with the prefix started at hist[c][b], and places with the
//                   ballot-per-bit group search: row = tot[b] + hist[c][b] + cnt[w][b] + rank.
// The workspace is hist [C][B] then total [B], int32.  hist is chunk-major: the count's stores and the place's loads, both grid C, are
// then contiguous rows, and the scan - the small launch - reads a column with stride B, but 64 neighbouring buckets by one wave, so its
// loads are contiguous too, 256 B of a row at a time.  Bucket-major would make the two large launches strided and the scan's
// lanes run along the chunks.
// No workgroup waits on another inside a launch: the kernel boundaries are the only ordering between workgroups.  No arrival counter,
// no atomics on global memory, plain vector stores.  Every word of the workspace a launch reads was written by an earlier launch of
// the same call: nothing assumes zeros, or anything else, from the caller.
#include "kernels.h"
#include "moe_route_sort.h"
#include "../../include/flute_amd.h"

namespace flute_amd {

constexpr int kScanBuckets = 64;                // buckets per workgroup of the scan: one per lane

template <typename IdT>
__global__ __launch_bounds__(kRouteThreads) void moe_route_count_kernel(const IdT* __restrict__ ids, int T, int k, int E,
                                                                        int chunk_tokens, int32_t* __restrict__ hist) {
    int lo, hi;
    route_chunk_pairs(blockIdx.x, chunk_tokens, T, k, &lo, &hi);
    route_count_chunk<IdT>(ids, lo, hi, E, hist + (size_t)blockIdx.x * (E + 1));
}

__global__ __launch_bounds__(kRouteThreads) void moe_route_scan_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ total,
                                                                       int C, int B) {
    __shared__ int part[kRouteWaves][kScanBuckets];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * kScanBuckets + lane;
    const int per = (C + kRouteWaves - 1) / kRouteWaves;
    const int c0 = min(w * per, C), c1 = min(c0 + per, C);
    int32_t* col = hist + b;                    // C B <= FLUTE_MOE_ROUTE_MAX_CHUNKS * 1025: an int index
    int sum = 0;
    if (b < B)
        for (int c = c0; c < c1; ++c) sum += col[c * B];
    part[w][lane] = sum;
    __syncthreads();
    int run = 0;
#pragma unroll
    for (int v = 0; v < kRouteWaves; ++v) run += v < w ? part[v][lane] : 0;
    if (b < B) {
        for (int c = c0; c < c1; ++c) {
            const int n = col[c * B];
            col[c * B] = run;
            run += n;
        }
        if (w == kRouteWaves - 1) total[b] = run;                   // the last stretch ends at the bucket's count over all chunks
    }
}

template <typename IdT, typename W>
__global__ __launch_bounds__(kRouteThreads) void moe_route_place_kernel(const IdT* __restrict__ ids,
                                                                        const typename RouteWeight<W>::type* __restrict__ weights,
                                                                        int T, int k, int E, int nbits, int chunk_tokens,
                                                                        const int32_t* __restrict__ hist,
                                                                        const int32_t* __restrict__ total,
                                                                        int32_t* __restrict__ offsets, int32_t* __restrict__ perm,
                                                                        int32_t* __restrict__ rows, float* __restrict__ row_weight,
                                                                        int32_t* __restrict__ pos) {
    int lo, hi;
    route_chunk_pairs(blockIdx.x, chunk_tokens, T, k, &lo, &hi);
    route_sort_chunk<IdT, W>(ids, weights, lo, hi, k, E, nbits, total, hist + (size_t)blockIdx.x * (E + 1),
                             blockIdx.x == 0 ? offsets : nullptr, perm, rows, row_weight, pos);
}

static bool route_raise_lds(const void* fn, size_t lds) {
    return lds <= 65536 || hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

// the second and third launch, which the gated and the ungated form share
template <typename IdT>
static int route_scan_place(int weight_dtype, int T, int k, int E, int C, int chunk_tokens, const IdT* ids, const void* weights,
                            int32_t* hist, int32_t* total, int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight,
                            int32_t* pos, hipStream_t stream) {
    const int B = E + 1;
    const size_t lds = route_lds_bytes(E);
    const int nbits = route_bucket_bits(E);
    hipLaunchKernelGGL(moe_route_scan_kernel, dim3((B + kScanBuckets - 1) / kScanBuckets), dim3(kRouteThreads), 0, stream, hist, total,
                       C, B);
#define FLUTE_PLACE(WT)                                                                                                  \
    {                                                                                                                    \
        auto kern = moe_route_place_kernel<IdT, WT>;                                                                     \
        if (!route_raise_lds((const void*)kern, lds)) return FLUTE_ERR_LAUNCH;                                           \
        hipLaunchKernelGGL(kern, dim3(C), dim3(kRouteThreads), lds, stream, ids,                                         \
                           reinterpret_cast<const typename RouteWeight<WT>::type*>(weights), T, k, E, nbits, chunk_tokens, \
                           hist, total, offsets, perm, rows, row_weight, pos);                                           \
    }
    if (weight_dtype == FLUTE_F16) FLUTE_PLACE(F16)
    else if (weight_dtype == FLUTE_BF16) FLUTE_PLACE(BF16)
    else FLUTE_PLACE(float)
#undef FLUTE_PLACE
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

template <typename IdT>
static int route_wide(int weight_dtype, int T, int k, int E, int C, int chunk_tokens, const void* ids, const void* weights,
                      int32_t* hist, int32_t* total, int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight,
                      int32_t* pos, hipStream_t stream) {
    auto kern = moe_route_count_kernel<IdT>;
    const size_t lds = route_lds_bytes(E);
    if (!route_raise_lds((const void*)kern, lds)) return FLUTE_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(C), dim3(kRouteThreads), lds, stream, reinterpret_cast<const IdT*>(ids), T, k, E, chunk_tokens,
                       hist);
    return route_scan_place<IdT>(weight_dtype, T, k, E, C, chunk_tokens, reinterpret_cast<const IdT*>(ids), weights, hist, total,
                                 offsets, perm, rows, row_weight, pos, stream);
}

int moe_route_wide_dispatch(int id_dtype, int weight_dtype, int T, int k, int E, int chunk_tokens, const void* ids,
                            const void* weights, int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos,
                            void* workspace, hipStream_t stream) {
    const int C = (T + chunk_tokens - 1) / chunk_tokens;
    int32_t* hist = reinterpret_cast<int32_t*>(workspace);
    int32_t* total = hist + (size_t)C * (E + 1);
    if (id_dtype == FLUTE_I32)
        return route_wide<int32_t>(weight_dtype, T, k, E, C, chunk_tokens, ids, weights, hist, total, offsets, perm, rows, row_weight,
                                   pos, stream);
    return route_wide<int64_t>(weight_dtype, T, k, E, C, chunk_tokens, ids, weights, hist, total, offsets, perm, rows, row_weight,
                               pos, stream);
}

int moe_gate_route_wide_dispatch(int logit_dtype, int T, int E, int k, const GateGroups* groups, int scoring, int renormalize,
                                 float scale, int chunk_tokens, const void* logits, const float* bias, int32_t* ids, float* weights,
                                 int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* workspace,
                                 hipStream_t stream) {
    const int C = (T + chunk_tokens - 1) / chunk_tokens;
    int32_t* hist = reinterpret_cast<int32_t*>(workspace);
    int32_t* total = hist + (size_t)C * (E + 1);
    const int rc = moe_gate_count_dispatch(logit_dtype, T, E, k, groups, scoring, renormalize, scale, chunk_tokens, logits, bias, ids,
                                           weights, hist, stream);
    if (rc) return rc;
    return route_scan_place<int32_t>(FLUTE_F32, T, k, E, C, chunk_tokens, ids, weights, hist, total, offsets, perm, rows, row_weight,
                                     pos, stream);
}

}  // namespace flute_amd
