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
// its range), but a prefill-sized P is sorted by 1024 threads: the multi-workgroup form for those is moe_route_wide.hip.
// The device code of the sort is moe_route_sort.h (moe_gate.hip runs the same phases behind its gating, moe_route_wide.hip
// one chunk of the pairs per workgroup).
#include "kernels.h"
#include "moe_route_sort.h"
#include "../../include/flute_amd.h"

namespace flute_amd {

template <typename IdT, typename W>
__global__ __launch_bounds__(kRouteThreads) void moe_route_kernel(const IdT* __restrict__ ids,
                                                                  const typename RouteWeight<W>::type* __restrict__ weights,
                                                                  int P, int k, int E, int nbits,
                                                                  int32_t* __restrict__ offsets, int32_t* __restrict__ perm,
                                                                  int32_t* __restrict__ rows, float* __restrict__ row_weight,
                                                                  int32_t* __restrict__ pos) {
    route_sort_phases<IdT, W>(ids, weights, P, k, E, nbits, offsets, perm, rows, row_weight, pos);
}

int moe_route_dispatch(int id_dtype, int weight_dtype, int P, int k, int E, const void* ids, const void* weights,
                       int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos,
                       hipStream_t stream) {
    const size_t lds = route_lds_bytes(E);
    const int nbits = route_bucket_bits(E);
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
