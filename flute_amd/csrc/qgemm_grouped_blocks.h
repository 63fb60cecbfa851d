// Host side of the block form of the grouped qgemm: qgemm_block2.h's 128-row blocks behind a grouped front end (the kernel text and
// the block map are described there), for experts with many rows - prefill and training - where the row form of qgemm_grouped.h
// streams an expert's weights once per 32 rows.  Plain and weighted modes, 4 and 2 bits; the SwiGLU mode and 3 bits stay on the row form.
#pragma once
#include "../../include/flute_amd.h"
#include "kernels.h"
#include "qgemm_block2.h"

// The order of the block map: 1 - the column block is the fast index of blockIdx, so the workgroups in flight share a row block's
// activations and spread over the column blocks of one expert; 0 (development builds, EXTRA=-DFLUTE_GROUPED_BLOCKS_ORDER=0) - the row
// block is.  Measured (W4G64 fp16, us per launch, order 0 -> 1, two alternating processes each, tools/grouped_bench.py's method;
// profiles/grouped_moe_prefill_block_order.jsonl): Mixtral gate / up 4096 rows 646 -> 592, 8192 rows 1149 -> 1056; down 4096 rows
// 662 -> 639, 1024 rows 215 -> 211; E 64 2048 x 2048 8192 rows 137 -> 134.
#ifndef FLUTE_GROUPED_BLOCKS_ORDER
#define FLUTE_GROUPED_BLOCKS_ORDER 1
#endif

namespace flute_amd {

// One launch: GM = 1 plain, 2 weighted.  The grid follows from (E, T, N) alone.
template <int BITS, int GM>
int qgemm_grouped_blocks_launch(const GroupedForward& g, hipStream_t stream) {
    const int dtype = g.dtype, tile_p = g.tile_p;
    GroupedBlockArgs a{};
    a.A = g.X; a.Q = reinterpret_cast<const uint32_t*>(g.Q[0]); a.D = g.Y; a.S = g.S[0];
    a.QM2 = reinterpret_cast<const uint32_t*>(g.QM2[0]);
    a.M = g.R; a.N = g.N; a.K = g.K; a.G = g.K >> g.lg; a.lg = g.lg;
    a.tiles_m = (int)grouped_blocks_row_blocks(g.E, g.R); a.tiles_n = g.N / 256;
    a.splitk = 1; a.k_per_split = g.K;
    a.order = FLUTE_GROUPED_BLOCKS_ORDER;
    a.offsets = reinterpret_cast<const int*>(g.offsets);
    a.row_weight = GM == 2 ? g.row_weight : nullptr;
    a.E = g.E; a.P = g.P;
    typedef void (*Kernel)(const GroupedBlockArgs);
    Kernel k = nullptr;
    if (tile_p == 32) k = dtype == 0 ? (Kernel)qgemm_block2_kernel<F16, 32, 8, BITS, GM> : (Kernel)qgemm_block2_kernel<BF16, 32, 8, BITS, GM>;
    else if (tile_p == 64) k = dtype == 0 ? (Kernel)qgemm_block2_kernel<F16, 64, 8, BITS, GM> : (Kernel)qgemm_block2_kernel<BF16, 64, 8, BITS, GM>;
    if (!k) return FLUTE_ERR_SHAPE;
    // pair table + three activation stages + per wave: two scale blocks and a sink (as plan_block sizes the dense launch)
    const size_t lds = (size_t)((128 << (2 * BITS)) + 3 * (kGroupedBlockRows / 16) * 2 * 1024 + 8 * 3 * 1024);
    // (above 64 KB; the attribute is per device and setting it is no stream operation: asked for at every launch, as moe_route.hip does)
    if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return FLUTE_ERR_LAUNCH;
    }
    void* kargs[] = {&a};
    if (hipLaunchKernel((const void*)k, dim3((unsigned)((long long)a.tiles_m * a.tiles_n)), dim3(512), kargs, lds, stream) != hipSuccess) {
        (void)hipGetLastError();
        return FLUTE_ERR_LAUNCH;
    }
    return FLUTE_OK;
}

}  // namespace flute_amd
