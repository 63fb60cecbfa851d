// Host side of the block form of the grouped qgemm: qgemm_block2.h's 128-row blocks behind a grouped front end (the kernel text and
// the block map are described there), for experts with many rows - prefill and training - where the row form of qgemm_grouped.h
// streams an expert's weights once per 32 rows.  Plain and weighted modes (flute_qgemm_grouped_ex / _weighted_ex with the block form)
// and the SwiGLU mode behind its own entry (flute_qgemm_grouped_glu_blocks), 4 and 2 bits; 3 bits stay on the row form.
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

// The LDS of a grouped block launch, every mode: pair table + three activation stages + per wave: two scale blocks and a sink (as
// plan_block sizes the dense launch).  The SwiGLU mode restages the one pair table between its two K passes and needs no more.
template <int BITS>
constexpr size_t grouped_blocks_lds_bytes() {
    return (size_t)((128 << (2 * BITS)) + BLK_STAGES * (kGroupedBlockRows / 16) * 2 * 1024 + 8 * 3 * 1024);
}

// What every mode's argument struct shares, from the launch's named operands (GM = 3: Q / S / QM2 are the gate stack's, N is F).
inline void grouped_block_args(GroupedBlockArgs& a, const GroupedForward& g) {
    a.A = g.X; a.Q = reinterpret_cast<const uint32_t*>(g.Q[0]); a.D = g.Y; a.S = g.S[0];
    a.QM2 = reinterpret_cast<const uint32_t*>(g.QM2[0]);
    a.M = g.R; a.N = g.N; a.K = g.K; a.G = g.K >> g.lg; a.lg = g.lg;
    a.tiles_m = (int)grouped_blocks_row_blocks(g.E, g.R); a.tiles_n = g.N / 256;
    a.splitk = 1; a.k_per_split = g.K;
    a.order = FLUTE_GROUPED_BLOCKS_ORDER;
    a.offsets = reinterpret_cast<const int*>(g.offsets);
    a.row_weight = nullptr;
    a.E = g.E; a.P = g.P;
}

// The launch of one resolved kernel: the grid follows from (E, R, N) alone.
template <int BITS, typename Args>
int grouped_blocks_enqueue(void (*k)(const Args), Args& a, hipStream_t stream) {
    if (!k) return FLUTE_ERR_SHAPE;
    const size_t lds = grouped_blocks_lds_bytes<BITS>();
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

// One launch: GM = 1 plain, 2 weighted.
template <int BITS, int GM>
int qgemm_grouped_blocks_launch(const GroupedForward& g, hipStream_t stream) {
    const int dtype = g.dtype, tile_p = g.tile_p;
    GroupedBlockArgs a{};
    grouped_block_args(a, g);
    a.row_weight = GM == 2 ? g.row_weight : nullptr;
    typedef void (*Kernel)(const GroupedBlockArgs);
    Kernel k = nullptr;
    if (tile_p == 32) k = dtype == 0 ? (Kernel)qgemm_block2_kernel<F16, 32, 8, BITS, GM> : (Kernel)qgemm_block2_kernel<BF16, 32, 8, BITS, GM>;
    else if (tile_p == 64) k = dtype == 0 ? (Kernel)qgemm_block2_kernel<F16, 64, 8, BITS, GM> : (Kernel)qgemm_block2_kernel<BF16, 64, 8, BITS, GM>;
    return grouped_blocks_enqueue<BITS>(k, a, stream);
}

// The SwiGLU launch (GM = 3): both stacks, the row index and the rows of Xsrc beside the shared arguments; the same grid.
template <int BITS>
int qgemm_grouped_glu_blocks_launch(const GroupedForward& g, hipStream_t stream) {
    const int dtype = g.dtype, tile_p = g.tile_p;
    GroupedGluBlockArgs a{};
    grouped_block_args(a, g);
    a.Q_up = reinterpret_cast<const uint32_t*>(g.Q[1]); a.S_up = g.S[1];
    a.QM2_up = reinterpret_cast<const uint32_t*>(g.QM2[1]);
    a.rows = reinterpret_cast<const int*>(g.rows);
    a.Tsrc = g.Tsrc;
    typedef void (*Kernel)(const GroupedGluBlockArgs);
    Kernel k = nullptr;
    if (tile_p == 32) k = dtype == 0 ? (Kernel)qgemm_block2_kernel<F16, 32, 8, BITS, 3> : (Kernel)qgemm_block2_kernel<BF16, 32, 8, BITS, 3>;
    else if (tile_p == 64) k = dtype == 0 ? (Kernel)qgemm_block2_kernel<F16, 64, 8, BITS, 3> : (Kernel)qgemm_block2_kernel<BF16, 64, 8, BITS, 3>;
    return grouped_blocks_enqueue<BITS>(k, a, stream);
}

}  // namespace flute_amd
