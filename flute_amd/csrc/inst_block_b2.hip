// Explicit instantiations of the block-tiled prefill kernel (qgemm_block2.h) for num_bits = 2.
#include "kernels.h"
#include "qgemm_block2.h"
namespace flute_amd {
// cfg 4: 256 x 256 blocks, cfg 5: 128 x 256 (the 1 x 8 wave split; the 2 x 4 split of qgemm_block.h is 4-bit only)
#define FLUTE_ROW(TP, CFG, RT) \
    if (tile_p == TP && cfg == CFG) return dtype == 0 ? (BlockKernel)qgemm_block2_kernel<F16, TP, RT, 2> : (BlockKernel)qgemm_block2_kernel<BF16, TP, RT, 2>;
BlockKernel block_kernel_b2(int dtype, int tile_p, int cfg) {
    FLUTE_ROW(32, 4, 16) FLUTE_ROW(64, 4, 16) FLUTE_ROW(32, 5, 8) FLUTE_ROW(64, 5, 8)
    return nullptr;
}
}  // namespace flute_amd
