// Explicit instantiations of the block-tiled prefill kernel (qgemm_block2.h) for num_bits = 4.
#include "kernels.h"
#include "qgemm_block2.h"
namespace flute_amd {
// cfg 4: 256 x 256 block split 1 x 8 over the waves (every weight dequantised once per workgroup); cfg 5: the same on
// 128-row blocks.  (cfg 0..3 were the 2 x 4 split of round 2, removed.)
#define FLUTE_ROW(TP, CFG, RT) \
    if (tile_p == TP && cfg == CFG) return dtype == 0 ? (BlockKernel)qgemm_block2_kernel<F16, TP, RT> : (BlockKernel)qgemm_block2_kernel<BF16, TP, RT>;
BlockKernel block_kernel_b4(int dtype, int tile_p, int cfg) {
    FLUTE_ROW(32, 4, 16) FLUTE_ROW(64, 4, 16) FLUTE_ROW(32, 5, 8) FLUTE_ROW(64, 5, 8)
    return nullptr;
}
}  // namespace flute_amd
