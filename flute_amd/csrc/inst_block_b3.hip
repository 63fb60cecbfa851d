// Explicit instantiations of the block-tiled prefill kernel for num_bits = 3 (qgemm_block3.h; TileP = 32 only,
// like every 3-bit template).
#include "kernels.h"
#include "qgemm_block3.h"
namespace flute_amd {
#define FLUTE_ROW(CFG, RT) \
    if (tile_p == 32 && cfg == CFG) return dtype == 0 ? (BlockKernel)qgemm_block3_kernel<F16, RT> : (BlockKernel)qgemm_block3_kernel<BF16, RT>;
BlockKernel block_kernel_b3(int dtype, int tile_p, int cfg) {
    FLUTE_ROW(4, 16) FLUTE_ROW(5, 8)           // cfg 4: 256 x 256 blocks (the second / third plane pieces of waves 6, 7 in LDS); cfg 5: 128 x 256 blocks
    FLUTE_ROW(9, 1) FLUTE_ROW(10, 2) FLUTE_ROW(12, 4)      // cfg 8 + RT: skinny blocks of RT = 1, 2, 4 row tiles for small batches (launched with a grid K split)
    return nullptr;
}
}  // namespace flute_amd
