// The block form of the grouped qgemm (qgemm_grouped_blocks.h: qgemm_block2.h behind its grouped front end) for num_bits = 2:
// plain and weighted, TileP 32 / 64, f16 / bf16 - 8 instantiations.
#include "qgemm_grouped_blocks.h"
namespace flute_amd {
int qgemm_grouped_blocks_unit_b2(const GroupedForward& g, hipStream_t stream) {
    if (g.mode == FLUTE_GROUPED_WEIGHTED) return qgemm_grouped_blocks_launch<2, 2>(g, stream);
    return qgemm_grouped_blocks_launch<2, 1>(g, stream);
}
}  // namespace flute_amd
