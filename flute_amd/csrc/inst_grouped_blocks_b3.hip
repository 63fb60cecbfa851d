// The block form of the grouped qgemm for num_bits = 3 (qgemm_grouped_blocks.h: qgemm_block3.h behind its grouped front end): plain and
// weighted, TileP 32 (3-bit layers have no other), f16 / bf16 - 4 instantiations.
#include "qgemm_grouped_blocks.h"
namespace flute_amd {
int qgemm_grouped_blocks_unit_b3(const GroupedForward& g, hipStream_t stream) {
    if (g.mode == FLUTE_GROUPED_WEIGHTED) return qgemm_grouped_w3_blocks_launch<2>(g, stream);
    return qgemm_grouped_w3_blocks_launch<1>(g, stream);
}
}  // namespace flute_amd
