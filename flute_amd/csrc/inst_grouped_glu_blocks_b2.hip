// The block form of the fused SwiGLU grouped launch (qgemm_grouped_blocks.h: qgemm_block2.h's GM = 3 member) for num_bits = 2:
// TileP 32 / 64, f16 / bf16 - 4 instantiations.
#include "qgemm_grouped_blocks.h"
namespace flute_amd {
int qgemm_grouped_glu_blocks_unit_b2(const GroupedForward& g, hipStream_t stream) {
    return qgemm_grouped_glu_blocks_launch<2>(g, stream);
}
}  // namespace flute_amd
