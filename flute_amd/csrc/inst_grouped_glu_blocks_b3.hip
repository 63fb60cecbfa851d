// The block form of the fused SwiGLU grouped launch for num_bits = 3 (qgemm_grouped_blocks.h: qgemm_block3.h's GM = 3 member): TileP 32
// (3-bit layers have no other), f16 / bf16 - 2 instantiations.
#include "qgemm_grouped_blocks.h"
namespace flute_amd {
int qgemm_grouped_glu_blocks_unit_b3(const GroupedForward& g, hipStream_t stream) {
    return g.dtype == 0 ? qgemm_grouped_glu_w3_blocks_launch<F16>(g, stream) : qgemm_grouped_glu_w3_blocks_launch<BF16>(g, stream);
}
}  // namespace flute_amd
