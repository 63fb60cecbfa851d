// The 256-row block form of the grouped input gradient for 3-bit stacks (qgemm_grouped_input_grad_w3_blocks256.h): TileP 32 (3-bit
// layers have no other) x f16 / bf16 x single / pair - 4 instantiations.
#include "qgemm_grouped_input_grad_w3_blocks256.h"
namespace flute_amd {
int qgemm_grouped_input_grad_blocks256_unit_b3(const GroupedInputGrad& g, hipStream_t stream) {
    return qgemm_grouped_input_grad_w3_blocks256_launch(g, stream);
}
}  // namespace flute_amd
