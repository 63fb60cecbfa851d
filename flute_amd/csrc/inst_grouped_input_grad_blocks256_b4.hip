// The 256-row block form of the grouped input gradient (qgemm_grouped_input_grad_blocks256.h), 4 bits: TileP 32 / 64 x f16 / bf16 x
// single / pair - 8 instantiations.
#include "qgemm_grouped_input_grad_blocks256.h"
namespace flute_amd {
int qgemm_grouped_input_grad_blocks256_unit_b4(const GroupedInputGrad& g, hipStream_t stream) {
    return qgemm_grouped_input_grad_blocks256_launch<4>(g, stream);
}
}  // namespace flute_amd
