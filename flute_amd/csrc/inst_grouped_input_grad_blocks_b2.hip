// The block form of the grouped input gradient (qgemm_grouped_input_grad_blocks.h), 2 bits: 8 instantiations.
#include "qgemm_grouped_input_grad_blocks.h"
namespace flute_amd {
int qgemm_grouped_input_grad_blocks_unit_b2(const GroupedInputGrad& g, hipStream_t stream) {
    return qgemm_grouped_input_grad_blocks_launch<2>(g, stream);
}
}  // namespace flute_amd
