// The grouped input gradient (qgemm_grouped_input_grad.h), 2 bits: 8 instantiations.
#include "qgemm_grouped_input_grad.h"
namespace flute_amd {
int qgemm_grouped_input_grad_unit_b2(const GroupedInputGrad& g, hipStream_t stream) {
    return qgemm_grouped_input_grad_launch<2>(g, stream);
}
}  // namespace flute_amd
