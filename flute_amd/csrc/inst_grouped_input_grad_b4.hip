// The grouped input gradient (qgemm_grouped_input_grad.h), 4 bits: 8 instantiations.
#include "qgemm_grouped_input_grad.h"
namespace flute_amd {
int qgemm_grouped_input_grad_unit_b4(const GroupedInputGrad& g, hipStream_t stream) {
    return qgemm_grouped_input_grad_launch<4>(g, stream);
}
}  // namespace flute_amd
