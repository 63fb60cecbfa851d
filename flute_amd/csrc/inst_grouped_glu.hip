// The grouped GLU launch (qgemm_grouped.h, Glu mode): 18 instantiations.
#include "qgemm_grouped.h"
namespace flute_amd {
int qgemm_grouped_glu_unit(const GroupedForward& g, hipStream_t stream) {
    return qgemm_grouped_launch<GroupedMode::Glu>(g, stream);
}
}  // namespace flute_amd
