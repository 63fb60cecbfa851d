// The weighted grouped qgemm (qgemm_grouped.h, Weighted mode): 18 instantiations.
#include "qgemm_grouped.h"
namespace flute_amd {
int qgemm_grouped_weighted_unit(const GroupedForward& g, hipStream_t stream) {
    return qgemm_grouped_launch<GroupedMode::Weighted>(g, stream);
}
}  // namespace flute_amd
