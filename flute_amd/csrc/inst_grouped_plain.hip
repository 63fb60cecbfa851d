// The plain grouped qgemm (qgemm_grouped.h, Plain mode): 18 instantiations.
#include "qgemm_grouped.h"
namespace flute_amd {
int qgemm_grouped_plain_unit(const GroupedForward& g, hipStream_t stream) {
    return qgemm_grouped_launch<GroupedMode::Plain>(g, stream);
}
}  // namespace flute_amd
