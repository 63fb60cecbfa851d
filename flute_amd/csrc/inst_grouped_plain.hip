// The plain grouped qgemm (qgemm_grouped.h, Plain mode): 18 instantiations.
#include "qgemm_grouped.h"
namespace flute_amd {
int qgemm_grouped_dispatch(int dtype, int num_bits, int tile_p, int lg, int E, int T, int N, int K, int P, const void* X,
                           const void* offsets, const void* Q, const void* S, const void* QM2, void* Y, int num_sms,
                           hipStream_t stream) {
    const GroupedArgs a = grouped_args(X, nullptr, offsets, Q, S, QM2, Q, S, QM2, nullptr, Y, T, T, N, K, P, lg, E);
    return qgemm_grouped_launch<GroupedMode::Plain>(dtype, num_bits, tile_p, a, num_sms, stream);
}
}  // namespace flute_amd
