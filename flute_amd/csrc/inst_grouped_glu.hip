// The grouped GLU launch (qgemm_grouped.h, Glu mode): 18 instantiations.
#include "qgemm_grouped.h"
namespace flute_amd {
int qgemm_grouped_glu_dispatch(int dtype, int num_bits, int tile_p, int lg, int E, int R, int Tsrc, int N, int K, int P,
                               const void* Xsrc, const void* rows, const void* offsets, const void* Qg, const void* Sg,
                               const void* QM2g, const void* Qu, const void* Su, const void* QM2u, void* H, int num_sms,
                               hipStream_t stream) {
    const GroupedArgs a = grouped_args(Xsrc, rows, offsets, Qg, Sg, QM2g, Qu, Su, QM2u, nullptr, H, R, Tsrc, N, K, P, lg, E);
    return qgemm_grouped_launch<GroupedMode::Glu>(dtype, num_bits, tile_p, a, num_sms, stream);
}
}  // namespace flute_amd
