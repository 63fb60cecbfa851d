// The weighted grouped qgemm (qgemm_grouped_fused.h, weighted form): 18 instantiations, as qgemm_grouped.hip's matrix.
#include "qgemm_grouped_fused.h"
namespace flute_amd {
int qgemm_grouped_weighted_dispatch(int dtype, int num_bits, int tile_p, int lg, int E, int T, int N, int K, int P,
                                    const void* X, const void* offsets, const void* Q, const void* S, const void* QM2,
                                    const void* row_weight, void* Y, int num_sms, hipStream_t stream) {
    GroupedFusedArgs a{};
    a.X = reinterpret_cast<const uint16_t*>(X);
    a.rows = nullptr;
    a.offsets = reinterpret_cast<const int*>(offsets);
    a.Q[0] = a.Q[1] = reinterpret_cast<const uint32_t*>(Q);
    a.S[0] = a.S[1] = reinterpret_cast<const uint16_t*>(S);
    a.QM2[0] = a.QM2[1] = reinterpret_cast<const uint32_t*>(QM2);
    a.row_weight = reinterpret_cast<const float*>(row_weight);
    a.Y = reinterpret_cast<uint16_t*>(Y);
    a.R = T; a.Tsrc = T; a.N = N; a.K = K; a.P = P; a.lg = lg; a.E = E;
    return qgemm_grouped_fused_launch<false>(dtype, num_bits, tile_p, lg, a, num_sms, stream);
}
}  // namespace flute_amd
