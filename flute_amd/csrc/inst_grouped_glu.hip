// The grouped GLU launch (qgemm_grouped_fused.h, GLU form): 18 instantiations, as qgemm_grouped.hip's matrix.
#include "qgemm_grouped_fused.h"
namespace flute_amd {
int qgemm_grouped_glu_dispatch(int dtype, int num_bits, int tile_p, int lg, int E, int R, int Tsrc, int N, int K, int P,
                               const void* Xsrc, const void* rows, const void* offsets, const void* Qg, const void* Sg,
                               const void* QM2g, const void* Qu, const void* Su, const void* QM2u, void* H, int num_sms,
                               hipStream_t stream) {
    GroupedFusedArgs a{};
    a.X = reinterpret_cast<const uint16_t*>(Xsrc);
    a.rows = reinterpret_cast<const int*>(rows);
    a.offsets = reinterpret_cast<const int*>(offsets);
    a.Q[0] = reinterpret_cast<const uint32_t*>(Qg); a.Q[1] = reinterpret_cast<const uint32_t*>(Qu);
    a.S[0] = reinterpret_cast<const uint16_t*>(Sg); a.S[1] = reinterpret_cast<const uint16_t*>(Su);
    a.QM2[0] = reinterpret_cast<const uint32_t*>(QM2g); a.QM2[1] = reinterpret_cast<const uint32_t*>(QM2u);
    a.row_weight = nullptr;
    a.Y = reinterpret_cast<uint16_t*>(H);
    a.R = R; a.Tsrc = Tsrc; a.N = N; a.K = K; a.P = P; a.lg = lg; a.E = E;
    return qgemm_grouped_fused_launch<true>(dtype, num_bits, tile_p, lg, a, num_sms, stream);
}
}  // namespace flute_amd
