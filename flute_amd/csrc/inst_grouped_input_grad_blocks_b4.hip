// The block form of the grouped input gradient (qgemm_grouped_input_grad_blocks.h), 4 bits: 8 instantiations.
#include "qgemm_grouped_input_grad_blocks.h"
namespace flute_amd {
int qgemm_grouped_input_grad_blocks_dispatch_b4(int dtype, int tile_p, int lg, int E, int R, int N, int K, int P, const void* dY,
                                                const void* offsets, const void* Q, const void* S, const void* QM2,
                                                const void* row_weight, const void* dY2, const void* Q2, const void* S2,
                                                const void* QM22, void* dX, hipStream_t stream) {
    const GroupedIgArgs a = grouped_ig_args(dY, offsets, Q, S, QM2, row_weight, dY2, Q2, S2, QM22, dX, R, N, K, P, lg, E);
    return qgemm_grouped_input_grad_blocks_launch<4>(dtype, tile_p, dY2 != nullptr, a, stream);
}
}  // namespace flute_amd
