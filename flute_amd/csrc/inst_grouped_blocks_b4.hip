// The block form of the grouped qgemm (qgemm_grouped_blocks.h: qgemm_block2.h behind its grouped front end) for num_bits = 4:
// plain and weighted, TileP 32 / 64, f16 / bf16 - 8 instantiations.
#include "qgemm_grouped_blocks.h"
namespace flute_amd {
int qgemm_grouped_blocks_dispatch_b4(int weighted, int dtype, int tile_p, int lg, int E, int T, int N, int K, int P, const void* X,
                                     const void* offsets, const void* Q, const void* S, const void* QM2, const void* row_weight,
                                     void* Y, hipStream_t stream) {
    if (weighted)
        return qgemm_grouped_blocks_launch<4, 2>(dtype, tile_p, lg, E, T, N, K, P, X, offsets, Q, S, QM2, row_weight, Y, stream);
    return qgemm_grouped_blocks_launch<4, 1>(dtype, tile_p, lg, E, T, N, K, P, X, offsets, Q, S, QM2, nullptr, Y, stream);
}
}  // namespace flute_amd
