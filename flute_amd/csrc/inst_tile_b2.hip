// Explicit instantiations of the LDS-DMA staged MFMA kernel (qgemm_tile.h) for num_bits = 2: R lanes share a
// unit, MT 16-row tiles per wave, (8 / R) * MT <= 16 accumulator tiles.
#include "kernels.h"
#include "qgemm_tile.h"
namespace flute_amd {
#define FLUTE_ROW(TP, R, MT) \
    if (tile_p == TP && r == R && mt == MT) return dtype == 0 ? (QGemmKernel)qgemm_tile_kernel<F16, 2, TP, R, MT> : (QGemmKernel)qgemm_tile_kernel<BF16, 2, TP, R, MT>;
QGemmKernel tile_kernel_b2(int dtype, int tile_p, int r, int mt) {
    FLUTE_ROW(32, 1, 1) FLUTE_ROW(32, 2, 1) FLUTE_ROW(32, 4, 1) FLUTE_ROW(32, 1, 2) FLUTE_ROW(32, 2, 2) FLUTE_ROW(32, 2, 4)
    FLUTE_ROW(64, 1, 1) FLUTE_ROW(64, 2, 1) FLUTE_ROW(64, 4, 1) FLUTE_ROW(64, 1, 2) FLUTE_ROW(64, 2, 2) FLUTE_ROW(64, 2, 4)
    return nullptr;
}
}  // namespace flute_amd
