// Explicit instantiations of the LDS-DMA staged MFMA kernel (qgemm_tile.h) for num_bits = 3: R lanes share a
// unit, MT 16-row tiles per wave, (16 / R) * MT <= 16 accumulator tiles.
#include "kernels.h"
#include "qgemm_tile.h"
namespace flute_amd {
#define FLUTE_ROW(TP, R, MT) \
    if (tile_p == TP && r == R && mt == MT) return dtype == 0 ? (QGemmKernel)qgemm_tile_kernel<F16, 3, TP, R, MT> : (QGemmKernel)qgemm_tile_kernel<BF16, 3, TP, R, MT>;
QGemmKernel tile_kernel_b3(int dtype, int tile_p, int r, int mt) {
    FLUTE_ROW(32, 1, 1)
    return nullptr;
}
}  // namespace flute_amd
