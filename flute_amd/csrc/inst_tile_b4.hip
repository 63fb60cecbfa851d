// Explicit instantiations of the LDS-DMA staged MFMA kernel (qgemm_tile.h) for num_bits = 4: R lanes share a
// unit, MT 16-row tiles per wave, (4 / R) * MT <= 16 accumulator tiles; SW slabs per wave.
#include "kernels.h"
#include "qgemm_tile.h"
namespace flute_amd {
#define FLUTE_ROW(TP, R, MT, SW) \
    if (tile_p == TP && r == R && mt == MT && sw == SW) return dtype == 0 ? (QGemmKernel)qgemm_tile_kernel<F16, 4, TP, R, MT, SW> : (QGemmKernel)qgemm_tile_kernel<BF16, 4, TP, R, MT, SW>;
// two slabs per wave at MT = 4: fp16 only (the bf16 path keeps a second accumulator set)
#define FLUTE_ROW_F16(TP, R, MT, SW) \
    if (tile_p == TP && r == R && mt == MT && sw == SW && dtype == 0) return (QGemmKernel)qgemm_tile_kernel<F16, 4, TP, R, MT, SW>;
QGemmKernel tile_kernel_b4(int dtype, int tile_p, int r, int mt, int sw) {
    FLUTE_ROW(32, 1, 1, 2) FLUTE_ROW(64, 1, 1, 2) FLUTE_ROW(32, 1, 2, 2) FLUTE_ROW(64, 1, 2, 2) FLUTE_ROW_F16(32, 1, 4, 2) FLUTE_ROW_F16(64, 1, 4, 2)
    FLUTE_ROW(32, 1, 1, 1) FLUTE_ROW(32, 2, 1, 1) FLUTE_ROW(32, 4, 1, 1) FLUTE_ROW(32, 1, 2, 1) FLUTE_ROW(32, 2, 2, 1) FLUTE_ROW(32, 1, 4, 1) FLUTE_ROW(32, 2, 4, 1)
    FLUTE_ROW(64, 1, 1, 1) FLUTE_ROW(64, 2, 1, 1) FLUTE_ROW(64, 4, 1, 1) FLUTE_ROW(64, 1, 2, 1) FLUTE_ROW(64, 2, 2, 1) FLUTE_ROW(64, 1, 4, 1) FLUTE_ROW(64, 2, 4, 1)
    return nullptr;
}
}  // namespace flute_amd
