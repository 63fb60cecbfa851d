// Explicit instantiations of the streaming decode kernel (qgemm_stream.h) for num_bits = 3:
// dtype x TileP x rows per pass x ring depth.  One translation unit per bit width (`make -j`).
#include "kernels.h"
#include "qgemm_stream.h"
namespace flute_amd {
#define FLUTE_ROW(TP, MB, D) \
    if (tile_p == TP && mb == MB && depth == D) return dtype == 0 ? (StreamKernel)qgemv_stream_kernel<F16, 3, TP, MB, D> : (StreamKernel)qgemv_stream_kernel<BF16, 3, TP, MB, D>;
StreamKernel stream_kernel_b3(int dtype, int tile_p, int mb, int depth) {
    FLUTE_ROW(32, 1, 2) FLUTE_ROW(32, 2, 2)
    FLUTE_ROW(32, 4, 2)      // four rows per pass (the 3-bit MFMA plans are 256 columns wide per wave and slow at M = 3, 4)
    return nullptr;
}
}  // namespace flute_amd
