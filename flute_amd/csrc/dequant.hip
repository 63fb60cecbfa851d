// The dense dequantized weight: W[n, k - k_begin] = round_T(pair(QM2, Q)[k, n] * S[n, k / group_size]) for
// k_begin <= k < k_begin + k_count, W [N, k_count] row-major in T (the nn.Linear weight layout).  The lookup is the
// qgemm kernels' (table2 only, pair index code[2 kappa] << b | code[2 kappa + 1]) and so is the one rounding
// (Num<T>::mul_scale), so W equals what qgemm(I) returns, element by element.
//
// A store-bound stream: per element b/8 bytes in and 2 bytes out.  One lane = one unit (layout: common.h) x 4
// consecutive kappa = 8 consecutive k: one 16-B load per plane from the unit's Q32 rows, which are contiguous in kappa,
// and one 16-B store of 8 consecutive k to each of the unit's J output rows.  Consecutive lanes take consecutive
// kappa quads of the same unit, so one wave-instruction stores up to 1 KB contiguous per row and loads 1 KB contiguous
// per plane.  Every workgroup stages the pair table (<= 1 KB) in LDS; the 8 k of a lane share one scale (8 divides
// every group size).
#include "kernels.h"
#include "layout_dispatch.h"

namespace flute_amd {

constexpr int kDequantThreads = 256;
// the grid is capped and every thread strides over it: the table is staged once per workgroup, not once per 16 KB
constexpr unsigned kDequantMaxBlocks = 8192;

template <typename T, int BITS, int TILEP>
__global__ __launch_bounds__(kDequantThreads) void dequant_kernel(const uint32_t* __restrict__ Q,
                                                                   const uint16_t* __restrict__ S,
                                                                   const uint32_t* __restrict__ QM2,
                                                                   uint16_t* __restrict__ W, int N, int K, int lg,
                                                                   int k_begin, int k_count) {
    using L = Layout<BITS>;
    constexpr int J = L::J;
    constexpr int NP = L::NPLANES;
    __shared__ uint32_t lut[L::LUT_N];
    for (int i = threadIdx.x; i < L::LUT_N; i += kDequantThreads) lut[i] = QM2[i];
    __syncthreads();

    const int K2 = K >> 1;
    const int G = K >> lg;
    const uint32_t nq = (uint32_t)k_count >> 3;                  // kappa quads per unit in the range
    const size_t total = (size_t)(N / J) * nq;
    const size_t stride = (size_t)gridDim.x * kDequantThreads;
    for (size_t idx = (size_t)blockIdx.x * kDequantThreads + threadIdx.x; idx < total; idx += stride) {
        const int u = (int)(idx / nq);
        const int q = (int)(idx - (size_t)u * nq);
        const int k0 = k_begin + 8 * q;                          // first k of this lane
        uint4 w4[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
            w4[pl] = *reinterpret_cast<const uint4*>(Q + (size_t)unit_row<BITS, TILEP>(u, pl, N) * K2 + (k0 >> 1));
        const int n0 = unit_col0<BITS, TILEP>(u);
        const int gi = k0 >> lg;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int n = n0 + j * TILEP;
            const uint32_t s = S[(size_t)n * G + gi];
            uint32_t o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                uint32_t w[NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) w[pl] = (&w4[pl].x)[e];
                // pair word: low half is k = 2 kappa, high half k = 2 kappa + 1 - two consecutive T of the output row
                o[e] = Num<T>::mul_scale(lut[field<BITS>(w, j)], s);
            }
            *reinterpret_cast<uint4*>(W + (size_t)n * k_count + 8 * q) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

int dequant_dispatch(int dtype, int num_bits, int tile_p, int N, int K, int lg, int k_begin, int k_count,
                     const void* Q, const void* S, const void* QM2, void* W, hipStream_t stream) {
    const int J = (num_bits == 3) ? 16 : 16 / num_bits;
    const size_t total = (size_t)(N / J) * (size_t)(k_count / 8);
    const size_t blocks = (total + kDequantThreads - 1) / kDequantThreads;
    const unsigned grid = (unsigned)(blocks < kDequantMaxBlocks ? blocks : kDequantMaxBlocks);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(Q);
    const uint16_t* s = reinterpret_cast<const uint16_t*>(S);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    uint16_t* w = reinterpret_cast<uint16_t*>(W);
    const int err = dispatch_layout(dtype, num_bits, tile_p, [&](auto t, auto bits, auto tp) {
        hipLaunchKernelGGL((dequant_kernel<decltype(t), bits(), tp()>), dim3(grid), dim3(kDequantThreads), 0, stream, q, s,
                           qm2, w, N, K, lg, k_begin, k_count);
    });
    if (err != FLUTE_OK) return err;
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
