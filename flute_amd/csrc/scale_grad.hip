// The gradient of a packed layer's scales: dS[n, j] = round_T(sum_m sum_{k in group j} dY[m, n] * X[m, k] * L[k, n]),
// L[k, n] = pair(QM2, Q)[k, n] the value dequant.hip multiplies by the scale (table2 only, the qgemm kernels' pair index),
// dY [M, N] and X [M, K] row-major T, dS [N, K / g] T.  Products and sums in fp32, one rounding to T.
//
// A GEMM that reduces over M with the code lookup in its epilogue (grad_gemm.h: the mainloop and this epilogue, shared
// with table_grad.hip).  When the blocks do not fill the chip, M is split across workgroups: each writes fp32 partials
// [split][N][K / g] to the caller's scratch and a second pass sums them in split order and rounds once
// (splitk_reduce_kernel).  No atomics: the same arguments give the same bits.
#include <algorithm>

#include "kernels.h"
#include "grad_gemm.h"
#include "layout_dispatch.h"

namespace flute_amd {

template <typename T, int BITS, int TILEP>
__global__ __launch_bounds__(kSgThreads) void scale_grad_kernel(const uint16_t* __restrict__ dY,
                                                                const uint16_t* __restrict__ X,
                                                                const uint32_t* __restrict__ Q,
                                                                const uint32_t* __restrict__ QM2,
                                                                uint16_t* __restrict__ dS, float* __restrict__ part,
                                                                int M, int N, int K, int lg, int steps_per_split) {
    using L = Layout<BITS>;
    __shared__ __attribute__((aligned(16))) char smem[kSgLds];
    const int tid = threadIdx.x;
    const int nb = blockIdx.x * kSgBN, kb = blockIdx.y * kSgBK;

    uint32_t* lut = reinterpret_cast<uint32_t*>(smem + kSgLut);
    for (int i = tid; i < L::LUT_N; i += kSgThreads) lut[i] = QM2[i];

    const int m_begin = (int)blockIdx.z * steps_per_split * kSgBM;
    const int m_end = (int)min((long)M, (long)m_begin + (long)steps_per_split * kSgBM);
    f32x4_t acc[4][4];
    grad_gemm_mainloop<T>(smem, dY, X, N, K, nb, kb, m_begin, m_end, acc);
    float* pout = part ? part + (size_t)blockIdx.z * N * (K >> lg) : nullptr;
    scale_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Q, dS, pout, N, K, lg, nb, kb);
}

// splits of M for the launch: 1 when the blocks fill the chip (two workgroups per CU) or the scratch holds no split
int scale_grad_splits(int M, int N, int K, int lg, int num_sms, size_t scratch_bytes) {
    const long blocks = (long)(N / kSgBN) * ((K + kSgBK - 1) / kSgBK);
    const long steps = ((long)M + kSgBM - 1) / kSgBM;
    const long target = 2L * (num_sms < 1 ? 256 : num_sms);
    const size_t per_split = (size_t)N * (size_t)(K >> lg) * 4;
    long splits = std::min((target + blocks - 1) / blocks, steps / kSgMinSteps);
    splits = std::min<long>(splits, (long)std::min<size_t>(scratch_bytes / per_split, 1024));
    if (splits < 2) return 1;
    const long sps = (steps + splits - 1) / splits;   // every split gets >= 1 step
    return (int)((steps + sps - 1) / sps);
}

size_t scale_grad_full_scratch(int N, int K, int lg, int num_sms) {
    const long blocks = (long)(N / kSgBN) * ((K + kSgBK - 1) / kSgBK);
    const long target = 2L * (num_sms < 1 ? 256 : num_sms);
    if (blocks < 1 || blocks >= target) return 0;
    return (size_t)((target + blocks - 1) / blocks) * (size_t)N * (size_t)(K >> lg) * 4;
}

int scale_grad_dispatch(int dtype, int num_bits, int tile_p, int lg, int M, int N, int K, const void* dY,
                        const void* X, const void* Q, const void* QM2, void* dS, void* scratch, size_t scratch_bytes,
                        int num_sms, hipStream_t stream) {
    const int splits = scratch ? scale_grad_splits(M, N, K, lg, num_sms, scratch_bytes) : 1;
    const long steps = ((long)M + kSgBM - 1) / kSgBM;
    const int sps = (int)((steps + splits - 1) / splits);
    const dim3 grid(N / kSgBN, (K + kSgBK - 1) / kSgBK, splits);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(dY);
    const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(Q);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    uint16_t* ds = reinterpret_cast<uint16_t*>(dS);
    float* part = splits > 1 ? reinterpret_cast<float*>(scratch) : nullptr;
    const int err = dispatch_layout(dtype, num_bits, tile_p, [&](auto t, auto bits, auto tp) {
        hipLaunchKernelGGL((scale_grad_kernel<decltype(t), bits(), tp()>), grid, dim3(kSgThreads), 0, stream, y, x, q, qm2,
                           ds, part, M, N, K, lg, sps);
    });
    if (err != FLUTE_OK) return err;
    if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    if (splits > 1) {
        const size_t mn = (size_t)N * (size_t)(K >> lg);  // a multiple of 16: N % 128 == 0
        const unsigned rgrid = (unsigned)((mn / 4 + 255) / 256);
        if (dtype == FLUTE_F16)
            hipLaunchKernelGGL(splitk_reduce_kernel<F16>, dim3(rgrid), dim3(256), 0, stream, part, ds, mn, splits);
        else
            hipLaunchKernelGGL(splitk_reduce_kernel<BF16>, dim3(rgrid), dim3(256), 0, stream, part, ds, mn, splits);
        if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    }
    return FLUTE_OK;
}

}  // namespace flute_amd
