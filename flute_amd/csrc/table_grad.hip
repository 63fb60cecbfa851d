// The gradient of a packed layer's lookup table with the codes fixed: for the 4^b x 2 pair codebook the kernels read,
//     dT2[c, e] = sum over (kappa, n) with idx(kappa, n) = c of G[2 kappa + e, n] * S[n, 2 kappa / g],
// G = X^T dY (reduced over M), idx the kernels' pair index code(2 kappa) << b | code(2 kappa + 1); e = 0 is the low half
// of the pair word.  dY [M, N], X [M, K] and S [N, K / g] in T, dT2 [4^b][2] fp32 (it feeds an fp32 master parameter).
// The table itself is not read.  With dS given the same launch also writes the scale gradient (scale_grad.hip) with
// that kernel's own epilogue and split of M: bit for bit what flute_qgemm_scale_grad returns given its full scratch.
//
// The mainloop and the epilogue (table_grad_epilogue, which table_grad_grouped.hip shares) are grad_gemm.h's.
// Epilogue: every wave owns 4^b x 2 fp32 bins in LDS (8 x 2 KB at 4 bits, in the
// operand buffers, free by then).  A lane decodes the pair index behind each accumulator pair, multiplies both
// accumulators by the group's scale in fp32 and adds them into its wave's bins with ds_add_f32.  Only lanes of ONE wave
// ever meet on a bin, inside one instruction, and a wave's LDS instructions complete in program order: nothing depends
// on timing between waves.  (That colliding lanes of one instruction resolve in a fixed order is what
// tests/test_table_grad_gpu.py::test_reproducible checks.)  After a barrier the 8 waves' bins are summed in wave order
// and the workgroup writes one fp32 partial [4^b][2] to the caller's scratch, at its own index.  table_grad_reduce_kernel
// sums the partials of all workgroups in fp64: per bin 32 threads take every 32nd workgroup in order, then a fixed
// binary tree over the 32, one rounding to fp32.  No global atomics: the same arguments give the same bits.
//
// Addition-chain depth d, the most fp32 roundings one term x * dy * s passes through:
//     32 * steps   the mainloop, counting an MFMA as 32 chained additions (steps = 32-row steps of the workgroup's M
//                  range, <= ceil(M / 32))
//     1            the product with the scale
//     2048         a wave's 64 x 64 sub-block holds 2048 elements of either pair half: all on one bin at worst
//     8            the waves, in order
//     1            the rounding of the fp64 total
// so d <= 32 * ceil(M / 32) + 2058, whatever the layer's size (tests/table_grad_ref.py restates it).
#include <algorithm>

#include "kernels.h"
#include "grad_gemm.h"
#include "layout_dispatch.h"

namespace flute_amd {

constexpr int kTgRedBins = 32, kTgRedSlots = 32;    // the reduce pass: bins x workgroup slots per workgroup

// (4 waves per SIMD = two workgroups per CU, as scale_grad_kernel reaches by itself: at most 128 VGPRs)
template <typename T, int BITS, int TILEP>
__global__ __launch_bounds__(kSgThreads, 4) void table_grad_kernel(const uint16_t* __restrict__ dY,
                                                                const uint16_t* __restrict__ X,
                                                                const uint32_t* __restrict__ Q,
                                                                const uint16_t* __restrict__ S,
                                                                const uint32_t* __restrict__ QM2,
                                                                uint16_t* __restrict__ dS, float* __restrict__ ds_part,
                                                                float* __restrict__ t_part, int M, int N, int K, int lg,
                                                                int steps_per_split) {
    using L = Layout<BITS>;
    constexpr int NB = 2 * L::LUT_N;                  // bins
    __shared__ __attribute__((aligned(16))) char smem[kSgLds];
    const int tid = threadIdx.x;
    const int nb = blockIdx.x * kSgBN, kb = blockIdx.y * kSgBK;

    uint32_t* lut = reinterpret_cast<uint32_t*>(smem + kSgLut);
    if (dS)
        for (int i = tid; i < L::LUT_N; i += kSgThreads) lut[i] = QM2[i];

    const int m_begin = (int)blockIdx.z * steps_per_split * kSgBM;
    const int m_end = (int)min((long)M, (long)m_begin + (long)steps_per_split * kSgBM);
    f32x4_t acc[4][4];
    grad_gemm_mainloop<T>(smem, dY, X, N, K, nb, kb, m_begin, m_end, acc);

    float* pout = ds_part ? ds_part + (size_t)blockIdx.z * N * (K >> lg) : nullptr;   // (null without a dS)
    const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    table_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Q, S, dS, pout, t_part + wg * NB, N, K, lg, nb, kb);
}

// dT2[bin] = sum over workgroups of part[wg][bin], in fp64 in a fixed order
__global__ __launch_bounds__(kTgRedBins* kTgRedSlots) void table_grad_reduce_kernel(const float* __restrict__ part,
                                                                                     float* __restrict__ dT2, int nbins,
                                                                                     long wgs) {
    __shared__ double red[kTgRedSlots][kTgRedBins];
    const int b = threadIdx.x % kTgRedBins, slot = threadIdx.x / kTgRedBins;
    const int bin = blockIdx.x * kTgRedBins + b;      // nbins is a multiple of 32
    double v = 0.0;
    for (long w = slot; w < wgs; w += kTgRedSlots) v += (double)part[(size_t)w * nbins + bin];
    red[slot][b] = v;
    __syncthreads();
    for (int s = kTgRedSlots / 2; s > 0; s >>= 1) {
        if (slot < s) red[slot][b] += red[slot + s][b];
        __syncthreads();
    }
    if (slot == 0) dT2[bin] = (float)red[0][b];
}

namespace {
struct TgShape { int splits; size_t ds_bytes, t_bytes; };
// the split of M is scale_grad's under its full scratch, with or without dS: dT2 does not depend on want_dS
TgShape table_grad_shape(int num_bits, int lg, int M, int N, int K, int want_dS, int num_sms) {
    TgShape s;
    s.splits = scale_grad_splits(M, N, K, lg, num_sms, scale_grad_full_scratch(N, K, lg, num_sms));
    const size_t wgs = (size_t)(N / kSgBN) * (size_t)((K + kSgBK - 1) / kSgBK) * (size_t)s.splits;
    s.ds_bytes = (want_dS && s.splits > 1) ? (size_t)s.splits * (size_t)N * (size_t)(K >> lg) * 4 : 0;
    s.t_bytes = wgs * ((size_t)2 << (2 * num_bits)) * 4;
    return s;
}
}  // namespace

size_t table_grad_scratch_bytes(int num_bits, int lg, int M, int N, int K, int want_dS, int num_sms) {
    const TgShape s = table_grad_shape(num_bits, lg, M, N, K, want_dS, num_sms);
    return s.ds_bytes + s.t_bytes;
}

int table_grad_dispatch(int dtype, int num_bits, int tile_p, int lg, int M, int N, int K, const void* dY,
                        const void* X, const void* Q, const void* S, const void* QM2, float* dT2, void* dS,
                        void* scratch, int num_sms, hipStream_t stream) {
    const TgShape sh = table_grad_shape(num_bits, lg, M, N, K, dS != nullptr, num_sms);
    const int splits = sh.splits;
    const long steps = ((long)M + kSgBM - 1) / kSgBM;
    const int sps = (int)((steps + splits - 1) / splits);
    const dim3 grid(N / kSgBN, (K + kSgBK - 1) / kSgBK, splits);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(dY);
    const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(Q);
    const uint16_t* s = reinterpret_cast<const uint16_t*>(S);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    uint16_t* ds = reinterpret_cast<uint16_t*>(dS);
    float* ds_part = sh.ds_bytes ? reinterpret_cast<float*>(scratch) : nullptr;
    float* t_part = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + sh.ds_bytes);
    const int err = dispatch_layout(dtype, num_bits, tile_p, [&](auto t, auto bits, auto tp) {
        hipLaunchKernelGGL((table_grad_kernel<decltype(t), bits(), tp()>), grid, dim3(kSgThreads), 0, stream, y, x, q, s,
                           qm2, ds, ds_part, t_part, M, N, K, lg, sps);
    });
    if (err != FLUTE_OK) return err;
    if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    const int nbins = 2 << (2 * num_bits);
    const long wgs = (long)grid.x * grid.y * grid.z;
    hipLaunchKernelGGL(table_grad_reduce_kernel, dim3(nbins / kTgRedBins), dim3(kTgRedBins * kTgRedSlots), 0, stream,
                       t_part, dT2, nbins, wgs);
    if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    if (ds_part) return splitk_reduce_dispatch(dtype, ds_part, dS, (size_t)N * (size_t)(K >> lg), splits, stream);
    return FLUTE_OK;
}

}  // namespace flute_amd
