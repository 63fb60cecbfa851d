// The gradient of the scales of E stacked packed layers over rows sorted by expert, ONE launch:
//     dS[e, n, j] = round_T(sum_{r in [b_e, e_e)} sum_{k in group j} dYw[r, n] * X[r, k] * L_e[k, n]),
// b_e = clamp(offsets[e], 0, R), e_e = clamp(offsets[e + 1], 0, R), L_e = pair(QM2[e], Q[e]) as in scale_grad.hip,
// dYw = dY, or round_T(row_weight[r] * dY[r, n]) (the product in fp32) formed where the dY tile is staged into LDS.
// dY [R, N] and X [R, K] row-major T, offsets [E + 1] int32 in device memory and read by the kernel only, Q [E, P, K],
// QM2 [E, 4^b], row_weight [R] fp32 or null, dS [E, N, K / g] T.
//
// The body is scale_grad_kernel's - the table stage, grad_gemm.h's mainloop and its scale epilogue - with the row range
// read from `offsets` and the two pointers the epilogue takes moved to expert e.  The grid is (N / 128, ceil(K / 256), E),
// from the shapes alone: a workgroup walks ALL rows of its expert in the dense kernel's order (no split of the row
// reduction, no scratch, no atomics), so an expert's dS has the bits of flute_qgemm_scale_grad on its rows wherever
// that launch does not split M, and equal arguments give equal bits.  A workgroup whose expert has no rows writes its
// block of dS as zeros and returns before it requests a code or a table word.  Every row index formed is in
// [b_e, e_e) inside [0, R): a malformed table is memory-safe, and rows from clamp(offsets[E]) on are never read.  Expert
// bases into Q / QM2 / dS and row bases into dY / X are 64-bit.
#include "kernels.h"
#include "grad_gemm.h"
#include "layout_dispatch.h"

namespace flute_amd {

// (4 waves per SIMD = two workgroups per CU: at most 128 VGPRs)
template <typename T, int BITS, int TILEP, bool WEIGHTED>
__global__ __launch_bounds__(kSgThreads, 4) void scale_grad_grouped_kernel(
    const uint16_t* __restrict__ dY, const uint16_t* __restrict__ X, const int* __restrict__ offsets,
    const uint32_t* __restrict__ Q, const uint32_t* __restrict__ QM2, const float* __restrict__ row_weight,
    uint16_t* __restrict__ dS, int R, int N, int K, int P, int lg) {
    using L = Layout<BITS>;
    __shared__ __attribute__((aligned(16))) char smem[kSgLds];
    const int tid = threadIdx.x;
    const int nb = blockIdx.x * kSgBN, kb = blockIdx.y * kSgBK;
    const int e = (int)blockIdx.z;
    const int G = K >> lg;
    const int rb = min(max(offsets[e], 0), R);
    const int re = min(max(offsets[e + 1], 0), R);
    uint16_t* __restrict__ dSe = dS + (size_t)e * (size_t)N * (size_t)G;

    if (re <= rb) {                                   // no rows: the block's groups below K as zeros, nothing of the expert read
        scale_grad_zero_block(dSe, N, K, lg, nb, kb);
        return;
    }

    uint32_t* lut = reinterpret_cast<uint32_t*>(smem + kSgLut);
    const uint32_t* __restrict__ Te = QM2 + (size_t)e * L::LUT_N;
    for (int i = tid; i < L::LUT_N; i += kSgThreads) lut[i] = Te[i];

    f32x4_t acc[4][4];
    grad_gemm_mainloop<T, WEIGHTED>(smem, dY, X, N, K, nb, kb, rb, re, acc, row_weight);
    const uint32_t* __restrict__ Qe = Q + (size_t)e * (size_t)P * (size_t)(K >> 1);
    scale_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Qe, dSe, nullptr, N, K, lg, nb, kb);
}

int scale_grad_grouped_dispatch(int dtype, int num_bits, int tile_p, int lg, int E, int R, int N, int K, int P,
                                const void* dY, const void* X, const void* offsets, const void* Q, const void* QM2,
                                const void* row_weight, void* dS, hipStream_t stream) {
    const dim3 grid(N / kSgBN, (K + kSgBK - 1) / kSgBK, E);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(dY);
    const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
    const int* off = reinterpret_cast<const int*>(offsets);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(Q);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    const float* rw = reinterpret_cast<const float*>(row_weight);
    uint16_t* ds = reinterpret_cast<uint16_t*>(dS);
    const int err = dispatch_layout(dtype, num_bits, tile_p, [&](auto t, auto bits, auto tp) {
        auto launch = [&](auto weighted) {
            hipLaunchKernelGGL((scale_grad_grouped_kernel<decltype(t), decltype(bits)::value, decltype(tp)::value,
                                                          decltype(weighted)::value>),
                               grid, dim3(kSgThreads), 0, stream, y, x, off, q, qm2, rw, ds, R, N, K, P, lg);
        };
        if (rw) launch(std::true_type{});
        else launch(std::false_type{});
    });
    if (err != FLUTE_OK) return err;
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
