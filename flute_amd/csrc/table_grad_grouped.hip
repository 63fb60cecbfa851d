// The gradient of the lookup tables of E stacked packed layers over rows sorted by expert, one main launch and one
// small reduce launch:
//     dT2[e, c, h] = sum over (kappa, n) with idx_e(kappa, n) = c of G_e[2 kappa + h, n] * S[e, n, 2 kappa / g],
//     G_e[k, n]    = sum_{r in [b_e, e_e)} X[r, k] * dYw[r, n],
// b_e = clamp(offsets[e], 0, R), e_e = clamp(offsets[e + 1], 0, R), idx_e expert e's pair index as in table_grad.hip,
// dYw = dY, or round_T(row_weight[r] * dY[r, n]) (the product in fp32) formed where the dY tile is staged into LDS.
// dY [R, N] and X [R, K] row-major T, offsets [E + 1] int32 in device memory and read by the kernels only, Q [E, P, K],
// S [E, N, K / g] T, row_weight [R] fp32 or null, dT2 [E, 4^b, 2] fp32.  With dS given the same launch also writes the
// stack's scale gradient [E, N, K / g] (it reads QM2 [E, 4^b] then and only then) with scale_grad_grouped.hip's own
// mainloop and epilogue: bit for bit what flute_qgemm_grouped_scale_grad returns.
//
// The body is table_grad_kernel's - grad_gemm.h's mainloop and its table_grad_epilogue - with the row range read from
// `offsets` and the Q / S / QM2 / dS bases moved to expert e (64-bit).  The grid is (N / 128, ceil(K / 256), E), from
// the shapes alone: a workgroup walks ALL rows of its expert (no split of the row reduction) and writes one fp32
// partial [4^b][2] to the caller's scratch at (e, by, bx).  The reduce launch, one blockIdx.y per expert, is
// table_grad_reduce_kernel's scheme: per bin 32 slots each take every 32nd partial of the expert in the order
// by * gridDim.x + bx in fp64, then a fixed binary tree over the 32 and one rounding to fp32 - the dense op's order
// when it does not split M, so dT2[e] has flute_qgemm_table_grad's bits on the expert's rows wherever that launch does
// not split M.  No global atomics: equal arguments give equal bits.
//
// A workgroup whose expert has no rows returns before it requests a code, a scale or a table word; with a dS it writes
// its block of dS as zeros; it writes no partial.  The reduce kernel reads `offsets` itself: for such an expert it
// writes dT2[e] as zeros and does not read the scratch.  Every row index formed is in [b_e, e_e) inside [0, R): a
// malformed table is memory-safe, and rows from clamp(offsets[E]) on are never read.
//
// Scratch: E * (N / 128) * ceil(K / 256) * 2 * 4^b * 4 bytes, from the shapes alone - every (expert, block) has its
// slot whether or not the expert has rows, which is what keeps the host from reading offsets.  At a large stack
// (E 256, N 2048, K 7168, 4 bits) that is 256 * 16 * 28 * 2 KB = 235 MB.
//
// Addition-chain depth d of expert e with M_e = e_e - b_e rows, the most fp32 roundings one term x * dy * s passes
// through (table_grad.hip's derivation with M_e for M and no split):
//     32 * ceil(M_e / 32)   the mainloop, counting an MFMA as 32 chained additions
//     1                     the product with the scale
//     2048                  a wave's 64 x 64 sub-block holds 2048 elements of either pair half: all on one bin at worst
//     8                     the waves, in order
//     1                     the rounding of the fp64 total
// so d <= 32 * ceil(M_e / 32) + 2058.  (The weighted form rounds the operand dYw once more, before the chain.)
#include "kernels.h"
#include "grad_gemm.h"
#include "layout_dispatch.h"

namespace flute_amd {

constexpr int kTggRedBins = 32, kTggRedSlots = 32;  // the reduce pass: bins x partial slots per workgroup

// (4 waves per SIMD = two workgroups per CU: at most 128 VGPRs)
template <typename T, int BITS, int TILEP, bool WEIGHTED>
__global__ __launch_bounds__(kSgThreads, 4) void table_grad_grouped_kernel(
    const uint16_t* __restrict__ dY, const uint16_t* __restrict__ X, const int* __restrict__ offsets,
    const uint32_t* __restrict__ Q, const uint16_t* __restrict__ S, const uint32_t* __restrict__ QM2,
    const float* __restrict__ row_weight, uint16_t* __restrict__ dS, float* __restrict__ t_part, int R, int N, int K,
    int P, int lg) {
    using L = Layout<BITS>;
    constexpr int NB = 2 * L::LUT_N;                  // bins
    __shared__ __attribute__((aligned(16))) char smem[kSgLds];
    const int tid = threadIdx.x;
    const int nb = blockIdx.x * kSgBN, kb = blockIdx.y * kSgBK;
    const int e = (int)blockIdx.z;
    const size_t NG = (size_t)N * (size_t)(K >> lg);
    const int rb = min(max(offsets[e], 0), R);
    const int re = min(max(offsets[e + 1], 0), R);
    uint16_t* __restrict__ dSe = dS ? dS + (size_t)e * NG : nullptr;

    if (re <= rb) {                                   // no rows: nothing of the expert read, no partial written
        if (dSe) scale_grad_zero_block(dSe, N, K, lg, nb, kb);
        return;
    }

    uint32_t* lut = reinterpret_cast<uint32_t*>(smem + kSgLut);
    if (dS) {
        const uint32_t* __restrict__ Te = QM2 + (size_t)e * L::LUT_N;
        for (int i = tid; i < L::LUT_N; i += kSgThreads) lut[i] = Te[i];
    }

    f32x4_t acc[4][4];
    grad_gemm_mainloop<T, WEIGHTED>(smem, dY, X, N, K, nb, kb, rb, re, acc, row_weight);
    const uint32_t* __restrict__ Qe = Q + (size_t)e * (size_t)P * (size_t)(K >> 1);
    const size_t wg = ((size_t)e * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    table_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Qe, S + (size_t)e * NG, dSe, nullptr, t_part + wg * NB, N, K,
                                        lg, nb, kb);
}

// dT2[e][bin] = sum over expert e's workgroups of part[e][wg][bin], in fp64 in table_grad_reduce_kernel's order; zeros
// for an expert without rows, whose partials were never written
__global__ __launch_bounds__(kTggRedBins* kTggRedSlots) void table_grad_grouped_reduce_kernel(
    const float* __restrict__ part, const int* __restrict__ offsets, float* __restrict__ dT2, int nbins, int wgs,
    int R) {
    __shared__ double red[kTggRedSlots][kTggRedBins];
    const int b = threadIdx.x % kTggRedBins, slot = threadIdx.x / kTggRedBins;
    const int bin = blockIdx.x * kTggRedBins + b;     // nbins is a multiple of 32
    const int e = (int)blockIdx.y;
    const int rb = min(max(offsets[e], 0), R);
    const int re = min(max(offsets[e + 1], 0), R);
    float* __restrict__ out = dT2 + (size_t)e * nbins;
    if (re <= rb) {                                   // uniform over the workgroup
        if (slot == 0) out[bin] = 0.f;
        return;
    }
    const float* __restrict__ pe = part + (size_t)e * (size_t)wgs * (size_t)nbins;
    double v = 0.0;
    for (int w = slot; w < wgs; w += kTggRedSlots) v += (double)pe[(size_t)w * nbins + bin];
    red[slot][b] = v;
    __syncthreads();
    for (int s = kTggRedSlots / 2; s > 0; s >>= 1) {
        if (slot < s) red[slot][b] += red[slot + s][b];
        __syncthreads();
    }
    if (slot == 0) out[bin] = (float)red[0][b];
}

size_t table_grad_grouped_scratch_bytes(int num_bits, int E, int N, int K) {
    return (size_t)E * (size_t)(N / kSgBN) * (size_t)((K + kSgBK - 1) / kSgBK) * ((size_t)2 << (2 * num_bits)) * 4;
}

int table_grad_grouped_dispatch(int dtype, int num_bits, int tile_p, int lg, int E, int R, int N, int K, int P,
                                const void* dY, const void* X, const void* offsets, const void* Q, const void* S,
                                const void* QM2, const void* row_weight, float* dT2, void* dS, void* scratch,
                                hipStream_t stream) {
    const dim3 grid(N / kSgBN, (K + kSgBK - 1) / kSgBK, E);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(dY);
    const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
    const int* off = reinterpret_cast<const int*>(offsets);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(Q);
    const uint16_t* s = reinterpret_cast<const uint16_t*>(S);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    const float* rw = reinterpret_cast<const float*>(row_weight);
    uint16_t* ds = reinterpret_cast<uint16_t*>(dS);
    float* t_part = reinterpret_cast<float*>(scratch);
    const int err = dispatch_layout(dtype, num_bits, tile_p, [&](auto t, auto bits, auto tp) {
        auto launch = [&](auto weighted) {
            hipLaunchKernelGGL((table_grad_grouped_kernel<decltype(t), decltype(bits)::value, decltype(tp)::value,
                                                          decltype(weighted)::value>),
                               grid, dim3(kSgThreads), 0, stream, y, x, off, q, s, qm2, rw, ds, t_part, R, N, K, P, lg);
        };
        if (rw) launch(std::true_type{});
        else launch(std::false_type{});
    });
    if (err != FLUTE_OK) return err;
    if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    const int nbins = 2 << (2 * num_bits);
    hipLaunchKernelGGL(table_grad_grouped_reduce_kernel, dim3(nbins / kTggRedBins, E),
                       dim3(kTggRedBins * kTggRedSlots), 0, stream, t_part, off, dT2, nbins, (int)(grid.x * grid.y), R);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
