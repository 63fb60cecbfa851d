// The two streams of the fused SwiGLU launch's backward that are not GEMMs (include/flute_amd.h, flute_swiglu_grad and
// flute_moe_gather state the contracts and the error account):
//
//   swiglu_grad_kernel   dg = round_T((dh u) ds(g)),  du = round_T(dh silu32(g))  from g, u, dh [R, F], fp32 in the header's order
//   moe_gather_kernel    out[r, :] = X[clamp(rows[r], 0, Tsrc - 1), :]            the transpose of moe_combine: a copy
//
// With `offsets` the rows at or past served = clamp(offsets[E], 0, R) are written as +0 and none of their operands is read
// (g, u, dh there are what the plain launches left unwritten; rows[r] there is whatever the routing left); without it every
// row is served.  Every element of every output is written: no zero fill before the launch, no atomics, no LDS.
//
// Both are pure streams and share ONE launch shape, moe_combine's: one lane = 8 consecutive columns of one row - 16-B loads
// and one or two 16-B stores, so a wave-instruction moves 1 KB contiguous - and a workgroup of 128 lanes takes 1024 columns
// of one row (grid: rows x column chunks, no striding), which makes the row, its `served` test and its source row uniform in
// the workgroup.  Every element offset is 64-bit.  Both branches of the served test end in the same stores, so a lane either
// returns at once (past the row's end) or writes its vectors.
#include "kernels.h"
#include "grouped_rows.h"
#include "silu32.h"

namespace flute_amd {

constexpr int kRowStreamThreads = 128;

// rows at or past this one are zeros; offsets null: every row is served
__device__ __forceinline__ int row_stream_served(const int32_t* __restrict__ offsets, int E, int R) {
    return offsets ? grouped_served(offsets, E, R) : R;
}

// One element of the header's formula.  Contraction is off: every operation below rounds once, in this order (an fma
// for 1 + g (1 - sig) would be another function than the one the error account counts).
template <typename T>
__device__ __forceinline__ void swiglu_grad_element(uint16_t g16, uint16_t u16, uint16_t dh16, uint16_t& dg16, uint16_t& du16) {
#pragma clang fp contract(off)
    const float g = Num<T>::to_float(g16), u = Num<T>::to_float(u16), dh = Num<T>::to_float(dh16);
    const float d = 1.0f + expf(-g);
    const float sl = silu32(g);                          // g / d: the compiler forms d once
    const float sig = 1.0f / d;
    const float ds = sig * (1.0f + g * (1.0f - sig));
    dg16 = Num<T>::from_float((dh * u) * ds);
    du16 = Num<T>::from_float(dh * sl);
}

template <typename T>
__global__ __launch_bounds__(kRowStreamThreads) void swiglu_grad_kernel(const uint16_t* __restrict__ G,
                                                                        const uint16_t* __restrict__ U,
                                                                        const uint16_t* __restrict__ DH,
                                                                        const int32_t* __restrict__ offsets,
                                                                        uint16_t* __restrict__ DG, uint16_t* __restrict__ DU,
                                                                        int E, int R, int F, int col_blocks) {
    const int r = blockIdx.x / col_blocks;
    const int col = 8 * ((blockIdx.x - r * col_blocks) * kRowStreamThreads + threadIdx.x);
    if (col >= F) return;
    const size_t at = (size_t)r * F + col;
    uint32_t og[4] = {0, 0, 0, 0}, ou[4] = {0, 0, 0, 0};
    if (r < row_stream_served(offsets, E, R)) {
        const uint4 gv = *reinterpret_cast<const uint4*>(G + at);
        const uint4 uv = *reinterpret_cast<const uint4*>(U + at);
        const uint4 hv = *reinterpret_cast<const uint4*>(DH + at);
        const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w}, uw[4] = {uv.x, uv.y, uv.z, uv.w}, hw[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint16_t a0, b0, a1, b1;
            swiglu_grad_element<T>((uint16_t)(gw[i] & 0xffffu), (uint16_t)(uw[i] & 0xffffu), (uint16_t)(hw[i] & 0xffffu), a0, b0);
            swiglu_grad_element<T>((uint16_t)(gw[i] >> 16), (uint16_t)(uw[i] >> 16), (uint16_t)(hw[i] >> 16), a1, b1);
            og[i] = (uint32_t)a0 | ((uint32_t)a1 << 16);
            ou[i] = (uint32_t)b0 | ((uint32_t)b1 << 16);
        }
    }
    *reinterpret_cast<uint4*>(DG + at) = make_uint4(og[0], og[1], og[2], og[3]);
    *reinterpret_cast<uint4*>(DU + at) = make_uint4(ou[0], ou[1], ou[2], ou[3]);
}

__global__ __launch_bounds__(kRowStreamThreads) void moe_gather_kernel(const uint16_t* __restrict__ X,
                                                                       const int32_t* __restrict__ rows,
                                                                       const int32_t* __restrict__ offsets,
                                                                       uint16_t* __restrict__ out, int E, int R, int Tsrc,
                                                                       int K, int col_blocks) {
    const int r = blockIdx.x / col_blocks;
    const int col = 8 * ((blockIdx.x - r * col_blocks) * kRowStreamThreads + threadIdx.x);
    if (col >= K) return;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < row_stream_served(offsets, E, R)) {
        const int src = min(max(rows[r], 0), Tsrc - 1);
        v = *reinterpret_cast<const uint4*>(X + (size_t)src * K + col);
    }
    *reinterpret_cast<uint4*>(out + (size_t)r * K + col) = v;
}

// column chunks of 1024 per row; 0 when rows x chunks does not fit the grid (moe_combine_grid's rule)
unsigned row_stream_grid(int R, int width) {
    const size_t col_blocks = ((size_t)width / 8 + kRowStreamThreads - 1) / kRowStreamThreads;
    const size_t grid = (size_t)R * col_blocks;
    return grid <= 0x7fffffffu ? (unsigned)grid : 0u;
}

int swiglu_grad_dispatch(int dtype, int R, int F, int E, const void* g, const void* u, const void* dh, const int32_t* offsets,
                         void* dg, void* du, hipStream_t stream) {
    const int col_blocks = (F / 8 + kRowStreamThreads - 1) / kRowStreamThreads;
    const unsigned grid = row_stream_grid(R, F);
    const uint16_t* g16 = reinterpret_cast<const uint16_t*>(g);
    const uint16_t* u16 = reinterpret_cast<const uint16_t*>(u);
    const uint16_t* h16 = reinterpret_cast<const uint16_t*>(dh);
    uint16_t* dg16 = reinterpret_cast<uint16_t*>(dg);
    uint16_t* du16 = reinterpret_cast<uint16_t*>(du);
    if (dtype == FLUTE_F16)
        hipLaunchKernelGGL(swiglu_grad_kernel<F16>, dim3(grid), dim3(kRowStreamThreads), 0, stream, g16, u16, h16, offsets, dg16,
                           du16, E, R, F, col_blocks);
    else
        hipLaunchKernelGGL(swiglu_grad_kernel<BF16>, dim3(grid), dim3(kRowStreamThreads), 0, stream, g16, u16, h16, offsets, dg16,
                           du16, E, R, F, col_blocks);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

// (a copy of 16-bit patterns: one kernel serves both types)
int moe_gather_dispatch(int R, int Tsrc, int K, int E, const void* X, const int32_t* rows, const int32_t* offsets, void* out,
                        hipStream_t stream) {
    const int col_blocks = (K / 8 + kRowStreamThreads - 1) / kRowStreamThreads;
    hipLaunchKernelGGL(moe_gather_kernel, dim3(row_stream_grid(R, K)), dim3(kRowStreamThreads), 0, stream,
                       reinterpret_cast<const uint16_t*>(X), rows, offsets, reinterpret_cast<uint16_t*>(out), E, R, Tsrc, K,
                       col_blocks);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
