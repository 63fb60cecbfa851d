// The end of a mixture-of-experts step: out[t, :] = round_T( sum over the slots j of token t, ascending, of Y[pos[t, j], :] ),
// fp32 additions in slot order from +0 and ONE rounding (include/flute_amd.h, flute_moe_combine).  Y [P, N] are the down
// projection's rows in sorted order, pos [T, k] is moe_route's inverse index.  A slot whose position is outside
// [0, served), served = clamp(offsets[E], 0, P), adds nothing and its row is never read, so whatever the rows no expert
// wrote hold cannot reach `out`; every element of `out` is written (no zero fill before the launch, no atomics).
//
// A pure stream of P N + T N elements.  One lane = 8 consecutive columns of one token: one 16-B load per slot and one
// 16-B store, so a wave-instruction moves 1 KB contiguous.  A workgroup of 128 lanes takes 1024 columns of one token
// (grid: tokens x column chunks), which makes the token, its k positions and `served` uniform in the workgroup.  The
// slots are taken four at a time so that four independent loads are in flight before the first addition; a slot that
// is skipped adds +0, which leaves an accumulator that started at +0 unchanged bit for bit (it is never -0).
#include "kernels.h"
#include "grouped_rows.h"

namespace flute_amd {

constexpr int kCombineThreads = 128;

template <typename T>
__global__ __launch_bounds__(kCombineThreads) void moe_combine_kernel(const uint16_t* __restrict__ Y,
                                                                      const int32_t* __restrict__ pos,
                                                                      const int32_t* __restrict__ offsets,
                                                                      uint16_t* __restrict__ out, int k, int E, int P,
                                                                      int N, int col_blocks) {
    const int t = blockIdx.x / col_blocks;
    const int col = 8 * ((blockIdx.x - t * col_blocks) * kCombineThreads + threadIdx.x);
    if (col >= N) return;
    const int served = grouped_served(offsets, E, P);
    const int32_t* __restrict__ slot = pos + (size_t)t * k;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
    for (int j = 0; j < k; j += 4) {
        uint4 y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            y[u] = make_uint4(0, 0, 0, 0);
            if (j + u < k) {
                const int p = slot[j + u];
                if (p >= 0 && p < served) y[u] = *reinterpret_cast<const uint4*>(Y + (size_t)p * N + col);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t word[4] = {y[u].x, y[u].y, y[u].z, y[u].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[2 * i] += Num<T>::to_float((uint16_t)(word[i] & 0xffffu));
                acc[2 * i + 1] += Num<T>::to_float((uint16_t)(word[i] >> 16));
            }
        }
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        o[i] = (uint32_t)Num<T>::from_float(acc[2 * i]) | ((uint32_t)Num<T>::from_float(acc[2 * i + 1]) << 16);
    *reinterpret_cast<uint4*>(out + (size_t)t * N + col) = make_uint4(o[0], o[1], o[2], o[3]);
}

// column chunks of 1024 per token; 0 when tokens x chunks does not fit the grid
unsigned moe_combine_grid(int T, int N) {
    const size_t col_blocks = ((size_t)N / 8 + kCombineThreads - 1) / kCombineThreads;
    const size_t grid = (size_t)T * col_blocks;
    return grid <= 0x7fffffffu ? (unsigned)grid : 0u;
}

int moe_combine_dispatch(int dtype, int T, int k, int E, int N, const void* Y, const int32_t* pos, const int32_t* offsets,
                         void* out, hipStream_t stream) {
    const int col_blocks = (N / 8 + kCombineThreads - 1) / kCombineThreads;
    const unsigned grid = moe_combine_grid(T, N);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(Y);
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    if (dtype == FLUTE_F16)
        hipLaunchKernelGGL(moe_combine_kernel<F16>, dim3(grid), dim3(kCombineThreads), 0, stream, y, pos, offsets, o, k, E,
                           T * k, N, col_blocks);
    else
        hipLaunchKernelGGL(moe_combine_kernel<BF16>, dim3(grid), dim3(kCombineThreads), 0, stream, y, pos, offsets, o, k, E,
                           T * k, N, col_blocks);
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
