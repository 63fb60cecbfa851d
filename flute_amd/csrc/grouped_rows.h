// What makes a kernel grouped: how the rows of a mixture-of-experts launch are read out of `offsets`.
//
// offsets [E + 1] int32 lives in device memory and is read by the kernels only (never by the host: every grid follows from the
// shapes alone, a launch is hipGraph-capturable and a replay honours whatever the table then holds).  Expert e < E serves the
// rows [offsets[e], offsets[e + 1]) of the R sorted rows; the rows from offsets[E] on are served by no expert.  Every read of
// the table in csrc is in this header, but for param_grad_kernel (grad_gemm.h), which applies grouped_clamp to its two entries
// itself (DESIGN.md 3.3o says why); moe_route_sort.h writes the table.  The contract of every grouped kernel:
//
//   * Every bound is clamped to [0, R] before it forms an address, and every row index a kernel forms is in [rb, re).
//   * An expert without rows (re <= rb) requests nothing: no weight, scale or table word of it is read, it owns no block.
//   * A malformed table (decreasing or overlapping ranges) therefore stays inside the operands; it may own a row twice - the
//     row then holds either expert's result - or own more 128-row blocks than the grid holds - the surplus is dropped and its
//     rows are left unwritten.
//
// The block forms (qgemm_block2.h's grouped front end, qgemm_grouped_input_grad_blocks.h) count the 128-row blocks of all
// experts in expert order, expert e owning ceil(max(re - rb, 0) / 128) of them; their grid holds grouped_blocks_row_blocks(E, R),
// the most a monotone table can own, and what they serve is decided by the two *_eligible rules below and nothing else.
#pragma once
#include "common.h"

namespace flute_amd {

constexpr int kGroupedBlockRows = 128;

// Row blocks of a launch: the most a monotone table over T rows and E experts can own, floor((T + 127 E) / 128) - an expert
// with r rows owns ceil(r / 128) <= (r + 127) / 128 blocks, and the sum of integers is at most the floor of the sum.
inline long long grouped_blocks_row_blocks(int E, int T) {
    return ((long long)T + (long long)(kGroupedBlockRows - 1) * E) / kGroupedBlockRows;
}

// What the block form of the forward serves (api_train.hip's form rule and refusal read this, nothing else decides it): plain (0) and
// weighted (2), 4 / 2 bits, scale rows in whole 8-group blocks, whole 256-column blocks, and the 32-bit descriptor limits of
// choose_block - activation byte offsets (a block reaches up to 127 rows past its expert's end), one expert's scale bytes - and
// a 31-bit grid.
inline bool grouped_blocks_eligible(int mode, int num_bits, int lg, int E, int T, int N, int K) {
    if (mode != 0 && mode != 2) return false;
    if (num_bits != 4 && num_bits != 2) return false;
    if (E < 1 || T < 1 || N < 256 || N % 256 || K < 64 || (K >> lg) % 8) return false;
    if ((size_t)(T + 256) * K * 2 >= (size_t)0xfffffff0u) return false;
    if ((size_t)N * (K >> lg) * 2 >= (size_t)0xfffffff0u) return false;
    return grouped_blocks_row_blocks(E, T) * (N / 256) <= 0x7fffffffLL;
}

// What the block form of the fused SwiGLU launch serves (flute_qgemm_grouped_glu_blocks; api_train.hip's refusal and query read this,
// nothing else decides it): the plain mode's conditions with F in N's place, but for the activations - the descriptor spans Xsrc
// and no block reaches past its expert, so Tsrc * K * 2 is what must stay below 2^32 - 16 - and a sorted-row index plus a block
// that stays an int (R is not bounded by Tsrc).
inline bool grouped_glu_blocks_eligible(int num_bits, int lg, int E, int R, int Tsrc, int F, int K) {
    if (num_bits != 4 && num_bits != 2) return false;
    if (E < 1 || R < 1 || Tsrc < 1 || F < 256 || F % 256 || K < 64 || (K >> lg) % 8) return false;
    if (R > 0x7fffffff - 2 * kGroupedBlockRows) return false;
    if ((size_t)Tsrc * K * 2 >= (size_t)0xfffffff0u) return false;
    if ((size_t)F * (K >> lg) * 2 >= (size_t)0xfffffff0u) return false;
    return grouped_blocks_row_blocks(E, R) * (F / 256) <= 0x7fffffffLL;
}

// What the block form of the input gradient serves (qgemm_grouped_input_grad_blocks.h; api_train.hip's form rule and refusal read
// this, nothing else decides it): 4 / 2 bits, whole 256-k blocks, a row index plus a block that stays an int, and a 31-bit
// grid.  (N, TileP and the group size are the slab form's, which the caller has checked with the layer; every base in the kernel
// is 64-bit and it builds no descriptor, so no operand size is refused.)
constexpr int kGroupedIgBlockK = 256;
inline bool grouped_input_grad_blocks_eligible(int num_bits, int E, int R, int N, int K) {
    if (num_bits != 4 && num_bits != 2) return false;
    if (E < 1 || R < 1 || N < 64 || N % 64 || K < kGroupedIgBlockK || K % kGroupedIgBlockK) return false;
    if (R > 0x7fffffff - 2 * kGroupedBlockRows) return false;
    return grouped_blocks_row_blocks(E, R) * (K / kGroupedIgBlockK) <= 0x7fffffffLL;
}

// The rows [rb, re) of expert e, both ends clamped to [0, R].
struct GroupedRows {
    int rb, re;
    __device__ __forceinline__ bool empty() const { return re <= rb; }
};
__device__ __forceinline__ int grouped_clamp(int v, int R) { return min(max(v, 0), R); }
__device__ __forceinline__ GroupedRows grouped_rows(const int* __restrict__ offsets, int e, int R) {
    return GroupedRows{grouped_clamp(offsets[e], R), grouped_clamp(offsets[e + 1], R)};
}
// The end of the rows some expert serves.
__device__ __forceinline__ int grouped_served(const int* __restrict__ offsets, int E, int R) {
    return grouped_clamp(offsets[E], R);
}

// The rows no expert serves, [grouped_served, R) of out [R, width] (16-bit elements, width % 4 == 0), written as zeros: 8 bytes
// per lane, grid-strided over the whole launch of THREADS-lane workgroups.
template <int THREADS>
__device__ __forceinline__ void grouped_zero_unserved(uint16_t* __restrict__ out, const int* __restrict__ offsets, int E, int R,
                                                      int width) {
    const int zb = grouped_served(offsets, E, R);
    const size_t n4 = (size_t)(R - zb) * (size_t)(width >> 2);
    ushort4* z = reinterpret_cast<ushort4*>(out + (size_t)zb * width);
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n4; i += (size_t)gridDim.x * THREADS)
        z[i] = ushort4{0, 0, 0, 0};
}

// The block map: row block b (the ROWS-row blocks of all experts counted in expert order) -> expert e, block `blk` of e and
// the expert's rows [rb, re); e < 0 for a b past the table's blocks.  Every wave finds the answer for itself - 64 experts per
// round, one per lane, an inclusive prefix sum over the lanes and a ballot - and it is wave-uniform, so the waves of a workgroup
// agree without LDS and without a barrier ahead of the first request.  The running total is 64-bit: a malformed table may claim
// more blocks than an int counts (a round's sum is < 2^31).
struct GroupedBlock {
    int e, blk, rb, re;
};
template <int ROWS>
__device__ __forceinline__ GroupedBlock grouped_block_map(const int* __restrict__ offsets, int E, int R, int b) {
    const int lane = threadIdx.x & 63;
    int e = -1, blk = 0, rb = 0, re = 0;
    long long base = 0;
    for (int c0 = 0; c0 < E; c0 += 64) {
        const int ee = c0 + lane;
        GroupedRows r{0, 0};
        if (ee < E) r = grouped_rows(offsets, ee, R);
        const int nb = (max(r.re - r.rb, 0) + ROWS - 1) / ROWS;    // blocks of expert ee
        int incl = nb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const unsigned long long hit = __ballot(base + incl > (long long)b);
        if (hit) {                                                 // the first lane whose running total passes b: its nb > 0
            const int src = __ffsll(hit) - 1;
            e = c0 + src;
            blk = (int)((long long)b - base) - __shfl(incl - nb, src);
            rb = __shfl(r.rb, src);
            re = __shfl(r.re, src);
            break;
        }
        base += __shfl(incl, 63);
    }
    return GroupedBlock{__builtin_amdgcn_readfirstlane(e), __builtin_amdgcn_readfirstlane(blk),
                        __builtin_amdgcn_readfirstlane(rb), __builtin_amdgcn_readfirstlane(re)};
}

}  // namespace flute_amd
