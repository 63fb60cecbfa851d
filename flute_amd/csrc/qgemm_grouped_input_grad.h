// The input gradient of the grouped qgemm: dX[r, :] = round_T( w_r * sum_n dY[r, n] * w^_e[n, :] ) for the rows r in
// [offsets[e], offsets[e + 1]) of every expert e < E, ONE launch whose grid does not depend on how the rows are spread.
// dY [R, N] holds the rows sorted by expert, offsets [E + 1] int32 lives in device memory and is read by the kernel only,
// Q [E, P, K] / S [E, N, K / g] / QM2 [E, 4^b] are the stacks flute_qgemm_grouped takes (layout: common.h).  It is a
// grouped GEMM over the packed stacks that contracts over N where the forward contracts over K.
//
// One kernel template, two forms (PAIR under `if constexpr`):
//
//   single   dX[r] = round_T( row_weight[r] * acc32 ) (row_weight null: no multiply)
//   pair     dX[r] = round_T( sum_n dY[r, n] w^(1)[n, :] + sum_n dY2[r, n] w^(2)[n, :] ): the n loop runs over the first
//            stack and then over the second into the SAME fp32 accumulators - the gradient of a row that fed both the
//            gate and the up projection of a gated MLP.
//
// Both write the rows [clamp(offsets[E]), R) - rows no expert serves - as zeros, spread over the whole grid.
//
// Arithmetic (include/flute_amd.h): w^ = round_T(lut * s) by Num<T>::mul_scale4, as dequant.hip and every MFMA kernel form
// it; products and sums in fp32 in the matrix core; one rounding of the output.  N is walked by ONE workgroup in a fixed
// order: no atomics, no split of the reduction across workgroups, equal arguments give equal bits.
//
// Work split.  A workgroup of 8 waves is (expert, k-slab of 128 k); it walks the expert's rows in blocks of 128 and, per
// row block, all of N in chunks of 64 columns.  A chunk is dequantized into LDS as dequant.hip forms the weight - one
// 16-B request per plane gives 8 consecutive k of a unit's J columns - by all 512 lanes: lane (unit ul < 64 / J, k-octet
// o < 16, field pair jp < J / 2) decodes fields 2 jp and 2 jp + 1 and writes 16 B to each of two rows of the
// [64 n][128 k] tile.  Tile row j * (64 / J) + ul is column unit_col0(u0 + ul) + j * TileP: any run of four rows is four
// consecutive columns of dY.  The contraction index of the MFMA is n, which the tile holds along its rows, so the A
// fragments are read back with ds_read_b64_tr_b16 (grad_gemm.h: lane 4 q + p of 16-lane group h supplies a row and the
// columns 4 p .. 4 p + 3; lane u of the group receives column u of the four rows).  Group h of a 32-n step takes rows
// 8 h .. 8 h + 7, the first read rows 8 h + 4 (h & 1) + q and the second the other four: each 32-lane half of a read then
// covers eight rows that differ mod 8, which the pitch of 72 dwords (8 mod 64) spreads over all 64 banks.  dY is the B
// operand, read from global memory as two 8-byte requests per lane and step in the same order of n.  Wave w owns rows
// 32 (w / 2) .. + 31 of the row block and k 64 (w % 2) .. + 63 of the slab: 2 x 4 accumulator tiles, so one decoded chunk
// feeds 8 MFMA row tiles in the workgroup, and per 32-n step a wave issues 4 x 2 transposed reads and 8 MFMAs.  A wave
// whose 32 rows lie past the expert's end, or whose 64 k lie past K (K % 64 == 0: the last slab may be half), still
// decodes and keeps the barriers but issues neither dY requests nor MFMAs.
//
// The tile is double buffered with one barrier per chunk: chunk c is written into buffer c % 2 and read after the barrier,
// and a wave reaches the writes of chunk c + 1 only behind the barrier of chunk c, which every wave passes after its reads
// of chunk c - 1.  The packed words, scales and dY of chunk c + 1 are requested before the MFMAs of chunk c.
//
// Rows.  [rb, re) of the expert, the zero fill and the contract on a malformed table: grouped_rows.h.  Expert bases into
// Q / S / QM2 and row bases into dY / dX are 64-bit.
#pragma once
#include "kernels.h"
#include "grouped_rows.h"
#include "mfma.h"
#include "grad_gemm.h"
#include "layout_dispatch.h"

namespace flute_amd {

constexpr int kIgWaves = 8;
constexpr int kIgThreads = kIgWaves * 64;
constexpr int kIgKS = 128;                                   // k per workgroup
constexpr int kIgRB = FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK;   // rows per pass over N
constexpr int kIgNC = 64;                                    // columns per chunk: two MFMA steps
constexpr int kIgPitch = kIgKS * 2 + 32;                     // bytes per tile row; 72 dwords = 8 mod 64
constexpr int kIgTile = kIgNC * kIgPitch;
constexpr int kIgLutWords = 2048;                            // per stack: LUT_N entries x C copies
static_assert(kIgRB == 128 && kIgKS == 128, "the wave layout below is 4 row groups x 2 k halves");

struct GroupedIgArgs {
    const uint16_t* dY[2];      // [R, N] T (pair: the second stack's)
    const int* offsets;         // [E + 1]
    const uint32_t* Q[2];       // [E, P, K / 2]
    const uint16_t* S[2];       // [E, N, K / g]
    const uint32_t* QM2[2];     // [E, 4^b]
    const float* row_weight;    // [R] or null (single form only)
    uint16_t* dX;               // [R, K]
    int R, N, K, P, lg, E, slabs;
};

// pair-table index of column j from the unit's words (w1, w2: 3 bits only), j a run-time value - a lane's two fields are
// fixed for the launch.  The words are passed by value: a select between elements of a local array becomes a load through
// a selected address, which puts the array into scratch.
template <int BITS>
__device__ __forceinline__ uint32_t field_rt(uint32_t w0, uint32_t w1, uint32_t w2, int j) {
    if constexpr (BITS == 4) {
        return (w0 >> (8 * j)) & 0xffu;
    } else if constexpr (BITS == 2) {
        return (w0 >> (4 * j)) & 0xfu;
    } else {
        const int m = j % 3, sh = 6 * (j / 3);
        const uint32_t ws = m == 0 ? w0 : (m == 1 ? w1 : w2);
        const uint32_t top = (w0 >> 30) | ((w1 >> 28) & 0xcu) | ((w2 >> 26) & 0x30u);
        return j == 15 ? top : ((ws >> sh) & 63u);
    }
}

// ---- what the slab form below and the block form (qgemm_grouped_input_grad_blocks.h) share

// copies of an expert's pair table in LDS, so that the lanes of a lookup spread over the banks: 8 / 32 / 32 at 4 / 3 / 2 bits
template <int BITS>
constexpr int kIgLutCopies = (kIgLutWords / Layout<BITS>::LUT_N) > 32 ? 32 : (kIgLutWords / Layout<BITS>::LUT_N);

// The table images of expert e, by the whole workgroup: stack s at lut + s * stride, entry i of copy c at word i * C + c.
template <int BITS, int NSTK>
__device__ __forceinline__ void ig_load_tables(uint32_t* lut, int stride, const GroupedIgArgs& a, int e) {
    using L = Layout<BITS>;
    constexpr int C = kIgLutCopies<BITS>;
#pragma unroll
    for (int s = 0; s < NSTK; ++s) {
        const uint32_t* __restrict__ Te = a.QM2[s] + (size_t)e * L::LUT_N;
        for (int i = threadIdx.x; i < L::LUT_N * C; i += kIgThreads) lut[s * stride + i] = Te[i / C];
    }
    __syncthreads();
}

// The decode of one k-octet of unit ul of a chunk, fields 2 jp and 2 jp + 1: from the unit's plane words w (8 consecutive k)
// and the two columns' scale words s, through the lane's copy lt of the stack's table image, 16 B to each of the tile rows
// (2 jp + f) * UC + ul at dst (the octet's place in tile row 0).  `in` false: the octet lies past K and zeros are written.
template <typename T, int BITS, int PITCH>
__device__ __forceinline__ void ig_decode_octet(const u32x4_t (&w)[Layout<BITS>::NPLANES], const uint32_t (&s)[2],
                                                const uint32_t* lt, int jp, int ul, bool in, char* dst) {
    constexpr int NP = Layout<BITS>::NPLANES;
    constexpr int UC = kIgNC / Layout<BITS>::J;
    constexpr int C = kIgLutCopies<BITS>;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int j = 2 * jp + f;
        uint32_t out[4] = {0, 0, 0, 0};
        if (in) {
            uint32_t v[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] = lt[field_rt<BITS>(w[0][d], w[NP > 1 ? 1 : 0][d], w[NP > 1 ? 2 : 0][d], j) * C];
            Num<T>::mul_scale4(v, s[f], out);
        }
        *reinterpret_cast<uint4*>(dst + (j * UC + ul) * PITCH) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// One A fragment: the two transposed reads of a 32-n step at byte `off` from the lane's addresses of step 0, k tile 0.
__device__ __forceinline__ u32x4_t ig_a_fragment(const uint32_t (&a_addr)[2], uint32_t off) {
    const uint2 a0 = lds_tr16(a_addr[0] + off);
    const uint2 a1 = lds_tr16(a_addr[1] + off);
    return u32x4_t{a0.x, a0.y, a1.x, a1.y};
}

// The epilogue of row tile t of a lane: its row `row` (< re) of dX at k0 + 16 kt .. + 3 for the four k tiles - the optional
// row weight (single form), one rounding, one 8-byte store per k tile.
template <typename T, bool PAIR, int RTILES>
__device__ __forceinline__ void ig_store_row(const GroupedIgArgs& a, const f32x4_t (&acc)[4][RTILES], int t, int row, int k0) {
    float w = 1.0f;
    if constexpr (!PAIR) {
        if (a.row_weight) w = a.row_weight[row];
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        f32x4_t s = acc[kt][t];
        if constexpr (!PAIR) {
            if (a.row_weight) { s[0] *= w; s[1] *= w; s[2] *= w; s[3] *= w; }
        }
        ushort4 v;
        v.x = Num<T>::from_float(s[0]); v.y = Num<T>::from_float(s[1]); v.z = Num<T>::from_float(s[2]); v.w = Num<T>::from_float(s[3]);
        *reinterpret_cast<ushort4*>(a.dX + (size_t)row * a.K + k0 + kt * 16) = v;
    }
}

template <typename T, int BITS, int TILEP, bool PAIR>
__global__ __launch_bounds__(kIgThreads) void qgemm_grouped_input_grad_kernel(const GroupedIgArgs a) {
    using L = Layout<BITS>;
    constexpr int J = L::J;
    constexpr int NP = L::NPLANES;
    constexpr int UC = kIgNC / J;                                  // units per chunk: 16 / 8 / 4
    constexpr int NSTK = PAIR ? 2 : 1;
    constexpr int C = kIgLutCopies<BITS>;
    static_assert(UC >= 4 && UC % 4 == 0 && TILEP % UC == 0 && UC * 16 * (J / 2) == kIgThreads, "chunk shape");

    __shared__ __attribute__((aligned(16))) char tile[2 * kIgTile];
    __shared__ uint32_t lut[NSTK][L::LUT_N * C];

    const int tid = threadIdx.x;
    const int R = a.R, N = a.N, K = a.K, lg = a.lg;

    grouped_zero_unserved<kIgThreads>(a.dX, a.offsets, a.E, R, K);

    const int e = (int)blockIdx.x / a.slabs;
    const int slab = (int)blockIdx.x - e * a.slabs;
    const GroupedRows er = grouped_rows(a.offsets, e, R);
    if (er.empty()) return;                                        // no rows: nothing of this expert is requested
    const int rb = er.rb, re = er.re;

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K2 = K >> 1;
    const int G = K >> lg;
    const int NCH = N / kIgNC;                                     // chunks per stack
    const int NCC = NSTK * NCH;
    const size_t q_base = (size_t)e * (size_t)a.P * (size_t)K2;
    const size_t s_base = (size_t)e * (size_t)N * (size_t)G;

    ig_load_tables<BITS, NSTK>(&lut[0][0], L::LUT_N * C, a, e);

    // ---- the lane as a decoder: unit ul of the chunk, k-octet o of the slab, fields 2 jp and 2 jp + 1
    const int o = tid & 15;
    const int ul = (tid >> 4) % UC;
    const int jp = (tid >> 4) / UC;
    const int k0 = slab * kIgKS + 8 * o;
    const bool k_in = k0 < K;                                      // K % 64 == 0: an octet is all in or all out
    const int gi = k0 >> lg;
    const int lut_lane = lane % C;
    struct Packed {
        u32x4_t w[NP];
        uint32_t s[2];
    };
    auto load_packed = [&](Packed& pk, int cc) {
        const bool in = k_in && cc < NCC;
        const int st = PAIR ? (cc >= NCH) : 0;
        const int u = (cc - st * NCH) * UC + ul;
        const uint32_t* __restrict__ Qs = a.Q[st] + q_base + (k0 >> 1);
        const uint16_t* __restrict__ Ss = a.S[st] + s_base + gi;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
            pk.w[pl] = in ? *reinterpret_cast<const u32x4_t*>(Qs + (size_t)unit_row<BITS, TILEP>(u, pl, N) * K2)
                          : u32x4_t{0, 0, 0, 0};
        const int n0 = unit_col0<BITS, TILEP>(u);
#pragma unroll
        for (int f = 0; f < 2; ++f) pk.s[f] = in ? (uint32_t)Ss[(size_t)(n0 + (2 * jp + f) * TILEP) * G] : 0u;
    };
    auto decode = [&](const Packed& pk, int cc) {
        ig_decode_octet<T, BITS, kIgPitch>(pk.w, pk.s, lut[PAIR ? (cc >= NCH) : 0] + lut_lane, jp, ul, k_in,
                                           tile + (cc & 1) * kIgTile + o * 16);
    };

    // ---- the lane in the MFMAs: rows 32 rg .. + 31 of the row block, k 64 kh .. + 63 of the slab
    const int rg = wave >> 1, kh = wave & 1;
    const int h = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3, r16 = lane & 15;
    const bool k_half_in = slab * kIgKS + kh * 64 < K;
    const uint32_t tbase = lds_base_of(tile);
    uint32_t a_addr[2];                                            // the two transposed reads of step 0, k tile 0, buffer 0
    int n_off[2][2];                                               // [step][read]: the lane's four columns of dY, from the chunk's first
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const int row = 8 * h + 4 * (hf ^ (h & 1));
        a_addr[hf] = tbase + (row + qq) * kIgPitch + (kh * 64 + 4 * p) * 2;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int rho = 32 * s + row;
            n_off[s][hf] = (rho / UC) * TILEP + rho % UC;
        }
    }

    for (int row0 = rb; row0 < re; row0 += kIgRB) {
        const bool active = k_half_in && row0 + 32 * rg < re;     // wave-uniform
        size_t yrow[2];
        bool yok[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = row0 + 32 * rg + 16 * t + r16;
            yok[t] = active && row < re;
            yrow[t] = (size_t)(yok[t] ? row : rb) * (size_t)N;    // < re <= R
        }
        struct Rows {
            u32x4_t y[2][2];                                       // [step][row tile]
        };
        auto load_rows = [&](Rows& rw, int cc) {
            const int st = PAIR ? (cc >= NCH) : 0;
            const uint16_t* __restrict__ Yp = a.dY[st] + unit_col0<BITS, TILEP>((cc - st * NCH) * UC);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    uint2 lo = make_uint2(0, 0), hi = make_uint2(0, 0);
                    if (yok[t] && cc < NCC) {
                        lo = *reinterpret_cast<const uint2*>(Yp + yrow[t] + n_off[s][0]);
                        hi = *reinterpret_cast<const uint2*>(Yp + yrow[t] + n_off[s][1]);
                    }
                    rw.y[s][t] = u32x4_t{lo.x, lo.y, hi.x, hi.y};
                }
        };

        f32x4_t acc[4][2];                                         // [k tile][row tile]
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[kt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

        Packed pk;
        Rows rw;
        load_packed(pk, 0);
        load_rows(rw, 0);
        for (int cc = 0; cc < NCC; ++cc) {
            decode(pk, cc);
            Packed pk_next;
            Rows rw_next;
            load_packed(pk_next, cc + 1);                          // past the end: no request, zeros
            load_rows(rw_next, cc + 1);
            __syncthreads();
            if (active) {
                const uint32_t buf = (cc & 1) * kIgTile;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4_t af[4];
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) af[kt] = ig_a_fragment(a_addr, buf + s * 32 * kIgPitch + kt * 32);
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int t = 0; t < 2; ++t) acc[kt][t] = Mfma<T>::run(af[kt], rw.y[s][t], acc[kt][t]);
                }
            }
            pk = pk_next;
            rw = rw_next;
        }

        // lane (q = h, r = r16) of tile (kt, t): row row0 + 32 rg + 16 t + r, k = slab 128 + 64 kh + 16 kt + 4 q .. + 3
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // (k < K: k_half_in and K % 64 == 0)
            if (yok[t]) ig_store_row<T, PAIR>(a, acc, t, row0 + 32 * rg + 16 * t + r16, slab * kIgKS + kh * 64 + 4 * h);
        }
        __syncthreads();                                           // the next row block's first chunk reuses buffer 0
    }
}

// The kernel's arguments from the launch's named operands; slabs is the launch's to set.
inline GroupedIgArgs grouped_ig_args(const GroupedInputGrad& g) {
    GroupedIgArgs a{};
    for (int s = 0; s < 2; ++s) {
        a.dY[s] = reinterpret_cast<const uint16_t*>(g.dY[s]);
        a.Q[s] = reinterpret_cast<const uint32_t*>(g.Q[s]);
        a.S[s] = reinterpret_cast<const uint16_t*>(g.S[s]);
        a.QM2[s] = reinterpret_cast<const uint32_t*>(g.QM2[s]);
    }
    a.offsets = reinterpret_cast<const int*>(g.offsets);
    a.row_weight = g.row_weight;
    a.dX = reinterpret_cast<uint16_t*>(g.dX);
    a.R = g.R; a.N = g.N; a.K = g.K; a.P = g.P; a.lg = g.lg; a.E = g.E;
    return a;
}

// The launch of either form for one bit width: kernel(T{}, int_c<TILEP>{}, pair as a type) names the instantiation - TileP
// 32 / 64 (3 bits: 32) x f16 / bf16 x single / pair -, lds its dynamic LDS (0: none; above 64 KB it has to be asked for - the
// attribute is per device and setting it is no stream operation: asked for at every launch, as moe_route.hip does).
template <int BITS, typename Kernel>
int grouped_ig_launch(const GroupedInputGrad& g, Kernel kernel, unsigned grid, int lds, const GroupedIgArgs& a, hipStream_t stream) {
    int rc = FLUTE_OK;
    const int err = dispatch_layout(g.dtype, BITS, g.tile_p, [&](auto t, auto bits, auto tp) {
        if constexpr (decltype(bits)::value == BITS) {  // the other widths live in their own units
            auto launch = [&](auto pr) {
                auto k = kernel(t, tp, pr);
                if (lds > 0 && hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
                    (void)hipGetLastError();
                    rc = FLUTE_ERR_LAUNCH;
                    return;
                }
                hipLaunchKernelGGL(k, dim3(grid), dim3(kIgThreads), lds, stream, a);
            };
            if (g.pair) launch(std::true_type{});
            else launch(std::false_type{});
        }
    });
    if (err != FLUTE_OK) return err;
    if (rc != FLUTE_OK) return rc;
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

// The slab form (inst_grouped_input_grad_b*.hip).  The grid is E x ceil(K / 128), from the shapes alone.
template <int BITS>
int qgemm_grouped_input_grad_launch(const GroupedInputGrad& g, hipStream_t stream) {
    GroupedIgArgs a = grouped_ig_args(g);
    a.slabs = (a.K + kIgKS - 1) / kIgKS;
    if ((long long)a.E * a.slabs > 0x7fffffffLL) return FLUTE_ERR_SHAPE;
    auto kernel = [](auto t, auto tp, auto pr) {
        return qgemm_grouped_input_grad_kernel<decltype(t), BITS, decltype(tp)::value, decltype(pr)::value>;
    };
    return grouped_ig_launch<BITS>(g, kernel, (unsigned)((long long)a.E * a.slabs), 0, a, stream);
}

}  // namespace flute_amd
