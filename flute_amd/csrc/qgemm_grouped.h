// Grouped qgemm for mixture-of-experts layers: Y[r, :] = X[r, :] @ W_e^T for the rows r in [offsets[e], offsets[e + 1]) of
// every expert e < E, ONE launch whose grid does not depend on how the rows are spread.  X [T, K] holds the rows sorted by
// expert, offsets [E + 1] int32 lives in device memory and is read by the kernel only (never by the host: the launch is
// hipGraph-capturable and a replay honours whatever the table then holds), Q [E, P, K] / S [E, N, K / g] / QM2 [E, 4^b] are E
// layers packed exactly as one FluteLinear's buffers (layout: common.h), all of one num_bits / group size / TileP.
//
// One kernel template, three epilogues (GroupedMode):
//
//   Plain     Y[r, :] = round_T( acc32 ); rows no expert covers are left unwritten.
//   Glu       H[r, :] = round_T( silu32(g) * u ),  g = Xsrc[rows[r]] @ Wgate_e^T,  u = Xsrc[rows[r]] @ Wup_e^T: one launch
//             instead of two grouped launches, a gather, silu and a multiply.  g, u are the fp32 sums after the
//             in-workgroup K reduction, silu32(g) = g / (1 + exp(-g)) in fp32 (silu32() below), one rounding to T at the store.
//   Weighted  Y[r, :] = round_T( row_weight[r] * acc32 ), one rounding, and the rows [clamp(offsets[E]), T) - rows no
//             expert serves - written as zeros by the same launch whichever experts have rows.
//
// What a mode adds sits under `if constexpr`; everything else is one program text, so Plain is Weighted without the zero
// fill and without the multiply.
//
// Arithmetic (include/flute_amd.h, as dequant.hip and the MFMA kernels): w^ = round_T(lut * s) by Num<T>::mul_scale4, fp32
// accumulation in the matrix core, one rounding of the output to T.  K is split over the waves of ONE workgroup only and
// the partial tiles are summed through LDS in wave order; no atomics, no split across workgroups: equal arguments give
// equal bits.
//
// Geometry (qgemm_skinny.h's, for every bit width through Layout / unit_row / unit_col0 / field).  v_mfma_f32_16x16x32 with
// the weights as the A operand: lane (u = l % 16, q = l / 16) loads, per plane, the 16 B of unit row u that hold k-pairs
// 4 q .. 4 q + 3 of a 32-k step; field j of each dword is looked up in the expert's pair table (LDS, 32 copies: lane l reads
// copy l % 32, so the 32 lanes of a ds_read_b32 group never share a bank) and multiplied by the scale of column
// unit_col0(u) + j TileP: one A fragment per column tile j < J.  The activations are the B operand: lane (r, q) loads its
// 16 B of row row0 + 16 t + r.  One weight request feeds J x (row tiles of the pass) MFMAs.  D[u][r] lands in lane (q, r) as
// units 4 q .. 4 q + 3 - four consecutive output columns, one 8-byte store per tile.
//
// Work split.  A workgroup is (expert, a run of `spw` 16-unit slabs); its 8 waves split K in blocks of U k-steps (U = 4,
// 128 k; 2 bits below group size 128: 2; 3 bits: 1), wave w taking blocks w, w + 8, ..: at any moment the waves of a
// workgroup read one contiguous 0.5 - 2 KB piece of each of the 16 unit rows.  A wave holds the next block's weights and
// activations in registers while it decodes the current one (plain loads: the compiler counts the waits).  The scales go
// through LDS: per K chunk the workgroup stages the slab's panel [16 J columns][groups of the chunk] with requests that run
// along a scale row (64 groups = one cache line per request; read per lane from global memory they were 2-byte requests
// touching 16 lines each, 9 - 21 % of the time at Mixtral shapes), in the 32 KB the reduction uses after the K loop; the
// row stride in dwords is odd, so the 16 units of a ds_read_u16 hit 16 banks.  A chunk is the largest multiple of 8 blocks
// whose groups fit (all of K up to 16 K at 4 bits and group size 64).  The expert index is the slow one of blockIdx
// (e = blockIdx / runs): consecutive blocks go to different XCDs, so the slabs of ONE busy expert spread over all eight
// dies - with the expert as the fast index a decode step that routes to two experts would run on two dies.
// The host picks spw in {1, 2, 4} as the largest that still leaves eight workgroups per CU; it and the grid follow from
// (E, N, num_bits, num_sms) alone, as include/flute_amd.h says (grouped_grid() below, the only place they are computed).
//
// Rows.  [rb, re) of the expert and the contract on a malformed table: grouped_rows.h.  The expert's rows are taken in
// passes of RT 16-row tiles (RT = 2; 3 bits: 1 - the accumulators, J x RT x 4 fp32, and two blocks of operands stay in
// registers, no scratch), the weights streamed once per pass; a tile of a pass that holds no row issues neither loads nor
// MFMAs (the K loop is compiled per tile count), rows past `re` inside a tile are fed as zeros and never stored.
//
// Glu.  A workgroup serves slab s of the gate stack and slab s of the up stack for the same rows: the K loop and the
// reduction run for the gate slab, waves 0 .. TR - 1 keep their reduced tiles in registers (NI / TR float4 per lane: 2 at
// 4 bits, 4 at 2 and 3 bits), the K loop and the reduction run again for the up slab, and the same lanes combine and
// store.  Both pair tables sit in LDS (4 bits: 2 x 32 KB beside the 32 KB of the reduction).  The activation rows are
// read through `rows` (int32, each entry clamped to [0, Tsrc) before it forms an address; null: row r is r) - the only
// place the index is used.
//
// Address arithmetic: the expert bases into Q / S / QM2 and the row bases into X / Y are 64-bit (stacked 8192 x 8192 4-bit
// experts pass 2 GiB of codes at E = 64).
#pragma once
#include "kernels.h"
#include "grouped_rows.h"
#include "mfma.h"
#include "silu32.h"
#include <type_traits>
#include "layout_dispatch.h"

namespace flute_amd {

enum class GroupedMode { Plain, Glu, Weighted };

constexpr int kGroupedWaves = 8;
constexpr int kGroupedThreads = kGroupedWaves * 64;
constexpr int kGroupedRedTiles = 4;          // output tiles per round of the LDS reduction (8 waves x 4 KB = 32 KB)

// Sized so that the accumulators (J x RT x 4 fp32) and two blocks of operands fit in 256 registers without scratch.
// LGC (2 bits only; 7 otherwise): 5 / 6 = log2(group size), 7 = group size >= 128
template <int BITS, int LGC> struct GroupedShape {
    static constexpr int RT = (BITS == 3) ? 1 : 2;                                           // 16-row tiles per pass
    static constexpr int U = (BITS == 3) ? 1 : (BITS == 2 && LGC < 7) ? 2 : 4;               // k-steps per block
};

// (silu32() and its error account: silu32.h, shared with the block form of the Glu mode, qgemm_block2.h GM = 3)

struct GroupedArgs {
    const uint16_t* X;          // [Tsrc, K] T
    const int* rows;            // [R] or null (Glu only)
    const int* offsets;         // [E + 1]
    const uint32_t* Q[2];       // [E, P, K / 2]: the stack (Glu: gate, up)
    const uint16_t* S[2];       // [E, N, K / g]
    const uint32_t* QM2[2];     // [E, 4^b]
    const float* row_weight;    // [R] (Weighted only)
    uint16_t* Y;                // [R, N]
    int R, Tsrc, N, K, P, lg, runs, spw, E;
};

// The kernel's arguments from the launch's named operands; runs / spw are the launch's to set.
inline GroupedArgs grouped_args(const GroupedForward& g) {
    GroupedArgs a{};
    a.X = reinterpret_cast<const uint16_t*>(g.X);
    a.rows = reinterpret_cast<const int*>(g.rows);
    a.offsets = reinterpret_cast<const int*>(g.offsets);
    for (int s = 0; s < 2; ++s) {
        a.Q[s] = reinterpret_cast<const uint32_t*>(g.Q[s]);
        a.S[s] = reinterpret_cast<const uint16_t*>(g.S[s]);
        a.QM2[s] = reinterpret_cast<const uint32_t*>(g.QM2[s]);
    }
    a.row_weight = g.row_weight;
    a.Y = reinterpret_cast<uint16_t*>(g.Y);
    a.R = g.R; a.Tsrc = g.Tsrc; a.N = g.N; a.K = g.K; a.P = g.P; a.lg = g.lg; a.E = g.E;
    return a;
}

template <typename T, int BITS, int TILEP, int LGC, GroupedMode MODE>
__global__ __launch_bounds__(kGroupedThreads) void qgemm_grouped_kernel(const GroupedArgs a) {
    using L = Layout<BITS>;
    using NT = Num<T>;
    constexpr bool GLU = MODE == GroupedMode::Glu;
    constexpr int J = L::J;
    constexpr int NP = L::NPLANES;
    constexpr int RT = GroupedShape<BITS, LGC>::RT;
    constexpr int U = GroupedShape<BITS, LGC>::U;
    constexpr int NI = J * RT;                                     // 16 x 16 output tiles per wave
    constexpr int KW = kGroupedWaves;
    constexpr int TR = kGroupedRedTiles;
    constexpr int NC = 16 * J;                                     // columns of a slab
    constexpr int NSTK = GLU ? 2 : 1;                              // weight stacks
    // scale panel of a K chunk: [NC][ST] T in the reduction's LDS; ST / 2 is odd, so the 16 units of a ds_read_u16 hit 16 banks
    constexpr int ST = (int)(KW * TR * 64 * sizeof(float4) / 2) / NC - 2;
    static_assert(NI % TR == 0 && (ST / 2) % 2 == 1 && ST >= 16, "reduction / panel shape");

    __shared__ uint32_t lut[NSTK][L::LUT_N * 32];
    __shared__ float4 red[KW * TR * 64];

    const int tid = threadIdx.x;
    const int R = a.R, N = a.N, K = a.K, lg = a.lg;
    uint16_t* __restrict__ Y = a.Y;

    if constexpr (MODE == GroupedMode::Weighted) grouped_zero_unserved<kGroupedThreads>(Y, a.offsets, a.E, R, N);

    const int e = (int)blockIdx.x / a.runs;
    const int run = (int)blockIdx.x - e * a.runs;
    const GroupedRows er = grouped_rows(a.offsets, e, R);
    if (er.empty()) return;                                        // no rows: nothing of this expert is requested
    const int rb = er.rb, re = er.re;

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u = lane & 15, q = lane >> 4;
    const int K2 = K >> 1;
    const int G = K >> lg;
    const int NS = K >> 5;                                         // k-steps
    const int NB = (NS + U - 1) / U;                               // blocks (the last one may be short: K % 64 == 0 only)
    const int slabs = (N / J) >> 4;
    const size_t q_base = (size_t)e * (size_t)a.P * (size_t)K2;
    const size_t s_base = (size_t)e * (size_t)N * (size_t)G;

    // table images: entry i of copy c at word i * 32 + c
#pragma unroll
    for (int s = 0; s < NSTK; ++s) {
        const uint32_t* __restrict__ Te = a.QM2[s] + (size_t)e * L::LUT_N;
        for (int i = tid; i < L::LUT_N * 32; i += kGroupedThreads) lut[s][i] = Te[i >> 5];
    }
    __syncthreads();
    uint16_t* panel = reinterpret_cast<uint16_t*>(red);
    // blocks per chunk: a multiple of KW whose groups (+ 2 for ragged ends) fit ST
    const int bpc = ((((ST - 2) << lg) / (U * 32)) / KW) * KW;

    for (int sl = 0; sl < a.spw; ++sl) {
        const int slab = run * a.spw + sl;
        if (slab >= slabs) break;
        const int unit = slab * 16 + u;
        size_t woff[NP];                                           // the lane's place in a plane, the same in both stacks
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) woff[pl] = q_base + (size_t)unit_row<BITS, TILEP>(unit, pl, N) * K2 + q * 4;

        for (int row0 = rb; row0 < re; row0 += 16 * RT) {
            const int nt = min(RT, (re - row0 + 15) >> 4);         // row tiles of this pass that hold a row
            const uint16_t* xrow[RT];
            bool xok[RT];
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const int row = row0 + 16 * t + u;
                xok[t] = row < re;
                int src = xok[t] ? row : rb;                       // < re <= R
                if constexpr (GLU) {
                    if (a.rows) src = min(max(a.rows[src], 0), a.Tsrc - 1);
                }
                xrow[t] = a.X + (size_t)src * K + q * 8;
            }

            f32x4_t acc[NI];

            // the K loop of a pass with NTC row tiles over stack s (a compile-time count: the accumulators of the tiles
            // without rows are never touched, and no MFMA sits behind a branch)
            auto k_loop = [&](auto nt_tag, auto s_tag) {
                constexpr int NTC = decltype(nt_tag)::value;
                constexpr int s = decltype(s_tag)::value;
                const uint32_t* __restrict__ Qs = a.Q[s];
                const uint16_t* __restrict__ Se = a.S[s] + s_base;
                const uint32_t* lut_lane = lut[s] + (lane & 31);
#pragma unroll
                for (int i = 0; i < NI; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                struct Block {
                    u32x4_t w[U][NP];
                    u32x4_t x[U][NTC];
                };
                // block b of this wave: k-steps b U .. b U + U - 1 (those < NS) while b lies in the chunk
                auto load_block = [&](Block& blk, int b, int cend) {
#pragma unroll
                    for (int i = 0; i < U; ++i) {
                        const int ks = b * U + i;
                        const bool in = b < cend && ks < NS;
#pragma unroll
                        for (int pl = 0; pl < NP; ++pl)
                            blk.w[i][pl] = in ? *reinterpret_cast<const u32x4_t*>(Qs + woff[pl] + ks * 16) : u32x4_t{0, 0, 0, 0};
#pragma unroll
                        for (int t = 0; t < NTC; ++t)
                            blk.x[i][t] = (in && xok[t]) ? *reinterpret_cast<const u32x4_t*>(xrow[t] + ks * 32)
                                                         : u32x4_t{0, 0, 0, 0};
                    }
                };
                // K in chunks of `bpc` blocks whose scale panel fits the LDS it shares with the reduction
                for (int cb = 0; cb < NB; cb += bpc) {
                    const int cend = min(NB, cb + bpc);
                    const int g_lo = (cb * U * 32) >> lg;
                    const int gc = min(G, ((cend * U * 32 - 1) >> lg) + 1) - g_lo;      // <= (bpc U 32 >> lg) + 2 <= ST
                    __syncthreads();                               // the panel's (or the reduction's) last readers are done
                    // panel[column tile j][unit u][group]: a wave stages whole scale rows, 64 consecutive groups per request
                    for (int ci = wave; ci < NC; ci += KW) {
                        const int col = unit_col0<BITS, TILEP>(slab * 16 + (ci & 15)) + (ci >> 4) * TILEP;
                        const uint16_t* src = Se + (size_t)col * G + g_lo;
                        for (int gg = lane; gg < gc; gg += 64) panel[ci * ST + gg] = src[gg];
                    }
                    __syncthreads();
                    const uint16_t* prow = panel + u * ST - g_lo;
                    Block cur;
                    load_block(cur, cb + wave, cend);
                    for (int b = cb + wave; b < cend; b += KW) {
                        Block nxt;
                        load_block(nxt, b + KW, cend);             // past the chunk: no request, zeros
#pragma unroll
                        for (int i = 0; i < U; ++i) {
                            const int ks = b * U + i;
                            if (ks < NS) {
                                const uint16_t* ps = prow + ((ks * 32) >> lg);
#pragma unroll
                                for (int j = 0; j < J; ++j) {
                                    uint32_t v[4], af4[4];
#pragma unroll
                                    for (int d = 0; d < 4; ++d) {
                                        uint32_t w[NP];
#pragma unroll
                                        for (int pl = 0; pl < NP; ++pl) w[pl] = cur.w[i][pl][d];
                                        v[d] = lut_lane[field<BITS>(w, j) << 5];
                                    }
                                    NT::mul_scale4(v, (uint32_t)ps[j * 16 * ST], af4);
                                    const u32x4_t af = {af4[0], af4[1], af4[2], af4[3]};
#pragma unroll
                                    for (int t = 0; t < NTC; ++t) acc[j * RT + t] = Mfma<T>::run(af, cur.x[i][t], acc[j * RT + t]);
                                }
                            }
                        }
                        cur = nxt;
                    }
                }
            };
            auto k_pass = [&](auto s) {
                if constexpr (RT == 1) {
                    k_loop(std::integral_constant<int, 1>{}, s);
                } else {
                    if (nt == 1) k_loop(std::integral_constant<int, 1>{}, s);
                    else k_loop(std::integral_constant<int, 2>{}, s);
                }
            };

            // K reduction inside the workgroup, TR tiles per round: tile i of a round is summed by wave i, in wave order,
            // and handed to `done(round, tile, sum)` in that wave
            auto reduce = [&](auto&& done) {
#pragma unroll
                for (int t0 = 0; t0 < NI; t0 += TR) {
                    __syncthreads();                               // the previous round's (or the panel's) readers are done
#pragma unroll
                    for (int i = 0; i < TR; ++i)
                        red[(wave * TR + i) * 64 + lane] = make_float4(acc[t0 + i][0], acc[t0 + i][1], acc[t0 + i][2], acc[t0 + i][3]);
                    __syncthreads();
                    if (wave < TR) {
                        float4 s = red[wave * 64 + lane];
                        for (int ww = 1; ww < KW; ++ww) {
                            const float4 p = red[(ww * TR + wave) * 64 + lane];
                            s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
                        }
                        done(t0 / TR, t0 + wave, s);
                    }
                }
            };
            // lane (q, r = u) of tile (j, t): row row0 + 16 t + r, units 4 q .. 4 q + 3 of the slab = four consecutive columns
            auto store = [&](int tile, float4 s) {
                const int j = tile / RT, t = tile % RT;
                const int row = row0 + 16 * t + u;
                if (row < re) {
                    if constexpr (MODE == GroupedMode::Weighted) {
                        const float w = a.row_weight[row];
                        s.x *= w; s.y *= w; s.z *= w; s.w *= w;
                    }
                    const int col = unit_col0<BITS, TILEP>(slab * 16 + 4 * q) + j * TILEP;
                    ushort4 o;
                    o.x = NT::from_float(s.x); o.y = NT::from_float(s.y); o.z = NT::from_float(s.z); o.w = NT::from_float(s.w);
                    *reinterpret_cast<ushort4*>(Y + (size_t)row * N + col) = o;
                }
            };

            if constexpr (GLU) {
                float4 gate[NI / TR];                              // the gate tiles this wave reduced (waves < TR)
                k_pass(std::integral_constant<int, 0>{});
                reduce([&](int round, int, float4 s) { gate[round] = s; });
                k_pass(std::integral_constant<int, 1>{});
                reduce([&](int round, int tile, float4 s) {
                    const float4 g = gate[round];
                    store(tile, make_float4(silu32(g.x) * s.x, silu32(g.y) * s.y, silu32(g.z) * s.z, silu32(g.w) * s.w));
                });
            } else {
                k_pass(std::integral_constant<int, 0>{});
                reduce([&](int, int tile, float4 s) { store(tile, s); });
            }
        }
    }
}

// spw, runs and the grid of a launch, from (E, N, num_bits, num_sms) alone: spw in {1, 2, 4} is the largest that still
// leaves eight workgroups per CU.  False: the grid does not fit 31 bits.
inline bool grouped_grid(int E, int N, int num_bits, int num_sms, int* spw_out, int* runs_out, unsigned* grid_out) {
    const int J = (num_bits == 3) ? 16 : 16 / num_bits;
    const int slabs = N / J / 16;
    const long long sms = num_sms >= 1 ? num_sms : 256;
    int spw = 1;
    while (spw < 4 && (long long)E * ((slabs + 2 * spw - 1) / (2 * spw)) >= 8 * sms) spw *= 2;
    const int runs = (slabs + spw - 1) / spw;
    if ((long long)E * runs > 0x7fffffffLL) return false;
    *spw_out = spw;
    *runs_out = runs;
    *grid_out = (unsigned)((long long)E * runs);
    return true;
}

// The launch of every form: the 18 instantiations of a mode (4 bits: TileP 32 / 64; 2 bits: TileP 32 / 64 x group size
// 32 / 64 / >= 128; 3 bits: TileP 32; each in f16 and bf16).
template <GroupedMode MODE>
int qgemm_grouped_launch(const GroupedForward& g, hipStream_t stream) {
    GroupedArgs a = grouped_args(g);
    unsigned grid;
    if (!grouped_grid(a.E, a.N, g.num_bits, g.num_sms, &a.spw, &a.runs, &grid)) return FLUTE_ERR_SHAPE;
    const int lg = a.lg;
    const int err = dispatch_layout(g.dtype, g.num_bits, g.tile_p, [&](auto t, auto bits, auto tp) {
        constexpr int B = decltype(bits)::value;
        auto launch = [&](auto lgc) {
            hipLaunchKernelGGL((qgemm_grouped_kernel<decltype(t), B, decltype(tp)::value, decltype(lgc)::value, MODE>),
                               dim3(grid), dim3(kGroupedThreads), 0, stream, a);
        };
        if constexpr (B == 2) {                         // only the 2-bit kernels take the group size as a constant
            if (lg == 5) launch(int_c<5>{});
            else if (lg == 6) launch(int_c<6>{});
            else launch(int_c<7>{});
        } else {
            launch(int_c<7>{});
        }
    });
    if (err != FLUTE_OK) return err;
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
