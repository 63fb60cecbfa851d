// The fused forms of the grouped qgemm (qgemm_grouped.hip) for a mixture-of-experts MLP, on that kernel's geometry:
//
//   GLU       H[r, :] = round_T( silu32(g) * u ),  g = Xsrc[rows[r]] @ Wgate_e^T,  u = Xsrc[rows[r]] @ Wup_e^T
//             for the rows r in [offsets[e], offsets[e + 1]) of every expert e: one launch instead of two grouped
//             launches, a gather, silu and a multiply.  g, u are the fp32 sums after the in-workgroup K reduction,
//             silu32(g) = g / (1 + exp(-g)) in fp32 (silu32() below), one rounding to T at the store.
//   weighted  Y[r, :] = round_T( row_weight[r] * acc32 ), one rounding, and the rows [clamp(offsets[E]), T) - rows no
//             expert serves - written as zeros by the same launch whichever experts have rows.
//
// This is a translation unit of its own on purpose: qgemm_grouped.hip is not touched, so every
// qgemm_grouped_kernel instantiation keeps its code and its bits.  What is shared is restated, not changed: Layout /
// unit_row / unit_col0 / field, the 8 waves that split K in interleaved blocks of U k-steps, the next block's
// operands held in registers, the scale panel staged per K chunk in the reduction's LDS, the pair table as 32 LDS
// copies, row passes of RT 16-row tiles with the K loop compiled per tile count, the reduction through LDS in wave
// order (no atomics, no split across workgroups: equal arguments give equal bits), 64-bit bases, the grid from
// (E, N, num_bits, num_sms) alone, and a workgroup whose expert has no rows requesting nothing.
//
// GLU.  A workgroup serves slab s of the gate stack and slab s of the up stack for the same rows: the K loop and the
// reduction run for the gate slab, waves 0 .. TR - 1 keep their reduced tiles in registers (NI / TR float4 per lane: 2 at
// 4 bits, 4 at 2 and 3 bits), the K loop and the reduction run again for the up slab, and the same lanes combine and
// store.  Both pair tables sit in LDS (4 bits: 2 x 32 KB beside the 32 KB of the reduction).  The activation rows are
// read through `rows` (int32, each entry clamped to [0, Tsrc) before it forms an address; null: row r is r) - the only
// place the index is used.
#pragma once
#include "kernels.h"
#include "mfma.h"
#include <type_traits>
#include "../../include/flute_amd.h"

namespace flute_amd {

constexpr int kFusedWaves = 8;
constexpr int kFusedThreads = kFusedWaves * 64;
constexpr int kFusedRedTiles = 4;            // output tiles per round of the LDS reduction (8 waves x 4 KB = 32 KB)

// qgemm_grouped.hip's GroupedShape: the accumulators (J x RT x 4 fp32) and two blocks of operands fit 256 registers
template <int BITS, int LGC> struct FusedShape {
    static constexpr int RT = (BITS == 3) ? 1 : 2;                                           // 16-row tiles per pass
    static constexpr int U = (BITS == 3) ? 1 : (BITS == 2 && LGC < 7) ? 2 : 4;               // k-steps per block
};

// silu32(g) = g / (1 + exp(-g)), fp32.  expf is within 1 ulp (2^-23 relative), the sum 1 + t and the quotient are
// correctly rounded (2^-24 each; IEEE division is hipcc's default), and an error of t enters 1 + t scaled by
// t / (1 + t) < 1: relative error <= 2^-23 + 2 * 2^-24 = 2^-22 to first order, for every |g| <= 88 (exp(88) is finite;
// exp(-88) underflows against the 1).  With the fp32 product by u (2^-24) behind it: eps_s = 2^-21 covers both.
__device__ __forceinline__ float silu32(float g) { return g / (1.0f + expf(-g)); }

struct GroupedFusedArgs {
    const uint16_t* X;          // [Tsrc, K] T
    const int* rows;            // [R] or null (GLU only)
    const int* offsets;         // [E + 1]
    const uint32_t* Q[2];       // [E, P, K / 2]: the stack (GLU: gate, up)
    const uint16_t* S[2];       // [E, N, K / g]
    const uint32_t* QM2[2];     // [E, 4^b]
    const float* row_weight;    // [R] (weighted only)
    uint16_t* Y;                // [R, N]
    int R, Tsrc, N, K, P, lg, runs, spw, E;
};

template <typename T, int BITS, int TILEP, int LGC, bool GLU>
__global__ __launch_bounds__(kFusedThreads) void qgemm_grouped_fused_kernel(const GroupedFusedArgs a) {
    using L = Layout<BITS>;
    using NT = Num<T>;
    constexpr int J = L::J;
    constexpr int NP = L::NPLANES;
    constexpr int RT = FusedShape<BITS, LGC>::RT;
    constexpr int U = FusedShape<BITS, LGC>::U;
    constexpr int NI = J * RT;                                     // 16 x 16 output tiles per wave
    constexpr int KW = kFusedWaves;
    constexpr int TR = kFusedRedTiles;
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

    if constexpr (!GLU) {
        // rows no expert serves, [clamp(offsets[E]), R): zeros, 8 bytes per lane, spread over the whole grid
        const int zb = min(max(a.offsets[a.E], 0), R);
        const size_t n4 = (size_t)(R - zb) * (size_t)(N >> 2);
        ushort4* z = reinterpret_cast<ushort4*>(Y + (size_t)zb * N);
        for (size_t i = (size_t)blockIdx.x * kFusedThreads + tid; i < n4; i += (size_t)gridDim.x * kFusedThreads)
            z[i] = ushort4{0, 0, 0, 0};
    }

    const int e = (int)blockIdx.x / a.runs;
    const int run = (int)blockIdx.x - e * a.runs;
    const int rb = min(max(a.offsets[e], 0), R);
    const int re = min(max(a.offsets[e + 1], 0), R);
    if (re <= rb) return;                                          // no rows: nothing of this expert is requested

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
        for (int i = tid; i < L::LUT_N * 32; i += kFusedThreads) lut[s][i] = Te[i >> 5];
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
                    if constexpr (!GLU) {
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

// The launch of either form: spw and the grid exactly as qgemm_grouped_dispatch picks them, from (E, N, num_bits, num_sms).
template <bool GLU>
int qgemm_grouped_fused_launch(int dtype, int num_bits, int tile_p, int lg, GroupedFusedArgs a, int num_sms, hipStream_t stream) {
    const int J = (num_bits == 3) ? 16 : 16 / num_bits;
    const int slabs = a.N / J / 16;
    const long long sms = num_sms >= 1 ? num_sms : 256;
    int spw = 1;
    while (spw < 4 && (long long)a.E * ((slabs + 2 * spw - 1) / (2 * spw)) >= 8 * sms) spw *= 2;
    a.spw = spw;
    a.runs = (slabs + spw - 1) / spw;
    if ((long long)a.E * a.runs > 0x7fffffffLL) return FLUTE_ERR_SHAPE;
    const unsigned grid = (unsigned)((long long)a.E * a.runs);
#define FLUTE_GRPF(TY, B, TP, LGC) \
    hipLaunchKernelGGL((qgemm_grouped_fused_kernel<TY, B, TP, LGC, GLU>), dim3(grid), dim3(kFusedThreads), 0, stream, a)
#define FLUTE_GRPF_L(TY, B, TP)                 \
    if (lg == 5) FLUTE_GRPF(TY, B, TP, 5);      \
    else if (lg == 6) FLUTE_GRPF(TY, B, TP, 6); \
    else FLUTE_GRPF(TY, B, TP, 7)
#define FLUTE_GRPF_T(B, TP)                               \
    if (dtype == FLUTE_F16) { FLUTE_GRPF_L(F16, B, TP); } \
    else { FLUTE_GRPF_L(BF16, B, TP); }
#define FLUTE_GRPF_7(B, TP)                                \
    if (dtype == FLUTE_F16) { FLUTE_GRPF(F16, B, TP, 7); } \
    else { FLUTE_GRPF(BF16, B, TP, 7); }
    if (num_bits == 4 && tile_p == 32) { FLUTE_GRPF_7(4, 32) }
    else if (num_bits == 4 && tile_p == 64) { FLUTE_GRPF_7(4, 64) }
    else if (num_bits == 2 && tile_p == 32) { FLUTE_GRPF_T(2, 32) }
    else if (num_bits == 2 && tile_p == 64) { FLUTE_GRPF_T(2, 64) }
    else if (num_bits == 3 && tile_p == 32) { FLUTE_GRPF_7(3, 32) }
    else return FLUTE_ERR_TEMPLATE_ID;
#undef FLUTE_GRPF_7
#undef FLUTE_GRPF_T
#undef FLUTE_GRPF_L
#undef FLUTE_GRPF
    return hipGetLastError() == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
}

}  // namespace flute_amd
