// The block form of the grouped input gradient: what qgemm_grouped_input_grad.h (the slab form) computes - same operands,
// same arithmetic, same bits - for experts with hundreds of rows, where the slab form's (expert, 128 k) workgroups read the
// expert's dY once per slab as 8-byte per-lane requests and feed 8 MFMAs from 8 transposed reads.  4 and 2 bits; 3 bits stay
// on the slab form (the decoder below would hold three planes of two octets in registers, and nothing asks for it).
//
// Work split.  A workgroup of 8 waves owns one 128-row block of one expert x one block of 256 k and walks all of N once, in
// the slab form's chunks of 64 columns (pair form: the first stack, then the second, into the same fp32 accumulators).  The
// row blocks are the forward block form's, found by grouped_rows.h's block map; the grid holds grouped_blocks_row_blocks(E, R)
// of them times K / 256: from (E, R, K) alone.  The k block is the fast index of blockIdx, so the workgroups in flight share
// a row block's dY.  A workgroup whose b is past the table's blocks returns before it requests a weight, scale or table word.
//
// Weights.  The slab form's decoder over twice the k: lane (unit ul < 64 / J, k-octet o < 16, field pair jp < J / 2) takes
// the octets o and o + 16 of the block - one 16-B request per octet - and writes fields 2 jp and 2 jp + 1 of each as 16 B
// to two rows of the [64 n][256 k] tile, tile row j * (64 / J) + ul being column unit_col0(u0 + ul) + j * TileP.  The pitch
// of 136 dwords (8 mod 64) spreads the eight rows of a half ds_read_b64_tr_b16 over all 64 banks, as in the slab form.
//
// dY.  Staged once per workgroup: the chunk's [128 rows][64 n] as 1024 16-B requests (two per lane; eight consecutive
// columns are eight consecutive tile rows: one 16-lane group's share of a 32-n step) into an LDS tile of pitch 36 dwords,
// read back as the B operand with one ds_read_b128 per row tile and step - the 16 rows of a read start 4 banks apart in a
// permutation of 16 slots: no conflict.  The slab form's fragment order has the odd lane groups take their second four
// tile rows first; the staging lane swaps the halves of those pieces, so the read needs no select.  Rows at or past the
// expert's end are not requested and staged as zeros.
//
// Both tiles are double buffered with ONE barrier per chunk (the slab form's protocol): chunk c is written into buffer
// c % 2 and read after the barrier, a wave reaches the writes of chunk c + 1 only behind the barrier of chunk c, which every
// wave passes after its reads of chunk c - 1.  The packed words, scales and dY of chunk c + 1 are requested before the
// MFMAs of chunk c.
//
// Wave w owns rows 64 (w / 4) .. + 63 and k 64 (w % 4) .. + 63 of the block: 4 x 4 accumulator tiles = 64 VGPRs; per
// 32-n step it issues 8 transposed reads, 4 ds_read_b128 and 16 MFMAs.  A wave whose 64 rows lie past the expert's end
// decodes, stages and keeps the barriers but issues no fragment read and no MFMA.
//
// The n order.  Chunks, steps and the position of every n inside a step's fragments are the slab form's, and an
// accumulator is one (row, k) in both: the two forms give EQUAL BITS on all inputs (tests/test_grouped_input_grad_blocks_gpu.py).
//
// LDS (dynamic, above 64 KB: one workgroup per CU): 2 x 34 KB weight tiles, 2 x 18 KB dY tiles, 8 KB of table copies per stack.
//
// Rows.  The contract on a malformed table is grouped_rows.h's.  Expert bases into Q / S / QM2 and row bases into dY / dX are
// 64-bit; there is no 32-bit descriptor.
#pragma once
#include "qgemm_grouped_input_grad.h"

namespace flute_amd {

constexpr int kIgbKB = 256;                                    // k per workgroup
constexpr int kIgbRB = kGroupedBlockRows;                      // rows per workgroup
constexpr int kIgbWPitch = kIgbKB * 2 + 32;                    // bytes per weight-tile row; 136 dwords = 8 mod 64
constexpr int kIgbWTile = kIgNC * kIgbWPitch;
constexpr int kIgbYPitch = kIgNC * 2 + 16;                     // bytes per dY-tile row; 36 dwords
constexpr int kIgbYTile = kIgbRB * kIgbYPitch;
constexpr int kIgbYAt = 2 * kIgbWTile;
constexpr int kIgbLutAt = kIgbYAt + 2 * kIgbYTile;
static_assert(kIgbRB == 128 && kIgbKB == 256, "the wave layout below is 2 row groups x 4 k quarters");

constexpr int grouped_ig_blocks_lds(bool pair) { return kIgbLutAt + (pair ? 2 : 1) * kIgLutWords * 4; }

static_assert(kIgbKB == kGroupedIgBlockK, "grouped_input_grad_blocks_eligible (grouped_rows.h) speaks of this k block");

template <typename T, int BITS, int TILEP, bool PAIR>
__global__ __launch_bounds__(kIgThreads) void qgemm_grouped_input_grad_blocks_kernel(const GroupedIgArgs a) {
    using L = Layout<BITS>;
    static_assert(BITS == 4 || BITS == 2, "3 bits stay on the slab form");
    constexpr int J = L::J;
    constexpr int NP = L::NPLANES;                                 // 1
    constexpr int UC = kIgNC / J;                                  // units per chunk: 16 / 8
    constexpr int NSTK = PAIR ? 2 : 1;
    constexpr int C = kIgLutCopies<BITS>;
    static_assert(UC % 8 == 0 && TILEP % UC == 0 && UC * 16 * (J / 2) == kIgThreads, "chunk shape");

    extern __shared__ __attribute__((aligned(16))) char igb_smem[];
    uint32_t* const lut_all = reinterpret_cast<uint32_t*>(igb_smem + kIgbLutAt);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.R, N = a.N, K = a.K, lg = a.lg;

    grouped_zero_unserved<kIgThreads>(a.dX, a.offsets, a.E, R, K);

    // ---- row block b -> (expert e, block of e, the expert's rows [rb, re)); the k block is the fast index
    const int kblocks = a.slabs;                                   // K / 256
    const int b = (int)blockIdx.x / kblocks;
    const int kb = ((int)blockIdx.x - b * kblocks) * kIgbKB;
    const GroupedBlock gb = grouped_block_map<kIgbRB>(a.offsets, a.E, R, b);
    const int e = gb.e, rb = gb.rb, re = gb.re;
    if (e < 0) return;                                             // b is past the table's blocks: nothing is requested
    const int row0 = rb + gb.blk * kIgbRB;                         // < re <= R

    const int K2 = K >> 1;
    const int G = K >> lg;
    const int NCH = N / kIgNC;                                     // chunks per stack
    const int NCC = NSTK * NCH;
    const size_t q_base = (size_t)e * (size_t)a.P * (size_t)K2;
    const size_t s_base = (size_t)e * (size_t)N * (size_t)G;

    ig_load_tables<BITS, NSTK>(lut_all, kIgLutWords, a, e);

    // ---- the lane as a decoder: unit ul of the chunk, k-octets o and o + 16 of the block, fields 2 jp and 2 jp + 1
    const int o = tid & 15;
    const int ul = (tid >> 4) % UC;
    const int jp = (tid >> 4) / UC;
    const int k0 = kb + 8 * o;                                     // the second octet: + 128; both < K (K % 256 == 0)
    const int lut_lane = lane % C;
    struct Packed {
        u32x4_t w[2][NP];                                          // [octet][plane]
        uint32_t s[2][2];                                          // [octet][field]
    };
    auto load_packed = [&](Packed& pk, int cc) {
        const bool in = cc < NCC;
        const int st = PAIR ? (cc >= NCH) : 0;
        const int u = (cc - st * NCH) * UC + ul;
        const uint32_t* __restrict__ Qs = a.Q[st] + q_base + (size_t)unit_row<BITS, TILEP>(u, 0, N) * K2 + (k0 >> 1);
        const uint16_t* __restrict__ Ss = a.S[st] + s_base;
        const int n0 = unit_col0<BITS, TILEP>(u);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            pk.w[hh][0] = in ? *reinterpret_cast<const u32x4_t*>(Qs + 64 * hh) : u32x4_t{0, 0, 0, 0};
            const int gi = (k0 + 128 * hh) >> lg;
#pragma unroll
            for (int f = 0; f < 2; ++f) pk.s[hh][f] = in ? (uint32_t)Ss[(size_t)(n0 + (2 * jp + f) * TILEP) * G + gi] : 0u;
        }
    };
    auto decode = [&](const Packed& pk, int cc) {
        char* dst = igb_smem + (cc & 1) * kIgbWTile + o * 16;
        const uint32_t* lt = lut_all + (PAIR ? (cc >= NCH) : 0) * kIgLutWords + lut_lane;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) ig_decode_octet<T, BITS, kIgbWPitch>(pk.w[hh], pk.s[hh], lt, jp, ul, true, dst + hh * 256);
    };

    // ---- the lane as a stager of dY: pieces (row yr + 64 t, tile rows 8 pc .. 8 pc + 7), t < 2
    const int pc = tid & 7, yr = tid >> 3;
    const int y_col = ((8 * pc) / UC) * TILEP + (8 * pc) % UC;     // from the chunk's first column
    const bool y_swap = pc & 1;                                    // an odd lane group's fragment: second four tile rows first
    bool yin[2];
    size_t yrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int row = row0 + yr + 64 * t;
        yin[t] = row < re;
        yrow[t] = (size_t)(yin[t] ? row : rb) * (size_t)N + y_col;     // < re <= R
    }
    struct Rows {
        uint4 y[2];
    };
    auto load_rows = [&](Rows& rw, int cc) {
        const int st = PAIR ? (cc >= NCH) : 0;
        const uint16_t* __restrict__ Yp = a.dY[st] + unit_col0<BITS, TILEP>((cc - st * NCH) * UC);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            rw.y[t] = (yin[t] && cc < NCC) ? *reinterpret_cast<const uint4*>(Yp + yrow[t]) : make_uint4(0, 0, 0, 0);
    };
    auto store_rows = [&](const Rows& rw, int cc) {
        char* dst = igb_smem + kIgbYAt + (cc & 1) * kIgbYTile + yr * kIgbYPitch + pc * 16;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 v = rw.y[t];
            *reinterpret_cast<uint4*>(dst + t * 64 * kIgbYPitch) = y_swap ? make_uint4(v.z, v.w, v.x, v.y) : v;
        }
    };

    // ---- the lane in the MFMAs: rows 64 rg .. + 63 of the row block, k 64 kq .. + 63 of the k block
    const int rg = wave >> 2, kq = wave & 3;
    const int h = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3, r16 = lane & 15;
    const bool active = row0 + 64 * rg < re;                       // wave-uniform
    const uint32_t tbase = lds_base_of(igb_smem);
    uint32_t a_addr[2];                                            // the two transposed reads of step 0, k tile 0, buffer 0
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
        a_addr[hf] = tbase + (8 * h + 4 * (hf ^ (h & 1)) + qq) * kIgbWPitch + (kq * 64 + 4 * p) * 2;
    const uint32_t y_addr = tbase + kIgbYAt + (64 * rg + r16) * kIgbYPitch + h * 16;   // row tile 0, step 0, buffer 0

    f32x4_t acc[4][4];                                             // [k tile][row tile]
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[kt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    Packed pk;
    Rows rw;
    load_packed(pk, 0);
    load_rows(rw, 0);
    for (int cc = 0; cc < NCC; ++cc) {
        decode(pk, cc);
        store_rows(rw, cc);
        Packed pk_next;
        Rows rw_next;
        load_packed(pk_next, cc + 1);                              // past the end: no request, zeros
        load_rows(rw_next, cc + 1);
        __syncthreads();
        if (active) {
            const uint32_t wbuf = (cc & 1) * kIgbWTile, ybuf = (cc & 1) * kIgbYTile;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                u32x4_t af[4], bf[4];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) af[kt] = ig_a_fragment(a_addr, wbuf + s * 32 * kIgbWPitch + kt * 32);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint4 y = lds_ld128(y_addr + ybuf + t * 16 * kIgbYPitch + s * 64);
                    bf[t] = u32x4_t{y.x, y.y, y.z, y.w};
                }
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[kt][t] = Mfma<T>::run(af[kt], bf[t], acc[kt][t]);
            }
        }
        pk = pk_next;
        rw = rw_next;
    }

    // lane (q = h, r = r16) of tile (kt, t): row row0 + 64 rg + 16 t + r, k = kb + 64 kq + 16 kt + 4 q .. + 3
    if (!active) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row = row0 + 64 * rg + 16 * t + r16;
        if (row < re) ig_store_row<T, PAIR>(a, acc, t, row, kb + kq * 64 + 4 * h);       // k < K
    }
}

// The launch of one bit width (inst_grouped_input_grad_blocks_b*.hip).  The grid is grouped_blocks_row_blocks(E, R) x K / 256,
// from the shapes alone; the caller has checked grouped_input_grad_blocks_eligible.
template <int BITS>
int qgemm_grouped_input_grad_blocks_launch(const GroupedInputGrad& g, hipStream_t stream) {
    GroupedIgArgs a = grouped_ig_args(g);
    a.slabs = a.K / kIgbKB;
    auto kernel = [](auto t, auto tp, auto pr) {
        return qgemm_grouped_input_grad_blocks_kernel<decltype(t), BITS, decltype(tp)::value, decltype(pr)::value>;
    };
    return grouped_ig_launch<BITS>(g, kernel, (unsigned)(grouped_blocks_row_blocks(a.E, a.R) * a.slabs), grouped_ig_blocks_lds(g.pair),
                                   a, stream);
}

}  // namespace flute_amd
