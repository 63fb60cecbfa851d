// The 256-row block form of the grouped input gradient for stacks of 3-bit experts: what qgemm_grouped_input_grad_w3_blocks.h
// (the 3-bit 128-row block form) and qgemm_grouped_input_grad.h (the slab form) compute at 3 bits - same operands, same
// arithmetic, same bits - for experts with many hundreds of rows, where the 128-row form decodes its [N x 256 k] panel once per
// 128 rows.  The work split, the buffers and the wave layout are qgemm_grouped_input_grad_blocks256.h's (4 / 2 bits); the decoder
// is the 3-bit 128-row form's; the staging of dY is that form's two 8-byte requests per piece, extended to 256 rows.
//
// Work split.  A workgroup of 8 waves owns one 256-row block of one expert x one block of 256 k and walks all of N once, in
// the slab form's chunks of 64 columns (pair form: the first stack, then the second, into the same fp32 accumulators).  The
// row blocks are grouped_rows.h's block map at 256 rows; the grid holds grouped_blocks256_row_blocks(E, R) of them times
// K / 256: from (E, R, K) alone.  The k block is the fast index of blockIdx, so the workgroups in flight share a row block's
// dY.  A workgroup whose b is past the table's blocks returns before it requests a weight, scale or table word.
//
// Weights.  Lane (unit ul < 4, k-octet o < 32 of the 256-k block, field quad jq < 4), jq = wave / 2 and so uniform in a wave:
// three 16-B plane requests for ONE octet, four scale requests, the fields 4 jq .. 4 jq + 3 by field_rt<3> - the sixteenth
// field, assembled from the top two bits of all three words, is a scalar branch that the jq == 3 waves alone take - and 16 B
// to each of the four tile rows j * 4 + ul of the [64 n][256 k] tile at pitch 136 dwords, which ig_a_fragment reads back
// transposed.  A decoded fragment feeds 32 MFMAs per 32-n step where the 128-row form's feeds 16.
//
// dY.  The chunk's [256 rows][64 n] at pitch 36 dwords.  A piece (row yr + 64 t, tile rows 8 pc .. 8 pc + 7), t < 4, is two
// runs of four consecutive columns, TileP apart: two 8-byte requests, placed as one 16-byte LDS write with the halves swapped
// for odd pieces, so the B fragments are one ds_read_b128 per row tile and step with no select.  Rows at or past the expert's
// end are not requested and are staged as zeros.  (A stager that asks for 16 B and keeps the second 8 for the following chunk
// was weighed and not built - DESIGN.md 3.3y: the kept halves of a chunk are 32 KB, the pair form's LDS map has 4 KB to spare,
// and in registers they are live across a chunk's MFMAs on top of the 128 accumulators.)
//
// Both tiles are double buffered with ONE barrier per chunk (the slab form's protocol); the packed words, scales and dY of
// chunk c + 1 are requested before the MFMAs of chunk c.
//
// Wave w owns rows 128 (w / 4) .. + 127 and k 64 (w % 4) .. + 63 of the block: 8 row tiles x 4 k tiles = 128 accumulator
// VGPRs; per 32-n step it issues 8 transposed reads, 8 ds_read_b128 and 32 MFMAs - the row tiles in two halves of four, so
// that four B fragments are live at a time.  A wave whose 128 rows lie past the expert's end decodes, stages and keeps the
// barriers but issues no fragment read and no MFMA.
//
// The n order.  Chunks, steps and the position of every n inside a step's fragments are the slab form's, and an accumulator
// is one (row, k) in all forms: EQUAL BITS on all inputs (tests/test_grouped_input_grad_w3_blocks256_gpu.py).
//
// LDS (dynamic; one workgroup per CU): qgemm_grouped_input_grad_blocks256.h's map - 2 x 34 KB weight tiles, 2 x 36 KB dY tiles,
// 8 KB of table copies per stack (the 3-bit image is 64 entries x 32 copies): 148 KB single, 156 KB pair.
//
// Registers (the compiler's resource report at gfx950, 512 threads, the four instantiations): 246 VGPRs fp16 single, 244 the other
// three, of the 256 that two waves per SIMD have; no AGPRs; NO SCRATCH - 128 accumulators, one chunk of packed words, scales and dY
// in flight, 4 A and 4 B fragments.  The Makefile fails the build of the unit on a spill.
//
// Measured (profiles/grouped_moe_input_grad_blocks256_w3.json): 5 - 7 % faster than the 3-bit 128-row form on Mixtral's
// down projection from a mean of 1024 rows per expert, not faster on gate / up, 1.6 - 1.8 x slower on E 64 2048 x 2048: the query
// never answers this form, a caller opts in.
//
// Rows.  The contract on a malformed table is grouped_rows.h's.  Expert bases into Q / S / QM2 and row bases into dY / dX are
// 64-bit; there is no 32-bit descriptor.
#pragma once
#include "qgemm_grouped_input_grad_blocks256.h"

namespace flute_amd {

template <typename T, int TILEP, bool PAIR>
__global__ __launch_bounds__(kIgThreads) void qgemm_grouped_input_grad_w3_blocks256_kernel(const GroupedIgArgs a) {
    using L = Layout<3>;
    constexpr int J = L::J;                                        // 16
    constexpr int NP = L::NPLANES;                                 // 3
    constexpr int UC = kIgNC / J;                                  // units per chunk: 4
    constexpr int FQ = 4;                                          // fields per lane
    constexpr int NSTK = PAIR ? 2 : 1;
    constexpr int C = kIgLutCopies<3>;
    static_assert(UC == 4 && TILEP % UC == 0 && UC * (kIgbKB / 8) * (J / FQ) == kIgThreads, "chunk shape");
    static_assert(L::LUT_N * C == kIgLutWords, "the table image fills grouped_ig_blocks256_lds's share");

    extern __shared__ __attribute__((aligned(16))) char igc3_smem[];
    uint32_t* const lut_all = reinterpret_cast<uint32_t*>(igc3_smem + kIgcLutAt);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.R, N = a.N, K = a.K, lg = a.lg;

    grouped_zero_unserved<kIgThreads>(a.dX, a.offsets, a.E, R, K);

    // ---- row block b -> (expert e, block of e, the expert's rows [rb, re)); the k block is the fast index
    const int kblocks = a.slabs;                                   // K / 256
    const int b = (int)blockIdx.x / kblocks;
    const int kb = ((int)blockIdx.x - b * kblocks) * kIgbKB;
    const GroupedBlock gb = grouped_block_map<kIgcRB>(a.offsets, a.E, R, b);
    const int e = gb.e, rb = gb.rb, re = gb.re;
    if (e < 0) return;                                             // b is past the table's blocks: nothing is requested
    const int row0 = rb + gb.blk * kIgcRB;                         // < re <= R

    const int K2 = K >> 1;
    const int G = K >> lg;
    const int NCH = N / kIgNC;                                     // chunks per stack
    const int NCC = NSTK * NCH;
    const size_t q_base = (size_t)e * (size_t)a.P * (size_t)K2;
    const size_t s_base = (size_t)e * (size_t)N * (size_t)G;

    ig_load_tables<3, NSTK>(lut_all, kIgLutWords, a, e);

    // ---- the lane as a decoder: unit ul of the chunk, k-octet o of the block, fields 4 jq .. 4 jq + 3 (jq: wave / 2)
    const int o = tid & 31;
    const int ul = (tid >> 5) & (UC - 1);
    const int jq = wave >> 1;
    const int k0 = kb + 8 * o;                                     // < K (K % 256 == 0)
    const int gi = k0 >> lg;
    const int lut_lane = lane % C;
    struct Packed {
        u32x4_t w[NP];
        uint32_t s[FQ];
    };
    auto load_packed = [&](Packed& pk, int cc) {
        const bool in = cc < NCC;
        const int st = PAIR ? (cc >= NCH) : 0;
        const int u = (cc - st * NCH) * UC + ul;
        const uint32_t* __restrict__ Qs = a.Q[st] + q_base + (k0 >> 1);
        const uint16_t* __restrict__ Ss = a.S[st] + s_base + gi;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
            pk.w[pl] = in ? *reinterpret_cast<const u32x4_t*>(Qs + (size_t)unit_row<3, TILEP>(u, pl, N) * K2) : u32x4_t{0, 0, 0, 0};
        const int n0 = unit_col0<3, TILEP>(u);
#pragma unroll
        for (int f = 0; f < FQ; ++f) pk.s[f] = in ? (uint32_t)Ss[(size_t)(n0 + (FQ * jq + f) * TILEP) * G] : 0u;
    };
    auto decode = [&](const Packed& pk, int cc) {
        char* dst = igc3_smem + (cc & 1) * kIgbWTile + (FQ * jq * UC + ul) * kIgbWPitch + o * 16;
        const uint32_t* lt = lut_all + (PAIR ? (cc >= NCH) : 0) * kIgLutWords + lut_lane;
#pragma unroll
        for (int f = 0; f < FQ; ++f) {
            const int j = FQ * jq + f;                             // scalar
            uint32_t v[4], out[4];
            if (f == FQ - 1 && jq == J / FQ - 1) {                 // field 15: the top two bits of the three words
#pragma unroll
                for (int d = 0; d < 4; ++d) v[d] = lt[field_rt<3>(pk.w[0][d], pk.w[1][d], pk.w[2][d], J - 1) * C];
            } else {
                __builtin_assume(j != J - 1);
#pragma unroll
                for (int d = 0; d < 4; ++d) v[d] = lt[field_rt<3>(pk.w[0][d], pk.w[1][d], pk.w[2][d], j) * C];
            }
            Num<T>::mul_scale4(v, pk.s[f], out);
            *reinterpret_cast<uint4*>(dst + f * UC * kIgbWPitch) = make_uint4(out[0], out[1], out[2], out[3]);
        }
    };

    // ---- the lane as a stager of dY: pieces (row yr + 64 t, tile rows 8 pc .. 8 pc + 7), t < 4; tile rows 8 pc .. + 3 are the
    // columns 2 pc TileP .. + 3 from the chunk's first, tile rows 8 pc + 4 .. + 7 the columns (2 pc + 1) TileP .. + 3
    const int pc = tid & 7, yr = tid >> 3;
    const int y_col = 2 * pc * TILEP;
    const bool y_swap = pc & 1;                                    // an odd lane group's fragment: second four tile rows first
    const int yrows = re - (row0 + yr);                            // piece t is inside the expert where 64 t < yrows
    const size_t yrow = (size_t)(row0 + yr) * (size_t)N + y_col;   // piece t: + 64 t N, an address only where the row is < re <= R
    struct Rows {
        uint2 y[4][2];                                             // [row][run]
    };
    auto load_rows = [&](Rows& rw, int cc) {
        const int st = PAIR ? (cc >= NCH) : 0;
        const uint16_t* __restrict__ Yp = a.dY[st] + unit_col0<3, TILEP>((cc - st * NCH) * UC);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
                rw.y[t][hf] = (64 * t < yrows && cc < NCC)
                                  ? *reinterpret_cast<const uint2*>(Yp + yrow + (size_t)(64 * t) * (size_t)N + hf * TILEP)
                                  : make_uint2(0, 0);
    };
    auto store_rows = [&](const Rows& rw, int cc) {
        char* dst = igc3_smem + kIgcYAt + (cc & 1) * kIgcYTile + yr * kIgbYPitch + pc * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint2 lo = rw.y[t][0], hi = rw.y[t][1];
            *reinterpret_cast<uint4*>(dst + t * 64 * kIgbYPitch) = y_swap ? make_uint4(hi.x, hi.y, lo.x, lo.y)
                                                                          : make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
    };

    // ---- the lane in the MFMAs: rows 128 rg .. + 127 of the row block, k 64 kq .. + 63 of the k block
    const int rg = wave >> 2, kq = wave & 3;
    const int h = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3, r16 = lane & 15;
    const bool active = row0 + 128 * rg < re;                      // wave-uniform
    const uint32_t tbase = lds_base_of(igc3_smem);
    uint32_t a_addr[2];                                            // the two transposed reads of step 0, k tile 0, buffer 0
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
        a_addr[hf] = tbase + (8 * h + 4 * (hf ^ (h & 1)) + qq) * kIgbWPitch + (kq * 64 + 4 * p) * 2;
    const uint32_t y_addr = tbase + kIgcYAt + (128 * rg + r16) * kIgbYPitch + h * 16;   // row tile 0, step 0, buffer 0

    f32x4_t acc[4][8];                                             // [k tile][row tile]
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[kt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    Packed pk;
    Rows rw;
    load_packed(pk, 0);
    load_rows(rw, 0);
    for (int cc = 0; cc < NCC; ++cc) {
        decode(pk, cc);
        store_rows(rw, cc);
        load_packed(pk, cc + 1);                                   // past the end: no request, zeros
        load_rows(rw, cc + 1);
        __syncthreads();
        if (active) {
            const uint32_t wbuf = (cc & 1) * kIgbWTile, ybuf = (cc & 1) * kIgcYTile;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                u32x4_t af[4];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) af[kt] = ig_a_fragment(a_addr, wbuf + s * 32 * kIgbWPitch + kt * 32);
#pragma unroll
                for (int th = 0; th < 2; ++th) {                   // row tiles 4 th .. 4 th + 3
                    u32x4_t bf[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const uint4 y = lds_ld128(y_addr + ybuf + (4 * th + t) * 16 * kIgbYPitch + s * 64);
                        bf[t] = u32x4_t{y.x, y.y, y.z, y.w};
                    }
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[kt][4 * th + t] = Mfma<T>::run(af[kt], bf[t], acc[kt][4 * th + t]);
                }
            }
        }
    }

    // lane (q = h, r = r16) of tile (kt, t): row row0 + 128 rg + 16 t + r, k = kb + 64 kq + 16 kt + 4 q .. + 3
    if (!active) return;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int row = row0 + 128 * rg + 16 * t + r16;
        if (row < re) ig_store_row<T, PAIR>(a, acc, t, row, kb + kq * 64 + 4 * h);       // k < K
    }
}

// The launch (inst_grouped_input_grad_blocks256_b3.hip).  The grid is grouped_blocks256_row_blocks(E, R) x K / 256, from the shapes
// alone; the caller has checked grouped_input_grad_w3_blocks256_eligible.
inline int qgemm_grouped_input_grad_w3_blocks256_launch(const GroupedInputGrad& g, hipStream_t stream) {
    GroupedIgArgs a = grouped_ig_args(g);
    a.slabs = a.K / kIgbKB;
    auto kernel = [](auto t, auto tp, auto pr) {
        return qgemm_grouped_input_grad_w3_blocks256_kernel<decltype(t), decltype(tp)::value, decltype(pr)::value>;
    };
    return grouped_ig_launch<3>(g, kernel, (unsigned)(grouped_blocks256_row_blocks(a.E, a.R) * a.slabs), grouped_ig_blocks256_lds(g.pair),
                                a, stream);
}

}  // namespace flute_amd
