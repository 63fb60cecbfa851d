// The block form of the grouped input gradient for stacks of 3-bit experts: what qgemm_grouped_input_grad.h (the slab form)
// computes at 3 bits - same operands, same arithmetic, same bits - for experts with hundreds of rows.  The 4- / 2-bit block
// form (qgemm_grouped_input_grad_blocks.h) gives the work split, the buffers, the fragment reads and the epilogue; the decoder
// and the staging of dY are this file's own, because a 3-bit unit is 16 columns in three plane rows and a 64-column chunk is
// therefore UC = 4 units.
//
// Work split.  As the 4- / 2-bit block form: a workgroup of 8 waves owns one 128-row block of one expert x 256 k and walks all
// of N once in the slab form's chunks of 64 columns (pair form: the first stack, then the second, into the same fp32
// accumulators); grid = grouped_blocks_row_blocks(E, R) x K / 256 from the shapes alone, the k block the fast index; a
// workgroup whose b is past the table's blocks returns before it requests a weight, scale or table word.
//
// Weights.  Lane (unit ul < 4, k-octet o < 32 of the 256-k block, field quad jq < 4): 4 x 32 x 4 = 512 lanes, jq the slow
// index - it is tid / 128, the same in both waves of a SIMD pair and uniform in a wave, so a field's plane and shift are scalar
// and the sixteenth field, which is assembled from the top two bits of all three words, is a scalar branch that the jq == 3
// waves alone take.  A lane makes three 16-B plane requests for ONE octet and four scale requests, decodes the fields
// 4 jq .. 4 jq + 3 (32 lookups, the 4-bit block form's count) and writes 16 B to each of the four tile rows j * UC + ul.  The
// 4- / 2-bit mapping (two octets, one field pair) would hold 2 x 3 plane requests and have 8 lanes ask for every plane word;
// here 4 do, and the packed words and scales of two chunks are 32 VGPRs.  The tile is [64 n][256 k] at pitch 136 dwords in
// the slab form's row order: tile row j * 4 + ul is column unit_col0(u0 + ul) + j * TileP, and the A fragments are read by
// ig_a_fragment unchanged.  The 32 lanes of a (ul, jq) write 512 contiguous bytes of a tile row.
//
// dY.  With UC = 4 eight consecutive tile rows are two runs of four consecutive columns, TileP apart, so a piece (row, tile
// rows 8 pc .. 8 pc + 7) is two 8-byte requests where the 4- / 2-bit stager makes one of 16 bytes.  They land in the same LDS
// layout - pitch 36 dwords, the halves swapped for odd pieces - and the B fragments are one ds_read_b128 per row tile and step
// with no select.  A chunk takes 8 B of each 64-B line of a dY row and the eight chunks of a 512-column block use the line
// fully (DESIGN.md 3.3v has the measurement of what that costs).  Rows at or past the expert's end are not requested and are
// staged as zeros.
//
// Buffers, barriers, waves, the n order (EQUAL BITS to the slab form on all inputs: tests/test_grouped_input_grad_w3_blocks_gpu.py),
// LDS and the row contract: qgemm_grouped_input_grad_blocks.h.  The 3-bit table image is 64 entries x 32 copies = kIgLutWords.
#pragma once
#include "qgemm_grouped_input_grad_blocks.h"

namespace flute_amd {

template <typename T, int TILEP, bool PAIR>
__global__ __launch_bounds__(kIgThreads) void qgemm_grouped_input_grad_w3_blocks_kernel(const GroupedIgArgs a) {
    using L = Layout<3>;
    constexpr int J = L::J;                                        // 16
    constexpr int NP = L::NPLANES;                                 // 3
    constexpr int UC = kIgNC / J;                                  // units per chunk: 4
    constexpr int FQ = 4;                                          // fields per lane
    constexpr int NSTK = PAIR ? 2 : 1;
    constexpr int C = kIgLutCopies<3>;
    static_assert(UC == 4 && TILEP % UC == 0 && UC * (kIgbKB / 8) * (J / FQ) == kIgThreads, "chunk shape");
    static_assert(L::LUT_N * C == kIgLutWords, "the table image fills grouped_ig_blocks_lds's share");

    extern __shared__ __attribute__((aligned(16))) char igb3_smem[];
    uint32_t* const lut_all = reinterpret_cast<uint32_t*>(igb3_smem + kIgbLutAt);

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
        char* dst = igb3_smem + (cc & 1) * kIgbWTile + (FQ * jq * UC + ul) * kIgbWPitch + o * 16;
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

    // ---- the lane as a stager of dY: pieces (row yr + 64 t, tile rows 8 pc .. 8 pc + 7), t < 2; tile rows 8 pc .. + 3 are the
    // columns 2 pc TileP .. + 3 from the chunk's first, tile rows 8 pc + 4 .. + 7 the columns (2 pc + 1) TileP .. + 3
    const int pc = tid & 7, yr = tid >> 3;
    const int y_col = 2 * pc * TILEP;
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
        uint2 y[2][2];                                             // [row][run]
    };
    auto load_rows = [&](Rows& rw, int cc) {
        const int st = PAIR ? (cc >= NCH) : 0;
        const uint16_t* __restrict__ Yp = a.dY[st] + unit_col0<3, TILEP>((cc - st * NCH) * UC);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
                rw.y[t][hf] = (yin[t] && cc < NCC) ? *reinterpret_cast<const uint2*>(Yp + yrow[t] + hf * TILEP) : make_uint2(0, 0);
    };
    auto store_rows = [&](const Rows& rw, int cc) {
        char* dst = igb3_smem + kIgbYAt + (cc & 1) * kIgbYTile + yr * kIgbYPitch + pc * 16;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint2 lo = rw.y[t][0], hi = rw.y[t][1];
            *reinterpret_cast<uint4*>(dst + t * 64 * kIgbYPitch) = y_swap ? make_uint4(hi.x, hi.y, lo.x, lo.y)
                                                                          : make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
    };

    // ---- the lane in the MFMAs: rows 64 rg .. + 63 of the row block, k 64 kq .. + 63 of the k block
    const int rg = wave >> 2, kq = wave & 3;
    const int h = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3, r16 = lane & 15;
    const bool active = row0 + 64 * rg < re;                       // wave-uniform
    const uint32_t tbase = lds_base_of(igb3_smem);
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

// The launch (inst_grouped_input_grad_blocks_b3.hip).  The grid is grouped_blocks_row_blocks(E, R) x K / 256, from the shapes
// alone; the caller has checked grouped_input_grad_w3_blocks_eligible.
inline int qgemm_grouped_input_grad_w3_blocks_launch(const GroupedInputGrad& g, hipStream_t stream) {
    GroupedIgArgs a = grouped_ig_args(g);
    a.slabs = a.K / kIgbKB;
    auto kernel = [](auto t, auto tp, auto pr) {
        return qgemm_grouped_input_grad_w3_blocks_kernel<decltype(t), decltype(tp)::value, decltype(pr)::value>;
    };
    return grouped_ig_launch<3>(g, kernel, (unsigned)(grouped_blocks_row_blocks(a.E, a.R) * a.slabs), grouped_ig_blocks_lds(g.pair), a,
                                stream);
}

}  // namespace flute_amd
