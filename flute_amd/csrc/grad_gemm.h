// G = X^T dY reduced over M, the GEMM both parameter gradients of a packed layer share, the scale gradient's and the
// table gradient's epilogues on it, and the one kernel template built from them (param_grad_kernel; param_grad.hip
// states what it computes and launches it).
//
// A workgroup of 8 waves owns a 256 (k) x 128 (n) block - whole groups up to g = 256 - and walks its M range in steps
// of 32 rows: both operand tiles are copied row-major into LDS (16 B per lane, coalesced; rows past the range and
// columns past K are written as zeros, never masked) and read back with ds_read_b64_tr_b16, which delivers the MFMA
// fragments k- / n-major.  Every wave keeps G for its 64 x 64 sub-block in fp32 accumulators (v_mfma_f32_16x16x32: rows
// k, columns n).  The MFMA's reduction index is the step's row m in a fixed permutation shared by both operands:
// element e of lane group h is row 4h + e (e < 4) or 16 + 4h + e - 4, so that each 32-lane half of a transposed read
// covers 8 consecutive rows, which an LDS pitch of 8 dwords mod 64 spreads over all 64 banks.
#pragma once
#include "common.h"
#include "grouped_rows.h"
#include "mfma.h"

namespace flute_amd {

constexpr int kSgThreads = 512;                     // 8 waves: 4 along k x 2 along n
constexpr int kSgBK = 256;                          // k per workgroup
constexpr int kSgBN = 128;                          // n per workgroup (every legal N is a multiple)
constexpr int kSgBM = 32;                           // rows per step: one MFMA reduction depth
constexpr int kSgXPitch = kSgBK * 2 + 32;           // bytes per LDS row; 136 dwords = 8 mod 64
constexpr int kSgYPitch = kSgBN * 2 + 32;           // 72 dwords = 8 mod 64
constexpr int kSgXBytes = kSgBM * kSgXPitch;
constexpr int kSgYBytes = kSgBM * kSgYPitch;
constexpr int kSgLut = 2 * (kSgXBytes + kSgYBytes); // pair table behind the two operand buffers
constexpr int kSgLds = kSgLut + 4 * 256;
constexpr int kSgMinSteps = 4;                      // fewest 32-row steps a split of M gets
constexpr int kTgBinsAt = 4096;                     // the table gradient's wave bins: behind the scale epilogue's 4 KB of chunk sums
static_assert(kTgBinsAt + 8 * 2 * 256 * 4 <= kSgLut, "wave bins fit in the operand buffers");

typedef short s16x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint2 lds_tr16(uint32_t addr) {
    const s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)addr);
    return __builtin_bit_cast(uint2, v);
}

// acc[kt][nt][r] = G[k][n] over rows [m_begin, m_end) for the block at (kb, nb): n = nb + wn * 64 + nt * 16 + (lane & 15),
// k = kb + wk * 64 + kt * 16 + 4 (lane >> 4) + r.  Ends behind a barrier: the operand buffers are free on return.
// ROW_WEIGHT: the dY tile is staged as round_T(row_weight[m] * dY[m, n]), the product in fp32.
template <typename T, bool ROW_WEIGHT = false>
__device__ __forceinline__ void grad_gemm_mainloop(char* smem, const uint16_t* __restrict__ dY,
                                                   const uint16_t* __restrict__ X, int N, int K, int nb, int kb,
                                                   int m_begin, int m_end, f32x4_t (&acc)[4][4],
                                                   const float* __restrict__ row_weight = nullptr) {
    const uint32_t base = lds_base_of(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave & 3, wn = wave >> 2;          // the wave's 64 k and 64 n inside the block
    const int nsteps = (m_end - m_begin + kSgBM - 1) / kSgBM;

    // loaders: X two 16-B chunks (rows xr, xr + 16), dY one (row yr)
    const int xc = tid & 31, xr = tid >> 5, yc = tid & 15, yr = tid >> 4;
    const bool x_in = kb + 8 * xc < K;                // K % 64 == 0: a chunk is all in or all out
    const uint16_t* xp = X + (size_t)(kb + 8 * xc);
    const uint16_t* yp = dY + (size_t)(nb + 8 * yc);
    uint4 xv[2], yv;
    float yw = 0.f;
    auto load = [&](int m0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = m0 + xr + 16 * h;
            xv[h] = (x_in && m < m_end) ? *reinterpret_cast<const uint4*>(xp + (size_t)m * K) : make_uint4(0, 0, 0, 0);
        }
        const int m = m0 + yr;
        yv = m < m_end ? *reinterpret_cast<const uint4*>(yp + (size_t)m * N) : make_uint4(0, 0, 0, 0);
        if constexpr (ROW_WEIGHT) yw = m < m_end ? row_weight[m] : 0.f;
    };
    auto weigh = [&](uint32_t v) {                    // two T: each times yw in fp32, one rounding
        const uint32_t lo = Num<T>::from_float(Num<T>::to_float((uint16_t)(v & 0xffffu)) * yw);
        const uint32_t hi = Num<T>::from_float(Num<T>::to_float((uint16_t)(v >> 16)) * yw);
        return lo | (hi << 16);
    };
    auto store = [&](int buf) {
        if constexpr (ROW_WEIGHT) yv = make_uint4(weigh(yv.x), weigh(yv.y), weigh(yv.z), weigh(yv.w));
        char* xs = smem + buf * kSgXBytes + xc * 16;
        *reinterpret_cast<uint4*>(xs + xr * kSgXPitch) = xv[0];
        *reinterpret_cast<uint4*>(xs + (xr + 16) * kSgXPitch) = xv[1];
        *reinterpret_cast<uint4*>(smem + 2 * kSgXBytes + buf * kSgYBytes + yr * kSgYPitch + yc * 16) = yv;
    };

    // transposed reads: lane 4q + p of 16-lane group h supplies row 4h + q (+ 16 for elements 4..7), columns 4p .. 4p + 3
    const int h = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const uint32_t xa = base + (4 * h + q) * kSgXPitch + (wk * 64 + 4 * p) * 2;
    const uint32_t ya = base + 2 * kSgXBytes + (4 * h + q) * kSgYPitch + (wn * 64 + 4 * p) * 2;

#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    if (nsteps > 0) { load(m_begin); store(0); }
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) load(m_begin + (s + 1) * kSgBM);
        const uint32_t xb = xa + (s & 1) * kSgXBytes, yb = ya + (s & 1) * kSgYBytes;
        u32x4_t af[4], bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint2 a0 = lds_tr16(xb + t * 32), a1 = lds_tr16(xb + 16 * kSgXPitch + t * 32);
            const uint2 b0 = lds_tr16(yb + t * 32), b1 = lds_tr16(yb + 16 * kSgYPitch + t * 32);
            af[t] = u32x4_t{a0.x, a0.y, a1.x, a1.y};
            bf[t] = u32x4_t{b0.x, b0.y, b1.x, b1.y};
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[kt][nt] = Mfma<T>::run(af[kt], bf[nt], acc[kt][nt]);
        if (more) store((s + 1) & 1);
        __syncthreads();
    }
}

// The packed words behind a lane's accumulators acc[kt][nt]: 4 consecutive k = 2 pair words (x: k0, k0 + 1; y: k0 + 2,
// k0 + 3) of column n's unit, one per plane.
template <int BITS, int TILEP>
struct GradColumn {
    using L = Layout<BITS>;
    static constexpr int NP = L::NPLANES;
    int j, u;                                         // column n is column j of unit u
    __device__ __forceinline__ explicit GradColumn(int n) {
        constexpr int JT = L::J * TILEP;
        const int nblk = n / JT, rem = n - nblk * JT;
        j = rem / TILEP;
        u = nblk * TILEP + (rem - j * TILEP);
    }
    __device__ __forceinline__ void words(const uint32_t* __restrict__ Q, int N, int K2, int k0, uint2 (&w2)[NP]) const {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
            w2[pl] = *reinterpret_cast<const uint2*>(Q + (size_t)unit_row<BITS, TILEP>(u, pl, N) * K2 + (k0 >> 1));
    }
    // pair index code(k0 + 2e) << b | code(k0 + 2e + 1)
    __device__ __forceinline__ uint32_t index(const uint2 (&w2)[NP], int e) const {
        uint32_t w[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) w[pl] = e ? w2[pl].y : w2[pl].x;
        return field<BITS>(w, j);
    }
};

// The scale gradient from the accumulators: a lane's accumulators are decoded as dequant_kernel does (Layout / unit_row
// / unit_col0 / field, table2 in LDS at `lut`), multiplied and summed per 32-k chunk; lanes and then waves (through LDS:
// the first 4 KB of smem) sum the chunks of a group in a fixed order.  Writes T to dS, or fp32 to pout when given.
template <typename T, int BITS, int TILEP>
__device__ __forceinline__ void scale_grad_epilogue(char* smem, const uint32_t* lut, const f32x4_t (&acc)[4][4],
                                                    const uint32_t* __restrict__ Q, uint16_t* __restrict__ dS,
                                                    float* __restrict__ pout, int N, int K, int lg, int nb, int kb) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave & 3, wn = wave >> 2, h = lane >> 4;
    const int K2 = K >> 1;
    float* red = reinterpret_cast<float*>(smem);      // [8 chunks of 32 k][128 n]; the operand buffers are free now
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int nl = wn * 64 + nt * 16 + (lane & 15);
        const GradColumn<BITS, TILEP> col(nb + nl);
        float c[2] = {0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int k0 = kb + wk * 64 + kt * 16 + 4 * h;
            if (k0 < K) {                             // columns past K hold zeros; their codes are not read
                uint2 w2[GradColumn<BITS, TILEP>::NP];
                col.words(Q, N, K2, k0, w2);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint32_t pr = lut[col.index(w2, e)];    // low half k = 2 kappa, high half 2 kappa + 1
                    c[kt >> 1] += acc[kt][nt][2 * e] * Num<T>::to_float((uint16_t)(pr & 0xffffu));
                    c[kt >> 1] += acc[kt][nt][2 * e + 1] * Num<T>::to_float((uint16_t)(pr >> 16));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            c[i] += __shfl_xor(c[i], 16, 64);
            c[i] += __shfl_xor(c[i], 32, 64);
        }
        if (lane < 16) {
            red[(wk * 2 + 0) * kSgBN + nl] = c[0];
            red[(wk * 2 + 1) * kSgBN + nl] = c[1];
        }
    }
    __syncthreads();

    // one output per (n, group of the block): the group's 32-k chunks in order
    const int G = K >> lg;
    const int lgb = 8 - lg;                           // log2(groups per block)
    const int cpg = 1 << (lg - 5);                    // chunks per group
    for (int it = tid; it < (kSgBN << lgb); it += kSgThreads) {
        const int nl = it >> lgb, jg = it & ((1 << lgb) - 1);
        if (kb + (jg << lg) >= K) continue;
        float v = 0.f;
        for (int ch = jg * cpg; ch < (jg + 1) * cpg; ++ch) v += red[ch * kSgBN + nl];
        const size_t o = (size_t)(nb + nl) * G + (kb >> lg) + jg;
        if (pout) pout[o] = v;
        else dS[o] = Num<T>::from_float(v);
    }
}

// The block's groups below K of a scale gradient as zeros: what a workgroup of the grouped kernels writes for an expert
// without rows, in scale_grad_epilogue's place.
__device__ __forceinline__ void scale_grad_zero_block(uint16_t* __restrict__ dS, int N, int K, int lg, int nb, int kb) {
    const int G = K >> lg;
    const int lgb = 8 - lg;
    for (int it = threadIdx.x; it < (kSgBN << lgb); it += kSgThreads) {
        const int nl = it >> lgb, jg = it & ((1 << lgb) - 1);
        if (kb + (jg << lg) >= K) continue;
        dS[(size_t)(nb + nl) * G + (kb >> lg) + jg] = 0;
    }
}

// The table gradient from the accumulators (param_grad.hip describes it): every wave zeroes its 4^b x 2 fp32 bins at
// smem + kTgBinsAt, decodes the pair index behind each accumulator pair, multiplies both accumulators by the group's
// scale S[n, k / g] in fp32 and adds them into its bins with ds_add_f32; after a barrier the 8 waves' bins are summed in
// wave order into t_out [4^b][2], the workgroup's partial.  With dS non-null (uniform) the scale gradient is written in
// between, by scale_grad_epilogue with `lut`, dS and pout: its chunk sums lie below the bins.
template <typename T, int BITS, int TILEP>
__device__ __forceinline__ void table_grad_epilogue(char* smem, const uint32_t* lut, const f32x4_t (&acc)[4][4],
                                                    const uint32_t* __restrict__ Q, const uint16_t* __restrict__ S,
                                                    uint16_t* __restrict__ dS, float* __restrict__ pout,
                                                    float* __restrict__ t_out, int N, int K, int lg, int nb, int kb) {
    using L = Layout<BITS>;
    constexpr int NB = 2 * L::LUT_N;                  // bins
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));                     // opaque: what the epilogue derives from it is computed here, not kept across the mainloop
    const int lane = tid & 63, wave = tid >> 6;
    const int wk = wave & 3, wn = wave >> 2, h = lane >> 4;
    float* all_bins = reinterpret_cast<float*>(smem + kTgBinsAt);
    float* bins = all_bins + wave * NB;               // this wave's alone until the barrier
    for (int i = lane; i < NB; i += 64) bins[i] = 0.f;

    const int K2 = K >> 1, G = K >> lg;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = nb + wn * 64 + nt * 16 + (lane & 15);
        const GradColumn<BITS, TILEP> col(n);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int k0 = kb + wk * 64 + kt * 16 + 4 * h;
            if (k0 < K) {                             // columns past K hold zeros; their codes are not read
                uint2 w2[GradColumn<BITS, TILEP>::NP];
                col.words(Q, N, K2, k0, w2);
                const float s = Num<T>::to_float(S[(size_t)n * G + (k0 >> lg)]);   // 4 k of one group: g >= 32
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    float* bin = bins + 2 * col.index(w2, e);
                    __hip_atomic_fetch_add(bin, acc[kt][nt][2 * e] * s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(bin + 1, acc[kt][nt][2 * e + 1] * s, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }

    if (dS) scale_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Q, dS, pout, N, K, lg, nb, kb);   // uniform: it holds a barrier
    __syncthreads();
    for (int i = tid; i < NB; i += kSgThreads) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += all_bins[w * NB + i];
        t_out[i] = v;
    }
}

// The parameter-gradient kernel in all its forms; the axes are compile-time, a workgroup is one (k, n) block of one z.
//   GROUPED   the row range: the rows of expert z (grouped_rows.h), with the Q / S / QM2 / dS bases
//             moved to that expert (64-bit) and a return before anything of an expert without rows is read (its block of
//             dS written as zeros, no partial); dense: the z-th run of steps_per_split 32-row steps of [0, rows), with
//             the scale gradient's fp32 partial at ds_part[z] when ds_part is given.
//   TABLE     the epilogue: table_grad_epilogue into the workgroup's slot of t_part, at ((z, y), x), with the scale
//             epilogue inside it when dS is given (uniform); else scale_grad_epilogue alone.
//   WEIGHTED  the mainloop's ROW_WEIGHT.
// QM2 is read when dS is written and only then.  Written for 4 waves per SIMD = two workgroups per CU: at most 128 VGPRs.
template <typename T, int BITS, int TILEP, bool GROUPED, bool TABLE, bool WEIGHTED>
__global__ __launch_bounds__(kSgThreads, 4) void param_grad_kernel(
    const uint16_t* __restrict__ dY, const uint16_t* __restrict__ X, const int* __restrict__ offsets,
    const uint32_t* __restrict__ Q, const uint16_t* __restrict__ S, const uint32_t* __restrict__ QM2,
    const float* __restrict__ row_weight, uint16_t* __restrict__ dS, float* __restrict__ ds_part,
    float* __restrict__ t_part, int rows, int N, int K, int P, int lg, int steps_per_split) {
    using L = Layout<BITS>;
    __shared__ __attribute__((aligned(16))) char smem[kSgLds];
    const int tid = threadIdx.x;
    const int nb = blockIdx.x * kSgBN, kb = blockIdx.y * kSgBK;
    const int z = (int)blockIdx.z;
    const int G = K >> lg;
    int rb, re;
    if constexpr (GROUPED) {
        // grouped_rows.h's range with its two clamps written out, deliberately (profiles/grouped_rows_ab.json)
        rb = grouped_clamp(offsets[z], rows);
        re = grouped_clamp(offsets[z + 1], rows);
        if (!TABLE || dS) dS += (size_t)z * (size_t)N * (size_t)G;
        if (re <= rb) {
            if (!TABLE || dS) scale_grad_zero_block(dS, N, K, lg, nb, kb);
            return;
        }
        Q += (size_t)z * (size_t)P * (size_t)(K >> 1);
        QM2 += (size_t)z * L::LUT_N;
        if constexpr (TABLE) S += (size_t)z * (size_t)N * (size_t)G;
    } else {
        rb = z * steps_per_split * kSgBM;
        re = (int)min((long)rows, (long)rb + (long)steps_per_split * kSgBM);
    }

    uint32_t* lut = reinterpret_cast<uint32_t*>(smem + kSgLut);
    if (!TABLE || dS)
        for (int i = tid; i < L::LUT_N; i += kSgThreads) lut[i] = QM2[i];

    f32x4_t acc[4][4];
    grad_gemm_mainloop<T, WEIGHTED>(smem, dY, X, N, K, nb, kb, rb, re, acc, row_weight);
    float* pout = nullptr;                            // (a grouped launch has no split: the branch on it folds away)
    if constexpr (!GROUPED)
        if (ds_part) pout = ds_part + (size_t)blockIdx.z * N * G;
    if constexpr (TABLE) {
        const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        table_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Q, S, dS, pout, t_part + wg * (2 * L::LUT_N), N, K, lg,
                                            nb, kb);
    } else {
        scale_grad_epilogue<T, BITS, TILEP>(smem, lut, acc, Q, dS, pout, N, K, lg, nb, kb);
    }
}

}  // namespace flute_amd
