// The gradient of a packed layer's scales: dS[n, j] = round_T(sum_m sum_{k in group j} dY[m, n] * X[m, k] * L[k, n]),
// L[k, n] = pair(QM2, Q)[k, n] the value dequant.hip multiplies by the scale (table2 only, the qgemm kernels' pair index),
// dY [M, N] and X [M, K] row-major T, dS [N, K / g] T.  Products and sums in fp32, one rounding to T.
//
// A GEMM that reduces over M with the code lookup in its epilogue.  A workgroup of 8 waves owns a 256 (k) x 128 (n) block
// - whole groups up to g = 256 - and walks its M range in steps of 32 rows: both operand tiles are copied row-major into
// LDS (16 B per lane, coalesced; rows past the range and columns past K are written as zeros, never masked) and read
// back with ds_read_b64_tr_b16, which delivers the MFMA fragments k- / n-major.  Every wave keeps G = X^T dY for its
// 64 x 64 sub-block in fp32 accumulators (v_mfma_f32_16x16x32: rows k, columns n).  The MFMA's reduction index is the
// step's row m in a fixed permutation shared by both operands: element e of lane group h is row 4h + e (e < 4) or
// 16 + 4h + e - 4, so that each 32-lane half of a transposed read covers 8 consecutive rows, which an LDS pitch of
// 8 dwords mod 64 spreads over all 64 banks.
//
// Epilogue: a lane's accumulators are 4 consecutive k = 2 pair words of one column n, decoded as dequant_kernel does
// (Layout / unit_row / unit_col0 / field, table2 in LDS), multiplied and summed per 32-k chunk; lanes and then waves
// (through LDS) sum the chunks of a group in a fixed order.  When the blocks do not fill the chip, M is split across
// workgroups: each writes fp32 partials [split][N][K / g] to the caller's scratch and a second pass sums them in split
// order and rounds once (splitk_reduce_kernel).  No atomics: the same arguments give the same bits.
#include <algorithm>

#include "kernels.h"
#include "mfma.h"
#include "../../include/flute_amd.h"

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

typedef short s16x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint2 lds_tr16(uint32_t addr) {
    const s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(uintptr_t)addr);
    return __builtin_bit_cast(uint2, v);
}

template <typename T, int BITS, int TILEP>
__global__ __launch_bounds__(kSgThreads) void scale_grad_kernel(const uint16_t* __restrict__ dY,
                                                                const uint16_t* __restrict__ X,
                                                                const uint32_t* __restrict__ Q,
                                                                const uint32_t* __restrict__ QM2,
                                                                uint16_t* __restrict__ dS, float* __restrict__ part,
                                                                int M, int N, int K, int lg, int steps_per_split) {
    using L = Layout<BITS>;
    constexpr int NP = L::NPLANES;
    constexpr int JT = L::J * TILEP;
    __shared__ __attribute__((aligned(16))) char smem[kSgLds];
    const uint32_t base = lds_base_of(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wk = wave & 3, wn = wave >> 2;          // the wave's 64 k and 64 n inside the block
    const int nb = blockIdx.x * kSgBN, kb = blockIdx.y * kSgBK;

    uint32_t* lut = reinterpret_cast<uint32_t*>(smem + kSgLut);
    for (int i = tid; i < L::LUT_N; i += kSgThreads) lut[i] = QM2[i];

    const int m_begin = (int)blockIdx.z * steps_per_split * kSgBM;
    const int m_end = (int)min((long)M, (long)m_begin + (long)steps_per_split * kSgBM);
    const int nsteps = (m_end - m_begin + kSgBM - 1) / kSgBM;

    // loaders: X two 16-B chunks (rows xr, xr + 16), dY one (row yr)
    const int xc = tid & 31, xr = tid >> 5, yc = tid & 15, yr = tid >> 4;
    const bool x_in = kb + 8 * xc < K;                // K % 64 == 0: a chunk is all in or all out
    const uint16_t* xp = X + (size_t)(kb + 8 * xc);
    const uint16_t* yp = dY + (size_t)(nb + 8 * yc);
    uint4 xv[2], yv;
    auto load = [&](int m0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = m0 + xr + 16 * h;
            xv[h] = (x_in && m < m_end) ? *reinterpret_cast<const uint4*>(xp + (size_t)m * K) : make_uint4(0, 0, 0, 0);
        }
        const int m = m0 + yr;
        yv = m < m_end ? *reinterpret_cast<const uint4*>(yp + (size_t)m * N) : make_uint4(0, 0, 0, 0);
    };
    auto store = [&](int buf) {
        char* xs = smem + buf * kSgXBytes + xc * 16;
        *reinterpret_cast<uint4*>(xs + xr * kSgXPitch) = xv[0];
        *reinterpret_cast<uint4*>(xs + (xr + 16) * kSgXPitch) = xv[1];
        *reinterpret_cast<uint4*>(smem + 2 * kSgXBytes + buf * kSgYBytes + yr * kSgYPitch + yc * 16) = yv;
    };

    // transposed reads: lane 4q + p of 16-lane group h supplies row 4h + q (+ 16 for elements 4..7), columns 4p .. 4p + 3
    const int h = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const uint32_t xa = base + (4 * h + q) * kSgXPitch + (wk * 64 + 4 * p) * 2;
    const uint32_t ya = base + 2 * kSgXBytes + (4 * h + q) * kSgYPitch + (wn * 64 + 4 * p) * 2;

    f32x4_t acc[4][4];
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

    // epilogue: lane holds G[k][n] for n = .. + nt * 16 + (lane & 15), k = .. + kt * 16 + 4 h + r (r = 0..3)
    const int K2 = K >> 1;
    float* red = reinterpret_cast<float*>(smem);      // [8 chunks of 32 k][128 n]; the operand buffers are free now
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int nl = wn * 64 + nt * 16 + (lane & 15);
        const int n = nb + nl;
        const int nblk = n / JT, rem = n - nblk * JT;
        const int j = rem / TILEP, u = nblk * TILEP + (rem - j * TILEP);
        float c[2] = {0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int k0 = kb + wk * 64 + kt * 16 + 4 * h;
            if (k0 < K) {                             // columns past K hold zeros; their codes are not read
                uint2 w2[NP];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
                    w2[pl] = *reinterpret_cast<const uint2*>(Q + (size_t)unit_row<BITS, TILEP>(u, pl, N) * K2 + (k0 >> 1));
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    uint32_t w[NP];
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) w[pl] = e ? w2[pl].y : w2[pl].x;
                    const uint32_t pr = lut[field<BITS>(w, j)];   // low half k = 2 kappa, high half 2 kappa + 1
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
    float* pout = part ? part + (size_t)blockIdx.z * N * G : nullptr;
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

// splits of M for the launch: 1 when the blocks fill the chip (two workgroups per CU) or the scratch holds no split
int scale_grad_splits(int M, int N, int K, int lg, int num_sms, size_t scratch_bytes) {
    const long blocks = (long)(N / kSgBN) * ((K + kSgBK - 1) / kSgBK);
    const long steps = ((long)M + kSgBM - 1) / kSgBM;
    const long target = 2L * (num_sms < 1 ? 256 : num_sms);
    const size_t per_split = (size_t)N * (size_t)(K >> lg) * 4;
    long splits = std::min((target + blocks - 1) / blocks, steps / kSgMinSteps);
    splits = std::min<long>(splits, (long)std::min<size_t>(scratch_bytes / per_split, 1024));
    if (splits < 2) return 1;
    const long sps = (steps + splits - 1) / splits;   // every split gets >= 1 step
    return (int)((steps + sps - 1) / sps);
}

int scale_grad_dispatch(int dtype, int num_bits, int tile_p, int lg, int M, int N, int K, const void* dY,
                        const void* X, const void* Q, const void* QM2, void* dS, void* scratch, size_t scratch_bytes,
                        int num_sms, hipStream_t stream) {
    const int splits = scratch ? scale_grad_splits(M, N, K, lg, num_sms, scratch_bytes) : 1;
    const long steps = ((long)M + kSgBM - 1) / kSgBM;
    const int sps = (int)((steps + splits - 1) / splits);
    const dim3 grid(N / kSgBN, (K + kSgBK - 1) / kSgBK, splits);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(dY);
    const uint16_t* x = reinterpret_cast<const uint16_t*>(X);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(Q);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    uint16_t* ds = reinterpret_cast<uint16_t*>(dS);
    float* part = splits > 1 ? reinterpret_cast<float*>(scratch) : nullptr;
#define FLUTE_SG(TY, B, TP)                                                                                          \
    hipLaunchKernelGGL((scale_grad_kernel<TY, B, TP>), grid, dim3(kSgThreads), 0, stream, y, x, q, qm2, ds, part, M, \
                       N, K, lg, sps)
#define FLUTE_SG_T(B, TP)                         \
    if (dtype == FLUTE_F16) FLUTE_SG(F16, B, TP); \
    else FLUTE_SG(BF16, B, TP)
    if (num_bits == 4 && tile_p == 32) { FLUTE_SG_T(4, 32); }
    else if (num_bits == 4 && tile_p == 64) { FLUTE_SG_T(4, 64); }
    else if (num_bits == 2 && tile_p == 32) { FLUTE_SG_T(2, 32); }
    else if (num_bits == 2 && tile_p == 64) { FLUTE_SG_T(2, 64); }
    else if (num_bits == 3 && tile_p == 32) { FLUTE_SG_T(3, 32); }
    else return FLUTE_ERR_TEMPLATE_ID;
#undef FLUTE_SG_T
#undef FLUTE_SG
    if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    if (splits > 1) {
        const size_t mn = (size_t)N * (size_t)(K >> lg);  // a multiple of 16: N % 128 == 0
        const unsigned rgrid = (unsigned)((mn / 4 + 255) / 256);
        if (dtype == FLUTE_F16)
            hipLaunchKernelGGL(splitk_reduce_kernel<F16>, dim3(rgrid), dim3(256), 0, stream, part, ds, mn, splits);
        else
            hipLaunchKernelGGL(splitk_reduce_kernel<BF16>, dim3(rgrid), dim3(256), 0, stream, part, ds, mn, splits);
        if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    }
    return FLUTE_OK;
}

}  // namespace flute_amd
