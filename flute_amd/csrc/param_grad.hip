// The parameter gradients of packed layers with the codes fixed: of the scales and of the lookup table, of one layer
// (dense) or of E stacked layers over rows sorted by expert (grouped).  One kernel template (grad_gemm.h:
// param_grad_kernel), one reduce kernel and one launch function serve all of them.
//
// Formulas.  G[k, n] = sum_r X[r, k] * dYw[r, n] over the row range, dYw = dY, or round_T(row_weight[r] * dY[r, n]) (the
// product in fp32, grouped only) formed where the dY tile is staged into LDS;
//     dS[n, j]  = round_T(sum_{k in group j} G[k, n] * L[k, n]),
//     dT2[c, h] = sum over (kappa, n) with idx(kappa, n) = c of G[2 kappa + h, n] * S[n, 2 kappa / g],
// L = pair(QM2, Q) the value dequant.hip multiplies by the scale (table2 only), idx the qgemm kernels' pair index
// code(2 kappa) << b | code(2 kappa + 1), h = 0 the low half of the pair word.  dY [rows, N], X [rows, K] row-major T,
// Q [P, K], S and dS [N, K / g] T, QM2 [4^b], dT2 [4^b][2] fp32 (it feeds an fp32 master parameter); products and sums in
// fp32.  The table itself is not read by the table gradient; with a dS the same launch writes the scale gradient too,
// bit for bit what the scale-only launch returns (dense: given its full scratch), and reads QM2 then and only then.
//
// Dense: the row range is [0, M).  When the blocks do not fill the chip M is split across workgroups
// (scale_grad_splits, the same split with or without a dT2): each split writes its dS as fp32 partials [split][N][K / g]
// to the scratch and splitk_reduce_kernel sums them in split order and rounds once.
//
// Grouped: Q, S, QM2, dS and dT2 carry a leading [E]; expert e's row range is [b_e, e_e), clamped to [0, R] (grouped_rows.h:
// offsets [E + 1] int32 in device memory and read by the kernels only); row_weight [R] fp32 or null.  The grid is (N / 128, ceil(K / 256), E), from the shapes alone: a workgroup walks ALL rows of its expert
// in the dense kernel's order, so an expert's dS and dT2 have the dense launch's bits on its rows wherever that launch does
// not split M.  Memory safety: every row index formed is in [b_e, e_e) inside [0, R) - a malformed table is safe, rows
// from clamp(offsets[E]) on are never read - and nothing of an expert without rows is read: its workgroups write their
// block of dS as zeros and return before they request a code, a scale or a table word, they write no partial, and the
// reduce kernel, which reads `offsets` itself, writes dT2[e] as zeros without reading the scratch.
//
// The table epilogue.  Every wave owns 4^b x 2 fp32 bins in LDS (8 x 2 KB at 4 bits, in the operand buffers, free by
// then).  A lane decodes the pair index behind each accumulator pair, multiplies both accumulators by the group's scale
// in fp32 and adds them into its wave's bins with ds_add_f32.  Only lanes of ONE wave ever meet on a bin, inside one
// instruction, and a wave's LDS instructions complete in program order: nothing depends on timing between waves.  (That
// colliding lanes of one instruction resolve in a fixed order is what tests/test_table_grad_gpu.py::test_reproducible
// checks.)  After a barrier the 8 waves' bins are summed in wave order and the workgroup writes one fp32 partial [4^b][2]
// to its own slot of the scratch, at ((z, y), x) of the grid - every (expert, block) has its slot whether or not the
// expert has rows, which is what keeps the host from reading offsets.  table_grad_reduce_kernel sums the partials.
//
// Equal arguments give equal bits: no atomics on global memory, every sum in a fixed order.
//
// Addition-chain depth d, the most fp32 roundings one term x * dy * s of dT2 passes through:
//     32 * steps   the mainloop, counting an MFMA as 32 chained additions (steps = 32-row steps of the workgroup's row
//                  range, <= ceil(M / 32); grouped: M = M_e = e_e - b_e)
//     1            the product with the scale
//     2048         a wave's 64 x 64 sub-block holds 2048 elements of either pair half: all on one bin at worst
//     8            the waves, in order
//     1            the rounding of the fp64 total
// so d <= 32 * ceil(M / 32) + 2058, whatever the layer's size (tests/table_grad_ref.py restates it).  (The weighted form
// rounds the operand dYw once more, before the chain.)
//
// Instantiations, 60: the ten layouts of layout_dispatch.h times dense scale, dense table, and grouped scale and grouped
// table each with and without a row weight.  There is no dense weighted form.
#include <algorithm>

#include "kernels.h"
#include "grad_gemm.h"
#include "layout_dispatch.h"

namespace flute_amd {

constexpr int kTgRedBins = 32, kTgRedSlots = 32;    // the reduce pass: bins x partial slots per workgroup

// dT2[e][bin] = sum over the wgs partials of e (dense: offsets null, one e) of part[e][w][bin]: per bin 32 slots each take
// every 32nd partial in order in fp64, then a fixed binary tree over the 32 and one rounding to fp32.  Zeros for an
// expert without rows, whose partials were never written.  Grid (bins / 32, E or 1).
__global__ __launch_bounds__(kTgRedBins* kTgRedSlots) void table_grad_reduce_kernel(const float* __restrict__ part,
                                                                                     const int* __restrict__ offsets,
                                                                                     float* __restrict__ dT2, int nbins,
                                                                                     long wgs, int R) {
    __shared__ double red[kTgRedSlots][kTgRedBins];
    const int b = threadIdx.x % kTgRedBins, slot = threadIdx.x / kTgRedBins;
    const int bin = blockIdx.x * kTgRedBins + b;      // nbins is a multiple of 32
    const int e = (int)blockIdx.y;
    float* __restrict__ out = dT2 + (size_t)e * nbins;
    if (offsets && grouped_rows(offsets, e, R).empty()) {                            // uniform over the workgroup
        if (slot == 0) out[bin] = 0.f;
        return;
    }
    const float* __restrict__ pe = part + (size_t)e * (size_t)wgs * (size_t)nbins;
    double v = 0.0;
    for (long w = slot; w < wgs; w += kTgRedSlots) v += (double)pe[(size_t)w * nbins + bin];
    red[slot][b] = v;
    __syncthreads();
    for (int s = kTgRedSlots / 2; s > 0; s >>= 1) {
        if (slot < s) red[slot][b] += red[slot + s][b];
        __syncthreads();
    }
    if (slot == 0) out[bin] = (float)red[0][b];
}

namespace {

long grad_blocks(int N, int K) { return (long)(N / kSgBN) * ((K + kSgBK - 1) / kSgBK); }
// the table partials of `blocks` workgroups: [blocks][4^b][2] fp32
size_t table_part_bytes(size_t blocks, int num_bits) { return blocks * ((size_t)2 << (2 * num_bits)) * 4; }

// splits of M for a dense launch: 1 when the blocks fill the chip (two workgroups per CU) or the scratch holds no split
int scale_grad_splits(int M, int N, int K, int lg, int num_sms, size_t scratch_bytes) {
    const long blocks = grad_blocks(N, K);
    const long steps = ((long)M + kSgBM - 1) / kSgBM;
    const long target = 2L * (num_sms < 1 ? 256 : num_sms);
    const size_t per_split = (size_t)N * (size_t)(K >> lg) * 4;
    long splits = std::min((target + blocks - 1) / blocks, steps / kSgMinSteps);
    splits = std::min<long>(splits, (long)std::min<size_t>(scratch_bytes / per_split, 1024));
    if (splits < 2) return 1;
    const long sps = (steps + splits - 1) / splits;   // every split gets >= 1 step
    return (int)((steps + sps - 1) / sps);
}

// the scratch with which scale_grad_splits is bounded by the shape alone: the most splits any M takes x [N][K / g] fp32
size_t scale_grad_full_scratch(int N, int K, int lg, int num_sms) {
    const long blocks = grad_blocks(N, K);
    const long target = 2L * (num_sms < 1 ? 256 : num_sms);
    if (blocks < 1 || blocks >= target) return 0;
    return (size_t)((target + blocks - 1) / blocks) * (size_t)N * (size_t)(K >> lg) * 4;
}

struct TgShape { int splits; size_t ds_bytes, t_bytes; };
// the split of M is the scale gradient's under its full scratch, with or without dS: dT2 does not depend on want_dS
TgShape table_grad_shape(int num_bits, int lg, int M, int N, int K, int want_dS, int num_sms) {
    TgShape s;
    s.splits = scale_grad_splits(M, N, K, lg, num_sms, scale_grad_full_scratch(N, K, lg, num_sms));
    s.ds_bytes = (want_dS && s.splits > 1) ? (size_t)s.splits * (size_t)N * (size_t)(K >> lg) * 4 : 0;
    s.t_bytes = table_part_bytes((size_t)grad_blocks(N, K) * (size_t)s.splits, num_bits);
    return s;
}

}  // namespace

size_t table_grad_scratch_bytes(int num_bits, int lg, int M, int N, int K, int want_dS, int num_sms) {
    const TgShape s = table_grad_shape(num_bits, lg, M, N, K, want_dS, num_sms);
    return s.ds_bytes + s.t_bytes;
}

size_t table_grad_grouped_scratch_bytes(int num_bits, int E, int N, int K) {
    return table_part_bytes((size_t)E * (size_t)grad_blocks(N, K), num_bits);
}

int param_grad_dispatch(const ParamGrad& a, hipStream_t stream) {
    const bool grouped = a.offsets != nullptr, table = a.dT2 != nullptr;
    const int N = a.N, K = a.K, lg = a.lg;
    // the grid's z and where the scratch goes: the experts and table partials alone, or the dense split and its dS partials
    int gz = a.E;
    float* ds_part = nullptr;
    float* t_part = reinterpret_cast<float*>(a.scratch);
    if (!grouped && table) {
        const TgShape sh = table_grad_shape(a.num_bits, lg, a.rows, N, K, a.dS != nullptr, a.num_sms);
        gz = sh.splits;
        if (sh.ds_bytes) ds_part = t_part;
        t_part = reinterpret_cast<float*>(reinterpret_cast<char*>(a.scratch) + sh.ds_bytes);
    } else if (!grouped) {
        gz = a.scratch ? scale_grad_splits(a.rows, N, K, lg, a.num_sms, a.scratch_bytes) : 1;
        if (gz > 1) ds_part = t_part;
    }
    const long steps = ((long)a.rows + kSgBM - 1) / kSgBM;
    const int sps = (int)((steps + gz - 1) / gz);     // (dense)
    const dim3 grid(N / kSgBN, (K + kSgBK - 1) / kSgBK, gz);
    const uint16_t* y = reinterpret_cast<const uint16_t*>(a.dY);
    const uint16_t* x = reinterpret_cast<const uint16_t*>(a.X);
    const int* off = reinterpret_cast<const int*>(a.offsets);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a.Q);
    const uint16_t* s = reinterpret_cast<const uint16_t*>(a.S);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(a.QM2);
    const float* rw = reinterpret_cast<const float*>(a.row_weight);
    uint16_t* ds = reinterpret_cast<uint16_t*>(a.dS);
    const int err = dispatch_layout(a.dtype, a.num_bits, a.tile_p, [&](auto t, auto bits, auto tp) {
        auto launch = [&](auto g, auto tb, auto w) {
            hipLaunchKernelGGL((param_grad_kernel<decltype(t), decltype(bits)::value, decltype(tp)::value,
                                                  decltype(g)::value, decltype(tb)::value, decltype(w)::value>),
                               grid, dim3(kSgThreads), 0, stream, y, x, off, q, s, qm2, rw, ds, ds_part, t_part, a.rows, N,
                               K, a.P, lg, sps);
        };
        auto form = [&](auto g, auto w) {
            if (table) launch(g, std::true_type{}, w);
            else launch(g, std::false_type{}, w);
        };
        if (!grouped) form(std::false_type{}, std::false_type{});
        else if (rw) form(std::true_type{}, std::true_type{});
        else form(std::true_type{}, std::false_type{});
    });
    if (err != FLUTE_OK) return err;
    if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    if (table) {
        const int nbins = 2 << (2 * a.num_bits);
        const long wgs = (long)grid.x * grid.y * (grouped ? 1 : gz);
        hipLaunchKernelGGL(table_grad_reduce_kernel, dim3(nbins / kTgRedBins, grouped ? gz : 1),
                           dim3(kTgRedBins * kTgRedSlots), 0, stream, t_part, off, a.dT2, nbins, wgs, a.rows);
        if (hipGetLastError() != hipSuccess) return FLUTE_ERR_LAUNCH;
    }
    if (ds_part) return splitk_reduce_dispatch(a.dtype, ds_part, a.dS, (size_t)N * (size_t)(K >> lg), gz, stream);
    return FLUTE_OK;
}

}  // namespace flute_amd
