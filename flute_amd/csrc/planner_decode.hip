// Host side of the C ABI, first planner unit: which kernels are built (the lookups over the instantiation units' row lists,
// kernels.h) and the launch-shape planners of the decode families, the skinny kernel, the split-K block kernel and the ring
// kernel.  planner.hip chooses among them; host.h declares what it reads here.  No device code.
#include <algorithm>
#include <string.h>
#include <vector>

#include "host.h"
#include "kernels.h"
#include "qgemm_persist.h"
#include "qgemm_fast.h"
#include "qgemm_fastm.h"
#include "qgemm_persistm.h"
#include "qgemm_skinny.h"
#include "qgemm_splitk.h"

namespace flute_amd::host {

// Workspace layout (every kernel): [0, kXwgFlagBytes) tile state words of the in-launch reductions (xwg.h; zero between
// calls), fp32 slabs behind them.  A planner sees the room behind the state words only.
size_t slab_room(size_t workspace_bytes) { return workspace_bytes > kXwgFlagBytes ? workspace_bytes - kXwgFlagBytes : 0; }

// ---- which kernels are built ---------------------------------------------------------------------------
// Each family's entry point for a call's layer (bit width, dtype, TileP) and the family's knobs, from the row lists of the
// instantiation units (kernels.h); nullptr: not built.  The only statement of which shapes exist: the planners ask these, and
// resolve_kernel stores the answer with the plan.
template <class Kernel> static const void* fn_of(Kernel k) { return reinterpret_cast<const void*>(k); }
#define FLUTE_BY_BITS(F, ...) (c.bits == 4 ? fn_of(F##_b4(__VA_ARGS__)) : (c.bits == 3 ? fn_of(F##_b3(__VA_ARGS__)) : fn_of(F##_b2(__VA_ARGS__))))
#define FLUTE_BY_DTYPE(F, ...) (c.dtype == 0 ? fn_of(F##_f16(__VA_ARGS__)) : fn_of(F##_bf16(__VA_ARGS__)))
const void* stream_fn(const Call& c, int mb, int depth) { return FLUTE_BY_BITS(stream_kernel, c.dtype, c.t.tile_p, mb, depth); }
const void* oneshot_fn(const Call& c, int mb, int depth, int had, int pipe) {
    if (c.bits == 3) return fn_of(oneshot_kernel_b3(c.dtype, c.t.tile_p, mb, depth, had, pipe));
    return c.bits == 4 ? FLUTE_BY_DTYPE(oneshot_kernel_b4, c.t.tile_p, mb, depth, had, pipe) : FLUTE_BY_DTYPE(oneshot_kernel_b2, c.t.tile_p, mb, depth, had, pipe);
}
const void* persist_fn(const Call& c, int mb, int depth, int nsets, int had) { return FLUTE_BY_BITS(persist_kernel, c.dtype, c.t.tile_p, mb, depth, nsets, had); }
const void* fast_fn(const Call& c, int waves, int kw, int depth, int mb) { return c.bits == 4 ? fn_of(fast_kernel_b4(c.dtype, c.t.tile_p, waves, kw, depth, mb)) : nullptr; }
const void* fastm_fn(const Call& c, int waves, int nm, int lg, int ng) { return c.bits == 4 ? fn_of(fastm_kernel_b4(c.dtype, c.t.tile_p, waves, nm, lg, ng)) : nullptr; }
const void* persistm_fn(const Call& c, int lg, int ng, int xr, int waves, int xres) {
    if (c.bits == 3) return nullptr;
    return c.bits == 4 ? FLUTE_BY_DTYPE(persistm_kernel_b4, c.t.tile_p, lg, ng, xr, waves, xres) : FLUTE_BY_DTYPE(persistm_kernel_b2, c.t.tile_p, lg, ng, xr, waves, xres);
}
const void* skinny_fn(const Call& c, int depth) { return c.bits == 4 ? fn_of(skinny_kernel_b4(c.dtype, c.t.tile_p, depth)) : nullptr; }
const void* splitk_fn(const Call& c, int rt, int kp) { return fn_of(splitk_kernel(c.bits, c.dtype, c.t.tile_p, rt, kp)); }
const void* block_fn(const Call& c, int cfg) { return FLUTE_BY_BITS(block_kernel, c.dtype, c.t.tile_p, cfg); }
const void* tile_fn(const Call& c, int r, int mt, int sw) {                     // sw: slabs per wave, 2 for 4-bit layers only
    if (c.bits == 4) return fn_of(tile_kernel_b4(c.dtype, c.t.tile_p, r, mt, sw));
    if (sw != 1) return nullptr;
    return c.bits == 3 ? fn_of(tile_kernel_b3(c.dtype, c.t.tile_p, r, mt)) : fn_of(tile_kernel_b2(c.dtype, c.t.tile_p, r, mt));
}
#undef FLUTE_BY_BITS
#undef FLUTE_BY_DTYPE

// ---- streaming decode kernel: launch shape ------------------------------------------------------------
// Every (waves per workgroup, in-workgroup K split) that fits LDS is priced by the piece-slots its busiest
// CU executes (1 piece = 1 KiB of one unit's packed row) plus a per-visit overhead, and the candidates are
// ranked; template knob Stages (2..5) picks the best / 2nd / 3rd / 4th, so the tuner's search over ids
// covers the shapes that matter.
namespace {
struct StreamShape {
    int W, kw, nchunks, kc, kx, upw, ngroups, nwg, visits, s_wave_bytes, s_fast;
    size_t x_off, s_off, red_off, total;
    double cost;
};

bool stream_shape(int bits, int mb, int lg, int units, int krange, int G, bool split_aligned, int num_sms, int W,
                  int kw, int threads_cap, StreamShape* o) {
    const int J = (bits == 3) ? 16 : 16 / bits;
    const int g = 1 << lg;
    const int gpp = 512 >> lg;
    const int lut = stream_lut_bytes(bits);
    const int align_k = std::max(512, 8 * g);                 // K boundaries on 16-B scale granules
    StreamShape s;
    s.W = W; s.kw = kw;
    s.upw = W / kw;
    s.ngroups = ceil_div(units, s.upw);
    bool fits = false;
    for (int nch = 1; nch <= 64; ++nch) {
        int kc = (nch == 1) ? round_up(krange, 512) : round_up(ceil_div(krange, nch), align_k);
        const int real_chunks = ceil_div(krange, kc);
        if (nch > 1 && real_chunks != nch) continue;
        const int pc = ceil_div(std::min(kc, krange), 512);
        const int pk = ceil_div(pc, kw);
        const int ngran = ceil_div(pk * gpp, 8);
        s.s_wave_bytes = ngran * J * 16;
        s.kx = round_up(std::min(kc, krange), 512);
        s.x_off = (size_t)lut;
        s.s_off = s.x_off + (size_t)mb * s.kx * 2;
        s.red_off = s.s_off + (size_t)W * s.s_wave_bytes;
        s.total = s.red_off + 64 + (size_t)2 * W * J * mb * 4;     // arrival counters + two partial-sum buffers
        if (s.total <= (size_t)kMaxLds) {
            s.nchunks = nch; s.kc = kc;
            const bool chunk_ok = nch == 1 || kc % (8 * g) == 0;
            const bool part_ok = kw == 1 || (pk * 512) % (8 * g) == 0;
            s.s_fast = (G % 8 == 0 && split_aligned && chunk_ok && part_ok) ? 1 : 0;
            const int occ = (threads_cap >= 1024 && W <= 8 && s.total <= (size_t)kMaxLds / 2) ? 2 : 1;
            s.nwg = std::min(s.ngroups, num_sms * occ);
            s.visits = ceil_div(s.ngroups, s.nwg);
            const int wgs_cu = ceil_div(s.nwg, num_sms);
            const double per_visit = pk + 1.5 + (kw > 1 ? 2.0 : 0.0) + (s.s_fast ? 0.0 : 4.0);
            double cost = (double)wgs_cu * W * s.visits * nch * per_visit;
            const int waves_cu = wgs_cu * W;
            if (waves_cu < 12) cost *= 1.0 + 0.05 * (12 - waves_cu);   // fewer bytes in flight per CU
            if (nch > 1) cost *= 1.25;                        // activations restaged per visit, barriers
            s.cost = cost;
            fits = true;
            break;
        }
    }
    if (!fits) return false;
    *o = s;
    return true;
}
}  // namespace

// ---- one-shot decode kernel (qgemm_oneshot.h): launch shape --------------------------------------------
// A workgroup of W = upw x kw waves owns upw units for the whole of K (no persistence, no grid K split): wave
// (ul, kpart) decodes pk <= D pieces of its unit.  Candidates: D pieces per wave x W in {4, 8, 16}, kw the
// smallest power of two that fits K into kw x D pieces.  Ranked by what tools/ubench/oneshot_lab measured on
// 4096^2 / 4096x11008 (profiles/r03_oneshot_lab.jsonl): launches that give every CU a workgroup first, then
// the smallest in-workgroup K split (kw = 1 needs no cross-wave reduction), then the smallest workgroup that
// keeps the launch at <= 3 workgroups per CU (every workgroup builds its own table image).
// Template knobs: Stages 2..5 -> rank 0..3; QuantMapMode digit (4-bit ids) 1 / 2 -> D = 4 / 8 only.
namespace {
struct OneShape { int W, kw, upw, pk, depth, pipe, ipw, grid; size_t lds; };
}  // namespace

int plan_oneshot(const Call& c, const Ovr& ov, flute_plan* p, OneArgs* oa) {
    const int bits = c.bits, lg = c.lg, M = c.M, N = c.N, K = c.K, num_sms = c.num_sms, template_id = c.template_id;
    const flute_template_info& t = c.t;
    if (lg < 6) return FLUTE_ERR_SHAPE;                       // 32-wide groups: twice the scale words per wave
    if ((K >> lg) & 1) return FLUTE_ERR_SHAPE;                // scale rows are read as aligned dwords (two groups each)
    const int J = (bits == 3) ? 16 : 16 / bits;
    const int units = N / J;
    const int npieces = ceil_div(K, 512);
    int mb = 1; while (mb < M) mb <<= 1;
    const int dlo = (bits == 3) ? 2 : 4, dhi = 2 * dlo;
    if (!oneshot_fn(c, mb, dlo, 0, 0)) return FLUTE_ERR_SHAPE;         // rows per pass: 1, 2, 4 (3 bits: 1, 2)
    int dsel = 0;                                             // 0: both depths
    if (bits == 4 && (template_id % 4) == 1) dsel = dlo;
    if (bits == 4 && (template_id % 4) == 2) dsel = dhi;
    if (ov.one_shot == 1 && (ov.depth == dlo || ov.depth == dhi)) dsel = ov.depth;
    const int wcap = std::min(t.threads, oneshot_max_threads(bits, mb)) / 64;
    const int runs = oneshot_lut_runs(bits);
    const int xpr = (mb == 4) ? 1 : 2;
    std::vector<OneShape> cands;
    for (int D = dhi; D >= dlo; D /= 2) {
        if ((dsel && D != dsel) || !oneshot_fn(c, mb, D, 0, 0)) continue;
        for (int W = 4; W <= 16; W *= 2) {
            int w = W;
            if (ov.waves > 0) { if (W != 4) continue; w = ov.waves; }
            if (w > wcap || w < 1) continue;
            int kw = 1;
            while (ceil_div(npieces, kw) > D) kw *= 2;
            if (ov.kw > 0) kw = floor_pow2(ov.kw);
            if (kw > w || w % kw || ceil_div(npieces, kw) > D) continue;
            OneShape s;
            s.W = w; s.kw = kw; s.upw = w / kw; s.pk = ceil_div(npieces, kw); s.depth = D;
            s.ipw = ceil_div(runs, w);
            if (s.ipw > (bits == 2 ? 16 : 8)) continue;       // table runs a wave writes: at most 8 (2 bits: 16, four per lane group) - more would leave the image incomplete
            if (npieces * 64 > xpr * w * 64) continue;        // activations staged from registers only
            s.grid = ceil_div(units, s.upw);
            s.lds = oneshot_lds_bytes(bits, mb, D, lg, K, w);
            if (s.lds > (size_t)kMaxLds) continue;
            // pipelined loop: one row, every wave holds D whole pieces
            s.pipe = (mb == 1 && s.pk == D && npieces == kw * s.pk && units % s.upw == 0 && K % 512 == 0) ? 1 : 0;
            cands.push_back(s);
        }
    }
    if (cands.empty()) return FLUTE_ERR_SHAPE;
    auto fills = [&](const OneShape& s) { return (long)s.grid * 10 >= (long)num_sms * 9; };
    std::stable_sort(cands.begin(), cands.end(), [&](const OneShape& a, const OneShape& b) {
        if (fills(a) != fills(b)) return fills(a);
        if (!fills(a)) return a.grid > b.grid;
        if (a.kw != b.kw) return a.kw < b.kw;
        const bool many_a = a.grid > 3 * num_sms, many_b = b.grid > 3 * num_sms;      // > 3 workgroups per CU: take the larger workgroup
        if (many_a != many_b) return many_b;
        if (a.W != b.W) return a.W < b.W;
        return a.depth > b.depth;
    });
    size_t pick = std::min((size_t)std::max(0, t.stages - 2), cands.size() - 1);
    if (ov.waves > 0 || ov.kw > 0) pick = 0;
    const OneShape& s = cands[pick];
    p->family = 0;
    p->m_block = mb; p->waves = s.W; p->kw = s.kw; p->splitk = 1; p->k_per_split = K;
    p->grid = (unsigned)s.grid; p->block = (unsigned)(s.W * 64);
    p->lds_bytes = s.lds; p->lut_copies = 32;
    p->ring_depth = s.depth; p->visits = 1; p->k_chunks = 1; p->one_shot = 1 + s.pipe;
    if (oa) { oa->lg = lg; oa->lkw = ilog2(s.kw); oa->upw = s.upw; oa->pk = s.pk; oa->ipw = s.ipw; oa->depth = s.depth; oa->pipe = s.pipe; }
    return FLUTE_OK;
}

// Lean one-row kernel (qgemm_fast.h, round 5): 4 bits, M = 1, K = 512 * D * KW a power of two.  Shapes (waves per workgroup, waves
// per unit row, pieces per wave) by K, first choice first - measured in tools/ubench/oneshot_lab (profiles/r05/fast_lab_run*.jsonl;
// us per launch next to the round-4 one-shot kernel in the same harness): K = 4096: (4, 1, 8) 4.24 / (8, 2, 4) 4.35 against 4.43
// on 4096 x 4096, 7.49 / 7.50 against 8.63 on 4096 x 11008; K = 8192: (8, 2, 8) 6.50 on 8192 x 4096 (g = 128).  rank = the
// template's Stages - 2.
int plan_fast(const Call& call, int rank, int want_waves, flute_plan* p, OneArgs* oa) {
    const int bits = call.bits, lg = call.lg, M = call.M, N = call.N, K = call.K, num_sms = call.num_sms;
    if (bits != 4 || M < 1 || M > 4 || lg < 6 || lg > 8) return FLUTE_ERR_SHAPE;
    int mb = 1; while (mb < M) mb <<= 1;                       // rows per pass: 1, 2, 4
    struct Shape { int W, KW, D; };
    std::vector<Shape> c;
    if (K == 2048) c = {{4, 1, 4}};
    else if (K == 3584) c = {{4, 1, 7}};                       // (Gemma-2-9B: 7 pieces per wave)
    else if (K == 4096) {
        // one round of workgroups (<= one per CU): a wave per unit row, no cross-wave sum (4096^2: 4.05 us against 4.16 with
        // 8 waves); more rounds: two waves per SIMD hide each other's stalls (11008: 6.86 against 6.97, 5120: 4.90 / 5.15,
        // 8192: 5.46 / 5.54 - profiles/r05/time_cases_lean_shapes.jsonl)
        if (N / 16 <= num_sms) c = {{4, 1, 8}, {8, 2, 4}};
        else c = {{8, 2, 4}, {4, 1, 8}};
    } else if (K == 8192) c = {{8, 2, 8}};
    else return FLUTE_ERR_SHAPE;
    Shape sh = c[std::min((size_t)std::max(0, rank), c.size() - 1)];
    if (want_waves > 0) {                                     // override `waves` picks the shape with that many waves
        bool found = false;
        for (const Shape& x : c) if (x.W == want_waves) { sh = x; found = true; break; }
        if (!found) return FLUTE_ERR_SHAPE;
    }
    // (built for the rows whose activations fit beside the table image, mb * K * 2 <= 32 KB: not four rows of K = 8192)
    if (!fast_fn(call, sh.W, sh.KW, sh.D, mb)) return FLUTE_ERR_SHAPE;
    const int units = N / 4, upw = sh.W / sh.KW;
    if (units % upw) return FLUTE_ERR_SHAPE;
    if (((size_t)N * (size_t)(K >> lg)) * 2 >= (size_t)0xfffffff0u || (size_t)units * K * 2 >= ((size_t)1 << 40)) return FLUTE_ERR_SHAPE;
    memset(p, 0, sizeof(*p));
    p->family = 0;
    p->m_block = mb; p->waves = sh.W; p->kw = sh.KW; p->splitk = 1; p->k_per_split = K;
    p->grid = (unsigned)(units / upw); p->block = (unsigned)(sh.W * 64);
    p->lds_bytes = fast_lds_bytes(sh.W, sh.KW, sh.D, lg, mb); p->lut_copies = 32;
    p->ring_depth = sh.D; p->visits = 1; p->k_chunks = 1; p->one_shot = 4;
    if (oa) { memset(oa, 0, sizeof(*oa)); oa->lg = lg; oa->lkw = ilog2(sh.KW); oa->upw = upw; oa->pk = sh.D; oa->depth = sh.D; oa->pipe = 1; }
    return FLUTE_OK;
}

// Lean MFMA decode kernel (qgemm_fastm.h, round 5): 4 bits, M <= 16, K = 4096 (8 waves x 512 k) or 2048 (8 x 256 k), a workgroup =
// 4 unit rows (16 columns) x all of K; every wave's K range must hold >= 2 groups (its scale words are read as whole dwords).
// Round 6: ng column groups (4 unit rows each) per workgroup share one staged activation set: the smallest of 1, 2, 3 that covers the
// layer in one round of workgroups (override slabs_per_wave = 1 / 2 / 3 fixes it).
int plan_fastm(const Call& c, int ng_ovr, flute_plan* p, OneArgs* oa) {
    const int bits = c.bits, lg = c.lg, M = c.M, N = c.N, K = c.K, num_sms = c.num_sms;
    if (bits != 4 || M < 1 || M > 16 || (K != 4096 && K != 2048)) return FLUTE_ERR_SHAPE;
    const int W = 8, nm = K / (128 * W);
    if (!fastm_fn(c, W, nm, lg, 1)) return FLUTE_ERR_SHAPE;      // group sizes 64 .. 256 that leave a wave's K range >= 2 groups
    const int units = N / 4;
    if (units % 4) return FLUTE_ERR_SHAPE;
    int ng = 1;
    while (ng < 3 && ceil_div(units / 4, ng) > num_sms) ++ng;
    if (ng_ovr >= 1 && ng_ovr <= 3) ng = ng_ovr;
    if (((size_t)N * (size_t)(K >> lg)) * 2 >= (size_t)0xfffffff0u || (size_t)units * K * 2 >= ((size_t)1 << 40)) return FLUTE_ERR_SHAPE;
    memset(p, 0, sizeof(*p));
    p->family = kFamilyFastM;
    p->m_block = 16; p->m_tiles = 1; p->slabs_per_wave = ng; p->waves = W; p->kw = W; p->splitk = 1; p->k_per_split = K;
    p->grid = (unsigned)ceil_div(units / 4, ng); p->block = (unsigned)(W * 64);
    p->lds_bytes = fastm_lds_bytes(K); p->lut_copies = 32;
    p->ring_depth = nm; p->visits = 1; p->k_chunks = 1; p->one_shot = 0;
    if (oa) { memset(oa, 0, sizeof(*oa)); oa->lg = lg; oa->depth = nm; }
    return FLUTE_OK;
}

// Persistent MFMA decode kernel (qgemm_persistm.h, round 6): 4 bits, M <= 16, K a multiple of 128 (>= 1024), group size 64 / 128.  A set =
// ng column groups (16 columns each); the sets are dealt round-robin to `grid` workgroups, `visits` sets each (the last round may be short);
// grid = the fewest workgroups that keep `visits` whole rounds.  ng (override slabs_per_wave) by the model below (ties: the smaller); visits by override m_tiles.
// Model (us; fitted to profiles/r06/call31_persistm_xr.log): the kernel is bound by a wave's in-order issue, not by HBM - a macro-step (128 k
// of ng groups) costs a wave 0.45 / 0.9 / 1.3 us for ng = 1 / 2 / 3 plus 0.04 / 0.135 / 0.35 us for its 1 / 2 / 4 activation requests, the
// busiest workgroup runs `visits` sets of ceil(K / 1024) macro-steps; never below the weights at 5.3 TB/s; 3.5 us fixed.
static double persistm_model_us(int M, int N, int K, int num_sms, int ng, int* grid_out, int* visits_out, int visits_ovr) {
    const int groups = N / 16;
    const int nsets = ceil_div(groups, ng);
    int visits = ceil_div(nsets, num_sms);
    if (visits_ovr >= 1) visits = visits_ovr;
    int grid = ceil_div(nsets, visits);
    if (grid > num_sms) { grid = num_sms; visits = ceil_div(nsets, grid); }
    static const double a_ng[4] = {0, 0.45, 0.9, 1.3};
    const double b_x = M <= 4 ? 0.04 : (M <= 8 ? 0.135 : 0.35);
    const double issue = (double)visits * ceil_div(K, 1024) * (a_ng[ng] + b_x);
    const double hbm = ((double)N * K / 2) / 5.3e6;
    if (grid_out) *grid_out = grid;
    if (visits_out) *visits_out = visits;
    return 3.5 + (hbm > issue ? hbm : issue);
}
int plan_persistm(const Call& c, int ng_ovr, int visits_ovr, int xres_ovr, flute_plan* p, OneArgs* oa) {
    const int bits = c.bits, lg = c.lg, M = c.M, N = c.N, K = c.K, num_sms = c.num_sms;
    // (sixteen waves per workgroup - four per SIMD, rings three deep - measured slower than eight on every layer: 28672 x 8192 M = 4 32.1 against
    // 31.1 us, 8192^2 13.3 against 11.1, profiles/r06/call33_persistm_16_waves_dropped.log; the kernel keeps the template parameter)
    // (group size 128: a column's scale row must be a whole number of dwords - the macro-step's 4-B scale request)
    if ((bits != 4 && bits != 2) || M < 1 || M > 16 || lg < 6 || lg > 7 || K % 128 || (lg == 7 && K % 256) || K < 1024 || N % 16) return FLUTE_ERR_SHAPE;
    if ((size_t)N * K * bits / 8 >= (size_t)0xfffffff0u || (size_t)N * (size_t)(K >> lg) * 2 >= (size_t)0xfffffff0u || (size_t)M * K * 2 >= (size_t)0xfffffff0u)
        return FLUTE_ERR_SHAPE;
    // Column groups per set (profiles/r06/planner_regret_persistm*.json).  M <= 8: one, unless a wave's stream is long - visits x macro-steps
    // >= 40 at one group per set (8192 x 28672, 28672 x 8192: two groups 28.4 against 31.1 us, 30.3 against 30.9; 8192^2, 16 macro-steps: one group
    // 10.9 against 12.5, 10240 x 8192 14.1 against 16.7).  M > 8, where every set pulls 16 rows of activations: by the model.
    int ng = 1, grid = 0, visits = 0;
    if (M <= 8) {
        const int groups = N / 16;
        if (groups > num_sms && (long)ceil_div(groups, num_sms) * ceil_div(K, 1024) >= 40) ng = 2;
    } else {
        double best = 0;
        for (int c = 1; c <= 3; ++c) {
            const double us = persistm_model_us(M, N, K, num_sms, c, nullptr, nullptr, visits_ovr);
            if (c == 1 || us < best * 0.98) { best = us; ng = c; }
        }
    }
    if (ng_ovr >= 1 && ng_ovr <= 3) ng = ng_ovr;
    // an override of the sets per workgroup that would need more workgroups than CUs cannot apply: refused, not replaced
    if (visits_ovr >= 1 && ceil_div(ceil_div(N / 16, ng), visits_ovr) > num_sms) return FLUTE_ERR_SHAPE;
    (void)persistm_model_us(M, N, K, num_sms, ng, &grid, &visits, visits_ovr);
    memset(p, 0, sizeof(*p));
    p->family = kFamilyPersistM;
    p->m_block = 16; p->m_tiles = 1; p->slabs_per_wave = ng; p->waves = 8; p->kw = 8; p->splitk = 1; p->k_per_split = K;
    p->grid = (unsigned)grid; p->block = 512u;
    const int xr = M <= 4 ? 1 : (M <= 8 ? 2 : 4);                  // activation requests per macro-step (4 rows each)
    // activations resident in LDS (staged once per workgroup, no activation request in the loop) where 4 xr rows x K fit in 64 KB beside the rest
    // and that member is built; override one_shot = 0 keeps the rings
    const bool xres = (long)K * xr <= 8192 && xres_ovr != 0 && persistm_fn(c, lg, ng, xr, 8, 1);
    p->lds_bytes = persistm_lds_bytes(ng, xr, 8, xres, bits); p->lut_copies = 32;
    p->ring_depth = PM_DW; p->visits = visits; p->k_chunks = xr; p->one_shot = xres ? 1 : 0;
    if (oa) { memset(oa, 0, sizeof(*oa)); oa->lg = lg; oa->depth = PM_DW; }
    return FLUTE_OK;
}

// Persistent one-shot kernel (qgemm_persist.h): W <= 8 waves per workgroup, each wave walks `visits` units of `k_chunks`
// segments (D pieces each; D = 4, 3 bits: 2 - halved while K is not a whole number of segments).  Shapes (W, workgroups
// per CU) are ranked by what tools/decode_lab.py time_persist_shape measured on the 8192 x 28672-class layers
// (profiles/r03/persist_lab_shapes.jsonl): first the unit rows the BUSIEST CU decodes (ceil(grid / CUs) x W x visits: the
// lookups are a per-CU cost - 3-bit layers are bound by it - so a grid of 299 workgroups on 256 CUs costs what 512 would:
// 42 us against 25.7 on 28672 x 8192 W3), then the launch closest to EIGHT waves per CU (7 - 8 waves per CU x 4 visits
// beat 14 - 16 x 2 by 4 - 6 %, 4 per CU lose 20 %), then the larger workgroup (fewer table images).
// Stages 2..5 -> rank 0..3.
int plan_persist(const Call& c, const Ovr& ov, flute_plan* p, OneArgs* oa) {
    const int bits = c.bits, lg = c.lg, M = c.M, N = c.N, K = c.K, num_sms = c.num_sms;
    const flute_template_info& t = c.t;
    if (M < 1 || M > 2 || lg < 6 || ((K >> lg) & 1) || K % 512) return FLUTE_ERR_SHAPE;
    int mb = 1; while (mb < M) mb <<= 1;                      // rows per pass (their staged activations must fit LDS: below)
    const int J = (bits == 3) ? 16 : 16 / bits;
    const int units = N / J;
    const int npieces = K / 512;
    const int NS = 2;
    auto built = [&](int d) { return persist_fn(c, mb, d, NS, 0) != nullptr; };
    int D = 4;                                                // the deepest built segment: 4 pieces, 3 bits 2
    while (D > 2 && (!built(D) || npieces % D)) D /= 2;
    if ((ov.depth == 2 || ov.depth == 4) && built(ov.depth)) D = ov.depth;
    if (npieces % D) return FLUTE_ERR_SHAPE;
    const int nch = npieces / D;
    if (nch > 255) return FLUTE_ERR_SHAPE;
    const int runs = oneshot_lut_runs(bits);
    const int wcap = std::min(t.threads, 512) / 64;
    struct Shape { int W, nwg, nvis; long load, off8; size_t lds; };
    std::vector<Shape> cands;
    for (int W = wcap; W >= 4; --W) {
        if (ov.waves > 0 && W != std::min(ov.waves, wcap)) continue;
        if (bits != 2 && ceil_div(runs, W) > 8) continue;
        const size_t lds = persist_lds_bytes(bits, mb, D, NS, lg, K, W);
        if (lds > (size_t)kMaxLds) continue;
        const int per_cu = std::max(1, std::min((int)((size_t)kMaxLds / lds), 16 / W));
        for (int c = 1; c <= per_cu; ++c) {
            if (ov.m_tiles > 0 && c != ov.m_tiles) continue;  // lab: workgroups per CU
            const int nvis = ceil_div(units, c * num_sms * W);
            const int nwg = ceil_div(units, W * nvis);
            bool dup = false;
            for (const Shape& o : cands) dup = dup || (o.W == W && o.nwg == nwg);
            if (dup) continue;
            cands.push_back(Shape{W, nwg, nvis, (long)ceil_div(nwg, num_sms) * W * nvis,
                                  std::labs((long)ceil_div(nwg, num_sms) * W - 8L), lds});
        }
    }
    if (cands.empty()) return FLUTE_ERR_SHAPE;
    std::stable_sort(cands.begin(), cands.end(), [](const Shape& a, const Shape& b) {
        if (a.load != b.load) return a.load < b.load;
        if (a.off8 != b.off8) return a.off8 < b.off8;
        return a.W > b.W;
    });
    size_t pick = std::min((size_t)std::max(0, t.stages - 2), cands.size() - 1);
    if (ov.waves > 0 || ov.m_tiles > 0) pick = 0;
    const Shape& best = cands[pick];
    p->family = 0;
    p->m_block = mb; p->waves = best.W; p->kw = 1; p->splitk = 1; p->k_per_split = K;
    p->grid = (unsigned)best.nwg; p->block = (unsigned)(best.W * 64);
    p->lds_bytes = best.lds; p->lut_copies = 32;
    p->ring_depth = D; p->visits = best.nvis; p->k_chunks = nch; p->one_shot = 3;
    if (oa) { oa->lg = lg; oa->lkw = 0; oa->upw = best.W; oa->pk = D; oa->ipw = ceil_div(runs, best.W); oa->depth = D; oa->pipe = 1;
              oa->nvis = best.nvis; oa->nch = nch; oa->nwg = best.nwg; oa->nsets = NS; }
    return FLUTE_OK;
}

// Skinny MFMA kernel (qgemm_skinny.h): 4-bit, M <= 16.  A wave = one slab (16 units) x D k-steps, the 4 or 8 waves of a
// workgroup share a K slice of the slab, so K = splitk x 32 D KW with D in {4, 8, 16}; splitk > 1 (round 4): the slices of a
// slab are neighbouring workgroups and meet through the workspace inside the launch (xwg.h, L form).
int plan_skinny(const Call& c, const Ovr& ov, flute_plan* p, OneArgs* ka) {
    const int bits = c.bits, lg = c.lg, M = c.M, N = c.N, K = c.K;
    const size_t workspace_bytes = c.workspace_bytes;
    if (bits != 4 || M < 1 || M > 16 || lg < 5 || ((K >> lg) & 1) || K % 128) return FLUTE_ERR_SHAPE;
    const int units = N / 4;
    if (units % 16) return FLUTE_ERR_SHAPE;
    if ((size_t)units * K * 2 >= (size_t)0xfffffff0u || (size_t)(M + 16) * K * 2 >= (size_t)0x7ffffff0u) return FLUTE_ERR_SHAPE;
    const int sk = ov.splitk > 1 ? ov.splitk : 1;
    if (sk > 1) {
        // slabs: 4 KB (four 16 x 16 fp32 tiles in fragment order) per slab and slice
        if (sk > 16 || (K / 32) % sk || units / 16 > kXwgMaxTiles || (size_t)sk * (units / 16) * 4096 > slab_room(workspace_bytes) ||
            (size_t)sk * (units / 16) * 4096 >= ((size_t)1 << 31))
            return FLUTE_ERR_SHAPE;
    }
    const int ksteps = K / 32 / sk;
    int KW = 0, D = 0;
    for (int kw : {8, 4}) {
        if (ov.waves > 0 && kw != ov.waves) continue;
        if (ksteps % kw) continue;
        const int d = ksteps / kw;
        if (!skinny_fn(c, d) || ((d * 32) >> lg) > 8) continue;
        KW = kw; D = d;
        break;
    }
    if (!KW) return FLUTE_ERR_SHAPE;
    p->family = kFamilySkinny;
    p->m_block = 1; p->m_tiles = 1; p->slabs_per_wave = 1; p->waves = KW; p->kw = KW; p->splitk = sk;
    p->k_per_split = K / sk;
    p->grid = (unsigned)(units / 16 * sk); p->block = (unsigned)(KW * 64);
    p->lds_bytes = skinny_lds_bytes(4, 1, KW); p->lut_copies = 32; p->ring_depth = D; p->visits = 1; p->k_chunks = 1; p->one_shot = 0;
    p->splitk_mode = sk > 1 ? 1 : 0;
    p->workspace_needed = sk > 1 ? (size_t)sk * (units / 16) * 4096 + kXwgFlagBytes : 0;
    if (ka) { memset(ka, 0, sizeof(*ka)); ka->lg = lg; ka->lkw = ilog2(KW); ka->ipw = ceil_div(oneshot_lut_runs(4), KW); ka->depth = D; }
    return FLUTE_OK;
}

// Split-K block kernel (qgemm_splitk.h): 128 x 128 tiles x `splitk` K slices, one workgroup each; the slices of a tile are
// neighbours in the block order (dispatched together), the row tiles of a column tile follow each other.  Legal splits:
// K / splitk a multiple of 2 x max(64, group) (two K halves per workgroup, each whole 64-k steps and whole groups), at
// most four 8-group scale blocks per K half, slabs + state words inside the workspace.  Cost model (us, measured on
// MI355X, profiles/r04/splitk_lab*.jsonl): rounds x (fixed + steps x per-step) + seam.
int plan_splitk(int bits, int lg, int M, int N, int K, int num_sms, const Ovr& ov, size_t workspace_bytes, flute_plan* p,
                int rank, double* cost_us) {
    if (bits != 2 && bits != 4) return FLUTE_ERR_SHAPE;
    const int g = 1 << lg, G = K >> lg;
    if (G % 8 || N % 128 || K % 128) return FLUTE_ERR_SHAPE;
    if ((size_t)(M + 128) * K * 2 >= (size_t)0xfffffff0u || (size_t)N * G * 2 >= (size_t)0xfffffff0u) return FLUTE_ERR_SHAPE;
    // Row tiles per workgroup: 8 (128-row tiles) or 4 (64-row tiles: twice the tiles, half the slab per slice, every weight
    // dequantised by twice as many workgroups); override m_tiles = 8 / 4 fixes it, else both are priced.  K parts per workgroup
    // (round 6): 2 (128-column tiles: four column groups x two K halves) or - 64-row tiles only - 4 (64-column tiles: two column groups
    // x four K quarters: twice the tiles with NO more K slices, i.e. M = 256 on 4096 x 4096 as 256 workgroups without a seam; twice
    // the activation bytes per workgroup); override kw = 2 / 4 fixes it.
    auto tiles_of = [&](int rt, int kp) { return (long)ceil_div(M, rt * 16) * (N / (256 / kp)); };
    auto slab_of = [&](int rt, int kp) { return (long)rt * 16384 / kp; };      // fp32 partial tile in fragment order: 8 waves x rt / kp row tiles x 2 KB
    auto legal = [&](int sk, int rt, int kp) {
        const int align = kp * std::max(64, g);                // every K part: whole 64-k steps and whole groups
        if (sk < 1 || sk > 16 || K % sk || (K / sk) % align) return false;
        if (tiles_of(rt, kp) > kXwgMaxTiles) return false;
        const int gw = (K / sk) >> lg;                         // groups of a workgroup's K range: one scale image of eight 8-group blocks per column group
        if (gw + ((gw % 8) ? 7 : 0) > 64) return false;
        const size_t slabs = (size_t)sk * tiles_of(rt, kp) * slab_of(rt, kp);
        if (sk > 1 && (slabs > slab_room(workspace_bytes) || slabs >= ((size_t)1 << 31))) return false;
        return true;
    };
    // us, fitted to tools/splitk_lab.py on MI355X (profiles/r04/splitk_lab_run8*.jsonl, run9*): a round of workgroups costs ~9.5 us
    // of launch, prologue, K-half exchange, ramp and stores + per 64-k step 0.65 .. 0.96 us (128-row tiles: 30.3 us on 64 CUs,
    // 32.9 on 172, 39.3 on 224, 40.3 on 256 at K = 4096 - the more of the chip is busy the slower) or 0.44 .. 0.52 us (64-row
    // tiles: 23.9 us on 128 CUs, 26.5 on 256); the seam grows with the MB published write-through (E form at 2 slices
    // ~1 + 0.15 / MB, 4 slices and the L form ~1.5 + 0.5 / MB)
    auto model_us = [&](int sk, int rt, int kp) {
        const long wgs = tiles_of(rt, kp) * sk;
        // a last, partly filled round costs less than a whole one (round 6: M = 384 on 8192^2, 128-row tiles x 2 slices = 1.5 rounds: 68 us
        // measured, 83 priced at two whole rounds - and the cheaper-looking 64-row plan, three whole rounds, ran 81): the mean of
        // the whole rounds and the exact share (profiles/r06_planner_regret_between_final.json)
        const double whole = (double)((wgs + num_sms - 1) / num_sms);
        const double rounds = wgs <= (long)num_sms ? 1.0 : 0.5 * (whole + (double)wgs / num_sms);
        const double fill = std::min(1.0, (double)wgs / num_sms);
        const double steps = (double)K / sk / (64.0 * kp);     // 64-k steps of a K part
        const int hr = rt / kp;
        const bool eform = (sk == 2 && hr % 2 == 0) || (sk == 4 && hr % 4 == 0);
        const double mb = sk == 1 ? 0.0 : (double)wgs * (slab_of(rt, kp) * 1e-6) * (eform ? (sk - 1.0) / sk : 1.0);
        // (L form on 32-KB slabs, measured at M = 48 .. 96: 2.2 us at four slices / 3.4 at eight of 8.4 MB - profiles/r04/splitk_64_row_tiles_below_m128.json)
        const double seam = sk == 1 ? 0.0 : (sk == 2 && eform ? 1.0 + 0.15 * mb : (rt == 4 ? 1.5 + 0.15 * mb : 1.5 + 0.5 * mb));
        const double step = rt == 8 ? 0.65 + 0.31 * fill * fill * fill : 0.44 + 0.08 * fill * fill * fill;
        // four K parts (64 x 64 tiles, round 6; tools/splitk_lab.py time_kp4, profiles/r06/call1_*.log, call16_*.log): a round costs 6.0 us
        // + 0.6 us per step whatever share of the chip is busy (16 steps: 15.5 us on 256 CUs, 15.4 on 128, 15.5 on 64; 32 steps 25.1;
        // 8 steps + the L-form seam of two slices 12.6)
        if (kp == 4) return rounds * (6.0 + steps * 0.6) + seam;
        return rounds * (9.5 + steps * step) + seam;
    };
    struct Cand { double us; int sk, rt, kp; };
    std::vector<Cand> c;
    for (int kp : {2, 4}) {
        if ((ov.kw == 2 || ov.kw == 4) && kp != ov.kw) continue;
        for (int rt : {8, 4}) {
            if ((ov.m_tiles == 8 || ov.m_tiles == 4) && rt != ov.m_tiles) continue;
            if (kp == 4 && rt != 4) continue;                  // four K parts: 64-row tiles only (LDS)
            for (int sk = 1; sk <= 16; ++sk) {
                if (ov.splitk > 0 && sk != ov.splitk) continue;
                if (legal(sk, rt, kp)) c.push_back(Cand{model_us(sk, rt, kp), sk, rt, kp});
            }
        }
    }
    if (c.empty()) return FLUTE_ERR_SHAPE;
    std::stable_sort(c.begin(), c.end(), [](const Cand& x, const Cand& y) { return x.us < y.us; });
    const Cand best = c[std::min((size_t)std::max(0, rank), c.size() - 1)];
    if (cost_us) *cost_us = best.us;
    memset(p, 0, sizeof(*p));
    p->family = kFamilySplitK;
    // four loader waves beside the eight compute waves (round 4: K = 4096 per workgroup 34.1 -> 30.3 us on 64 CUs, 35.2 -> 32.9 on
    // 172, 41.8 -> 40.3 on 256; the variant without them - override waves = 8 - was dropped in round 6)
    if (ov.waves > 0 && ov.waves != 12) return FLUTE_ERR_SHAPE;
    const int ldw = SK_LOADERS;
    // m_block: row tiles of a column tile per XCD group (block order of launches without K slices); override 1 / 2 / 4 / 8
    {
        const int tm = ceil_div(M, best.rt * 16);
        // (round 6: as many of a column tile's row tiles as divide them, up to eight - M = 256 on 4096^2, four 64-row tiles: 16.4 / 15.9 / 15.6 us
        // at 1 / 2 / 4 per group, profiles/r06/call20_*.log; M = 512 on 2048 x 4096: 16.4 / 16.3 / 16.1 / 16.1 at 1 / 2 / 4 / 8)
        int E = 8;
        while (E > 1 && (tm % E || ((tm / E) & (tm / E - 1)))) E >>= 1;
        if (ov.m_block == 1 || ov.m_block == 2 || ov.m_block == 4 || ov.m_block == 8) E = ov.m_block;
        if (best.sk != 1 || tm % E || ((tm / E) & (tm / E - 1))) E = 1;
        p->m_block = E;
    }
    p->m_tiles = best.rt; p->slabs_per_wave = 1; p->waves = 8 + ldw; p->kw = best.kp;
    p->splitk = best.sk; p->k_per_split = K / best.sk;
    p->grid = (unsigned)(tiles_of(best.rt, best.kp) * best.sk); p->block = (unsigned)(512 + 64 * ldw);
    p->lds_bytes = (size_t)splitk_lds_bytes(bits, best.rt, best.kp); p->lut_copies = 32;
    p->splitk_mode = best.sk > 1 ? 1 : 0;
    p->workspace_needed = best.sk > 1 ? (size_t)best.sk * tiles_of(best.rt, best.kp) * slab_of(best.rt, best.kp) + kXwgFlagBytes : 0;
    return FLUTE_OK;
}

int plan_stream(int dtype, int bits, int lg, int M, int N, int K, int num_sms, const flute_template_info& t,
                const Ovr& ov, size_t workspace_bytes, flute_plan* p, StreamArgs* sa) {
    const int J = (bits == 3) ? 16 : 16 / bits;
    const int units = N / J;
    const int G = K >> lg;
    int mb = 1; while (mb < M) mb <<= 1;
    const int dec_max = 4;
    if (ov.m_block > 0 && ov.m_block >= M && ov.m_block <= dec_max) mb = floor_pow2(ov.m_block);
    int depth = (bits == 3) ? 2 : (t.sms_multiple == 1 ? 4 : 2);
    if (ov.depth == 2 || (ov.depth == 4 && bits != 3)) depth = ov.depth;
    const int threads_cap = std::min(t.threads, stream_max_threads(bits, mb, depth));
    const int wcap = threads_cap / 64;

    // grid-level K split only for layers too narrow to give every CU eight waves even at the deepest
    // in-workgroup split
    int splitk = 1;
    while ((long)units * 16 * splitk < (long)num_sms * 8 && K / (splitk * 2) >= 1024) splitk *= 2;
    if (ov.splitk > 0) splitk = ov.splitk;
    const int align_k = std::max(512, 8 << lg);
    int kps = round_up(ceil_div(K, splitk), align_k);
    splitk = ceil_div(K, kps);
    while (splitk > 1 && (size_t)splitk * M * N * 4 > workspace_bytes) {
        splitk >>= 1;
        kps = round_up(ceil_div(K, splitk), align_k);
        splitk = ceil_div(K, kps);
    }
    if (splitk == 1) kps = round_up(K, 512);
    const int krange = std::min(K, kps);
    const bool split_aligned = splitk == 1 || kps % (8 << lg) == 0;

    std::vector<StreamShape> cands;
    for (int W = 1; W <= wcap; ++W) {
        if (ov.waves > 0 && W != std::min(ov.waves, wcap)) continue;
        for (int kw = 1; kw <= W; kw <<= 1) {
            if (W % kw) continue;
            if (ov.kw > 0 && kw != std::min(floor_pow2(ov.kw), floor_pow2(W))) continue;
            StreamShape s;
            if (stream_shape(bits, mb, lg, units, krange, G, split_aligned, num_sms, W, kw, threads_cap, &s))
                cands.push_back(s);
        }
    }
    if (cands.empty()) return FLUTE_ERR_SHAPE;
    // shapes of fewer than 8 waves are only worth ranking when nothing larger exists
    if (ov.waves <= 0) {
        const int wmin = std::min(8, wcap);
        bool any = false;
        for (const StreamShape& c : cands) any = any || c.W >= wmin;
        if (any) cands.erase(std::remove_if(cands.begin(), cands.end(), [&](const StreamShape& c) { return c.W < wmin; }),
                             cands.end());
    }
    std::stable_sort(cands.begin(), cands.end(), [](const StreamShape& a, const StreamShape& b) {
        if (a.cost != b.cost) return a.cost < b.cost;
        if (a.W != b.W) return a.W > b.W;
        return a.kw < b.kw;
    });
    // Stages 2..5 -> rank 0..3 among shapes that differ in (W, kw); explicit overrides leave one candidate
    size_t pick = std::min((size_t)std::max(0, t.stages - 2), cands.size() - 1);
    if (ov.waves > 0 || ov.kw > 0) pick = 0;
    const StreamShape& s = cands[pick];

    p->family = 0;
    p->m_block = mb; p->waves = s.W; p->kw = s.kw; p->splitk = splitk;
    p->k_per_split = (splitk == 1) ? K : kps;
    p->grid = (unsigned)(s.nwg * splitk);
    p->block = (unsigned)(s.W * 64);
    p->lds_bytes = s.total;
    p->lut_copies = 32;
    p->ring_depth = depth; p->visits = s.visits; p->k_chunks = s.nchunks;
    p->one_shot = 0;
    if (sa) {
        memset(sa, 0, sizeof(*sa));
        sa->M = M; sa->N = N; sa->K = K; sa->G = G; sa->lg = lg;
        sa->units = units; sa->ngroups = s.ngroups;
        sa->upw = s.upw; sa->kw = s.kw; sa->lkw = ilog2(s.kw);
        sa->nwg = s.nwg; sa->vis_q = s.ngroups / s.nwg; sa->vis_r = s.ngroups % s.nwg;
        sa->splitk = splitk; sa->k_per_split = kps;
        sa->kc = s.kc; sa->nchunks = s.nchunks; sa->kx = s.kx;
        sa->x_off = (int)s.x_off; sa->s_off = (int)s.s_off; sa->red_off = (int)s.red_off;
        sa->s_wave_bytes = s.s_wave_bytes; sa->s_fast = s.s_fast;
    }
    (void)dtype;
    return FLUTE_OK;
}

}  // namespace flute_amd::host
