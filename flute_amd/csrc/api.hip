// Host side of the C ABI (include/flute_amd.h): template table, launch planning
// and dispatch.  Mirrors the role of flute/csrc/qgemm.cpp:39-83 (qgemm_raw) +
// qgemm_kernel_raw_generated.cu:15-768 (_qgemm_raw's template switch) +
// qgemm_kernel.hpp:824-939 (qgemm_host), re-thought for gfx950: instead of one
// Stream-K kernel with 36/144 tile variants there are several kernel families (flute_plan::family: decode kernels for a few
// rows, per-wave / skinny / split-K / block-tiled MFMA kernels above) whose launch geometry is derived
// from the template's knobs and the problem shape.  Nothing here is process-global mutable state
// except the per-device "large LDS granted" cache (mutex-guarded): plan overrides travel with the call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <mutex>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/flute_amd.h"
#include "kernels.h"
#include "qgemm_stream.h"
#include "qgemm_persist.h"
#include "qgemm_fast.h"
#include "qgemm_fastm.h"
#include "qgemm_persistm.h"
#include "qgemm_skinny.h"
#include "mfma.h"
#include "qgemm_tile.h"
#include "qgemm_block.h"
#include "grouped_rows.h"
#include "qgemm_splitk.h"

using namespace flute_amd;

namespace {

// had8: set by flute_qgemm_hadamard for M <= 4 - the DECODE planners then prefer 8-wave workgroups (the fused rotation is
// done by the workgroup's waves, 512 k each); it never reaches the MFMA planners, whose wave count is the template's
struct Ovr { int family, m_block, waves, kw, splitk, m_tiles, slabs, depth, one_shot, had8; };
Ovr ovr_of(const flute_overrides* o) {
    if (!o) return Ovr{-1, -1, -1, -1, -1, -1, -1, -1, -1, 0};
    return Ovr{o->family, o->m_block, o->waves, o->kw, o->splitk, o->m_tiles, o->slabs_per_wave, o->ring_depth, o->one_shot, 0};
}

constexpr int kMaxLds = 160 * 1024;
constexpr size_t kTileInLaunchMax = 4 << 20;    // bytes of slabs up to which the per-wave kernel's K slices meet inside the launch (plan_tile)
constexpr int kFamilyBlock = 3;                 // block-tiled prefill kernel (qgemm_block.h)
constexpr int kFamilySkinny = 5;                // registers-only MFMA kernel for 3 <= M <= 32 (qgemm_skinny.h)
constexpr int kFamilySplitK = 6;                // 128 / 64 x 128 / 64 tiles, K split over workgroups, combined in the launch (qgemm_splitk.h)
constexpr int kFamilyFastM = 7;                 // lean MFMA decode kernel: 4 unit rows x all of K per workgroup, M <= 16 (qgemm_fastm.h)
constexpr int kFamilyPersistM = 8;              // persistent MFMA decode kernel: workgroups stream column-group sets x all of K, M <= 16 (qgemm_persistm.h)
// Workspace layout (every kernel): [0, kXwgFlagBytes) tile state words of the in-launch reductions (xwg.h; zero between
// calls), fp32 slabs behind them.  A planner sees the room behind the state words only.
size_t slab_room(size_t workspace_bytes) { return workspace_bytes > kXwgFlagBytes ? workspace_bytes - kXwgFlagBytes : 0; }

int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
int floor_pow2(int v) { int p = 1; while (p * 2 <= v) p *= 2; return p; }
int ceil_div(int a, int b) { return (a + b - 1) / b; }
// 3-bit skinny blocks (64 rows x the K split the launcher will pick) on at least 80 % of the CUs?  Up to M = 48 the per-wave kernel
// (three row tiles per wave) wins where they do not: 10240 x 8192 M = 48, 40 blocks x 4 slices = 160 workgroups, 44.5 us against 32.4;
// with 224 - 256 workgroups the blocks win by 3 - 24 % (8192^2, 28672 x 8192, 8192 x 28672, 14336 x 4096, 4096 x 14336:
// profiles/r05_planner_regret_between_*.json)
bool skinny3_fills(int M, int col_blocks, int K, int lg, int num_sms) {
    const long tiles = (long)ceil_div(M, 64) * col_blocks;
    const int align_k = std::max(64, 8 << lg);
    long sk = 1;
    while (tiles * sk * 2 <= (long)num_sms && K / (sk * 2) >= std::max(256, align_k)) sk *= 2;
    return tiles * sk * 5 >= (long)num_sms * 4;
}
int round_up(int a, int b) { return ceil_div(a, b) * b; }
// rows of a block-kernel configuration (flute_plan::m_block of family 3): 4 / 5 = 256 / 128 rows,
// 8 + RT = the skinny 3-bit blocks of RT row tiles
int block_rows(int cfg) { return cfg >= 8 ? (cfg - 8) * 16 : ((cfg & 1) ? 128 : 256); }

// Template id -> knobs.  Enumeration order is the reference's
// (flute/codegen_utils.py:110-152): SMs_Multiple {1,2,4} x tile {0,1,2} x
// stages {2,3,4,5} x (b=4 only) QuantMapMode {Vectorized,_32,_16,_8}; tile 0
// has TileP 64, tiles 1,2 TileP 32, so id -> TileP is identical to the
// reference table and reference-packed weights keep their id.
bool decode_template(int bits, int id, flute_template_info* t) {
    if (bits != 2 && bits != 3 && bits != 4) return false;
    const int nq = (bits == 4) ? 4 : 1;
    const int total = 3 * 3 * 4 * nq;
    if (id < 0 || id >= total) return false;
    const int q = id % nq;
    const int st = (id / nq) % 4;
    const int tile = (id / (nq * 4)) % 3;
    const int mult = id / (nq * 12);
    static const int kMult[3] = {1, 2, 4};
    static const int kThreads[3] = {1024, 1024, 512};
    static const int kTileM[3] = {64, 64, 16};
    static const int kTileP[3] = {64, 32, 32};
    static const int kCopies[4] = {1, 32, 16, 8};
    t->num_bits = bits;
    t->template_id = id;
    t->sms_multiple = kMult[mult];
    t->threads = kThreads[tile];
    t->tile_m = kTileM[tile];
    t->tile_k = 64;
    t->tile_p = kTileP[tile];
    t->stages = 2 + st;
    // the reference's QuantMapMode slot; b=2/3 templates have none
    t->lut_copies = (bits == 4) ? kCopies[q] : 32;
    return true;
}

// What every entry point checks of a layer (check_layer), and one planner call: the layer, the shape, the CU count, the workspace
// and the overrides.
struct Layer { int bits, lg, J, units; flute_template_info t; };
struct Call : Layer { int dtype, M, N, K, template_id, num_sms; size_t workspace_bytes; Ovr ov; };

// ---- which kernels are built ---------------------------------------------------------------------------
// Each family's entry point for a call's layer (bit width, dtype, TileP) and the family's knobs, from the row lists of the
// instantiation units (kernels.h); nullptr: not built.  The only statement of which shapes exist: the planners ask these, and
// resolve_kernel stores the answer with the plan.
template <class Kernel> const void* fn_of(Kernel k) { return reinterpret_cast<const void*>(k); }
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

// ---- one-shot decode kernel (qgemm_oneshot.h): launch shape --------------------------------------------
// A workgroup of W = upw x kw waves owns upw units for the whole of K (no persistence, no grid K split): wave
// (ul, kpart) decodes pk <= D pieces of its unit.  Candidates: D pieces per wave x W in {4, 8, 16}, kw the
// smallest power of two that fits K into kw x D pieces.  Ranked by what tools/ubench/oneshot_lab measured on
// 4096^2 / 4096x11008 (profiles/r03_oneshot_lab.jsonl): launches that give every CU a workgroup first, then
// the smallest in-workgroup K split (kw = 1 needs no cross-wave reduction), then the smallest workgroup that
// keeps the launch at <= 3 workgroups per CU (every workgroup builds its own table image).
// Template knobs: Stages 2..5 -> rank 0..3; QuantMapMode digit (4-bit ids) 1 / 2 -> D = 4 / 8 only.
struct OneShape { int W, kw, upw, pk, depth, pipe, ipw, grid; size_t lds; };
struct OneArgs { int lg, lkw, upw, pk, ipw, depth, pipe, nvis, nch, nwg, nsets; };

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
double persistm_model_us(int M, int N, int K, int num_sms, int ng, int* grid_out, int* visits_out, int visits_ovr) {
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
                int rank = 0, double* cost_us = nullptr) {
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

// ---- the planner ------------------------------------------------------------------------------------------

// What every entry point checks of a layer - bits, group size (0: none, flute_unpack), template id, then N and K alignment -
// in the order of its error codes.  *l describes the layer that passes.
int check_layer(int bits, int group, int template_id, int N, int K, int k_align, Layer* l) {
    if (bits != 2 && bits != 3 && bits != 4) return FLUTE_ERR_NUM_BITS;
    if (group && group != 32 && group != 64 && group != 128 && group != 256) return FLUTE_ERR_GROUP_SIZE;
    if (!decode_template(bits, template_id, &l->t)) return FLUTE_ERR_TEMPLATE_ID;
    if (bits == 3 && l->t.tile_p != 32) return FLUTE_ERR_TEMPLATE_ID;   // utils.py:137-139
    l->bits = bits;
    l->J = (bits == 3) ? 16 : 16 / bits;
    l->lg = group ? ilog2(group) : 0;
    if (N < 1 || K < 1 || N % (l->J * l->t.tile_p) || K % k_align) return FLUTE_ERR_SHAPE;
    l->units = N / l->J;
    return FLUTE_OK;
}

// A plan, the launch arguments the decode kernels take beside it, and its kernel (resolve_kernel): fn_had is the member that rotates
// the activations while it stages them, where that is an instantiation of its own (one-shot and persistent one-shot kernels; else null).
struct Planned { flute_plan p; OneArgs oa; StreamArgs sa; const void* fn; const void* fn_had; };

int lds_fits(const flute_plan& p) { return p.lds_bytes > (size_t)kMaxLds ? FLUTE_ERR_SHAPE : FLUTE_OK; }
// workspace of a grid K split whose fp32 slabs are [splitk][M][N] behind the state words
size_t split_slabs(int splitk, int M, int N) { return splitk > 1 ? (size_t)splitk * M * N * 4 + kXwgFlagBytes : 0; }

// The per-wave kernel's overrides (m_tiles, waves, kw, splitk, slabs, m_block) by their largest value: < 0 none given at all,
// <= 0 none that asks for anything (0 reads as automatic in the per-wave planner)
int wave_ovr_max(const Ovr& o) { return std::max({o.m_tiles, o.waves, o.kw, o.splitk, o.slabs, o.m_block}); }
// ids whose last digit leaves the kernel choice to the planner: 4-bit QuantMapMode digit 0, every 2- / 3-bit id
bool auto_digit_sk(int bits, int template_id) { return bits != 4 || (template_id % 4) == 0; }
// ... and, for the 4-bit lean and MFMA decode kernels, SMs_Multiple 1 besides
bool auto_lean_id(const Call& c) { return c.bits == 4 && (c.template_id % 4) == 0 && c.t.sms_multiple == 1; }

// Every decode kernel reads the scales through one descriptor with 32-bit byte offsets (qgemm_stream.h:271,302, qgemm_oneshot.h:400,411,
// qgemm_persist.h:96,114, qgemm_fast.h:225): a layer whose scales reach that range takes the per-wave kernel (64-bit pointers), forced
// family 0 as well.
bool decode_fits(const Call& c) { return (size_t)c.N * (size_t)(c.K >> c.lg) * 2 < (size_t)0xfffffff0u; }

// Streaming decode kernel: M <= 2; its four-row variant (2- / 4-bit) only on request (override family 0, which
// flute_qgemm_hadamard sets for small layers so that the rotation stays fused): measured at M = 3, 4 the MFMA
// kernel is as fast on 4096^2 (7.6 vs 7.75 us) and 15-25 % faster on every larger layer (8192x28672: 38.6 vs 48.9).
// (3-bit layers up to 24 M weights also take it by themselves: their MFMA plans are 256 columns wide per wave -
// 4096^2 M = 4: 9.9 against 13.7 us; larger 3-bit layers are faster on the MFMA kernel.)
// round 4: 2- / 4-bit layers up to 16 M weights take the four-row one-shot kernel at M = 3, 4 too (4096^2 M = 4: 6.3 us
// against 7.1 on the MFMA kernel, profiles/r04_planner_regret_before_fixes.json - the one-shot kernel of round 3 was not
// there when the MFMA kernel was measured level with the ring kernel)
// (only ids whose last digit leaves the choice to the planner: a 4-bit id with QuantMapMode digit 3 keeps the skinny MFMA kernel it was
// tuned on - "a tuned id keeps the kernel it was timed on", tests/test_abi.py)
bool decode_auto(const Call& c) {
    if (!decode_fits(c)) return false;
    if (c.M <= 2) return true;
    if (c.M > 4) return false;
    const size_t weights = (size_t)c.N * c.K;
    if (c.bits == 3) return weights <= ((size_t)24 << 20);
    return weights <= ((size_t)16 << 20) && auto_digit_sk(c.bits, c.template_id);
}

// Persistent MFMA decode kernel (qgemm_persistm.h, round 6): by override (family 8), or automatically - under the ids that leave the choice
// to the planner, as the lean MFMA decode kernel - for 3 <= M <= 16 rows of a 4-bit layer with K >= 6144 (group size 64 / 128).  Measured (profiles/r06/call31_persistm_xr.log,
// us, table's plan -> this): M = 4: 8192 x 28672 [N x K] 34.6 -> 29.4, 10240 x 8192 20.6 -> 14.3, 4096 x 11008 14.7 -> 9.2, 3584 x 14336 14.6 -> 10.0,
// 4096 x 14336 14.7 -> 10.5, 8192^2 12.9 -> 11.7, 28672 x 8192 33.0 -> 31.1; M = 16: 10240 x 8192 22.2 -> 17.4, 4096 x 11008 14.9 -> 11.9,
// 8192^2 15.8 -> 13.9; not taken: K = 4096 (14336 x 4096: 11.1 against 11.5 .. 12.4; the lean MFMA decode kernel's and the skinny kernel's
// layers)
// (second sweep, profiles/r06/planner_regret_persistm*.json: also K >= 3584 at M <= 4 - 14336 x 3584 13.2 -> 10.3, 11008 x 4096 11.1 -> 9.6,
// 6144 x 4096 8.3 -> 7.6 - and at every M <= 16 where K is neither 2048 nor 4096, the lean MFMA decode / skinny kernels' depths -
// 14336 x 3584 M = 8 13.2 -> 11.9; and no limit on the activations at M > 8: equal at M = 16 on the 28672-wide / -deep layers, 7 - 15 % faster at M = 11)
// (third step, profiles/r06/call37_persistm_resident_activations.log: with the activations RESIDENT in LDS - K * ceil(M / 4) rows within 64 KB - also
// K = 4096 at M <= 8: 4096^2 M = 8 5.9 -> 5.5, 11008 x 4096 10.9 -> 9.3, 14336 x 4096 11.4 -> 11.3)
// 2-bit member (profiles/r06/call38_persistm_2bit.log, us, table's plan -> this): every 2-bit id leaves the choice to the planner and no lean kernel
// competes - from K = 3584 and 16 M weights at every 3 <= M <= 16: 4096^2 M = 4 / 16 8.4 / 8.6 -> 5.0 / 6.1, 4096 x 11008 14.1 -> 8.1, 10240 x 8192 18.3 -> 13.8,
// 8192 x 28672 30.7 -> 25.8; above M = 8 not where the busiest workgroup pulls more than 28672 k of sixteen-row activations (28672 x 8192: 33.4 against 31.5)
bool persistm_auto(const Call& c) {
    const int M = c.M, N = c.N, K = c.K;
    const bool pm_k = K >= 6144 || (K >= 3584 && (M <= 8 || (K != 4096 && K != 2048)));
    const bool pm4 = auto_lean_id(c) && pm_k && (size_t)N * K + (M >= 5 ? 1 : 0) > ((size_t)16 << 20);
    const bool pm2 = c.bits == 2 && K >= 3584 && (size_t)N * K >= ((size_t)16 << 20);
    return (pm4 || pm2) && M >= 3 && M <= 16 && (c.lg == 6 || c.lg == 7) &&
           (long)(N / 16) * 2 >= (long)c.num_sms &&      // (smaller layers: the decode kernels / too few sets for the chip; 4-bit 4096^2 itself from M = 5)
           wave_ovr_max(c.ov) < 0 && c.ov.one_shot < 0 && c.ov.depth <= 0;
}
bool persistm_taken(const Call& c, const flute_plan& p) { return c.bits == 4 || c.M <= 8 || (long)p.visits * c.K <= 28672; }

// Lean MFMA decode kernel (qgemm_fastm.h, round 5): by override (family 7), or automatically for 5 <= M <= 16 rows of a 4-bit layer
// with K = 2048 / 4096 that ONE round of its workgroups (4 unit rows each) covers, under the ids whose last digit leaves the
// choice to the planner (QuantMapMode digit 0, SMs_Multiple 1).  Measured (tools/time_cases.py, us, automatic plan of round 4 ->
// this kernel; profiles/r05/time_cases_fastm*.jsonl): 4096^2 M = 5 / 8 / 16 7.13 / 7.13 / 7.18 -> 5.9 / 5.9 / 6.1, 4096 x 2048
// 5.7 / 5.7 / 5.8 -> 4.3 / 4.3 / 4.5, 2048 x 4096 7.6 / 7.6 / 7.7 -> 5.4 / 5.4 / 5.6; not taken: more than one round (8192 x 4096:
// 10.2 .. 10.8 against the skinny kernel's 8.9 .. 9.6: every workgroup pulls all of X through its CU), M <= 4 (the dot-product
// lean kernel: 5.05 against 5.9)
// Round 6: two / three column groups per workgroup on ONE staged activation set make wider layers one round of workgroups
// (profiles/r06/call18_fastm_column_groups.log, M = 16, us, table's plan -> this): 8192 x 4096 10.1 -> 8.9 (2 groups, 256 workgroups),
// 11008 12.6 -> 11.4 (3 groups, 230), 6144 9.4 -> 8.4, 5120 9.2 -> 8.0, 8192 x 2048 6.9 -> 6.2; M = 8 on 11008 11.6 -> 11.0; not taken:
// more than one round even at three groups (14336: 16.0 against 13.1; 28672: 30 against 23)
bool fastm_auto(const Call& c) {
    const long groups = c.N / 16, ns = c.num_sms;
    const long wgs = groups <= ns ? groups : (groups <= 2 * ns ? (groups + 1) / 2 : (groups + 2) / 3);
    return auto_lean_id(c) && c.M >= 5 && c.M <= 16 && (c.K == 4096 || c.K == 2048) && wgs <= ns && wgs * 2 >= ns &&
           wave_ovr_max(c.ov) < 0;
}

// Skinny MFMA kernel (qgemm_skinny.h): by override (family 5), by template (4-bit QuantMapMode digit 3 at M <= 16, where
// the digit's other meaning - two slabs per wave - does not exist; digit 2: never), or automatically (digit 0) for
// 3 <= M <= 16 on layers whose slabs (64 columns) fill 55 .. 100 % of the CUs in ONE round - a workgroup pulls its slab's
// weights AND all of X through one CU, so fewer slabs leave CUs idle; wider layers take the per-wave kernel with two
// slabs per wave (4096 x 28672: 21.1 us against 23.3 here).  Measured (profiles/r03/skinny_lab.jsonl, M = 16, us, per-wave kernel -> skinny):
// 4096 x 11008 17.9 -> 12.0, 4096 x 14336 18.3 -> 12.6 (M = 4: 17.6 -> 11.8), 4096 x 28672 26.6 -> 23.3, 4096 x 6144
// 13.1 -> 11.7, 2048 x 8192 7.6 -> 7.0; 4096 x 8192 10.0 -> 11.8 and 4096^2 7.6 -> 11.6 (not taken).
bool skinny_auto(const Call& c) {
    const long slabs = c.units / 16;
    const bool fills = slabs * 20 >= 11L * c.num_sms && slabs <= c.num_sms;
    const int q4 = c.template_id % 4;
    return c.bits == 4 && c.M >= 3 && c.M <= 16 && ((q4 == 0 && c.K >= 4096 && fills) || q4 == 3);
}
// Round 4: narrower layers through a grid-level K split (the slices of a slab meet inside the launch, xwg.h: 1.5 - 1.7 us
// of seam, profiles/r04/xwg_seam_price.json) - the smallest power-of-two split that fills 55 % of the CUs, while a
// slice keeps >= 2048 k.  Measured (profiles/r04_planner_regret_before_fixes.json, us, per-wave kernel -> split skinny):
// M = 4: 3584 x 8192 10.1 -> 8.7, 8192^2 14.6 -> 13.0, 6144 x 4096 9.2 -> 8.5; M = 16: 3584 x 8192 10.2 -> 9.6; not
// taken: 4096^2 (four slices of 1024 k: 7.6 against 7.2).  Returns the split, 0: none.
int skinny_split_auto(const Call& c) {
    const long slabs = c.units / 16;
    const int q4 = c.template_id % 4;
    if (c.ov.splitk >= 0 || c.bits != 4 || c.M < 3 || c.M > 16 || (q4 != 0 && q4 != 3) || c.K < 4096 || slabs * 20 >= 11L * c.num_sms)
        return 0;
    int sk = 2;
    while (sk < 16 && slabs * sk * 20 < 11L * c.num_sms) sk *= 2;
    return (slabs * sk <= c.num_sms && c.K / sk >= 2048) ? sk : 0;
}

// Split-K block kernel (qgemm_splitk.h): by override (family 6); by template - Stages 5 of the automatic digit at
// M >= 128 (SMs_Multiple 1 / 2 / 4: the cost model's best / second / third K split; those ids' old meaning, a quarter of
// the per-wave kernel's in-workgroup K split, is still reachable through digits 1 .. 3); automatically below, when
// its modelled time beats what the other MFMA kernels are modelled at
// (round 4, late: 4-bit layers from M = 33, 2-bit layers from M = 65 - 64-row tiles x K slices against the per-wave kernel:
// M = 64 x 8192^2 24.7 -> 20.0 us, M = 33 23.7 -> 19.5, M = 96 x 14336 x 4096 41.2 -> 24.6, M = 96 x 8192^2 45.3 -> 28.6;
// 2 bits M = 96: 8192^2 43.3 -> 29.0, 14336 x 4096 40.5 -> 25.4; 2 bits at M = 64 gain 3 .. 9 % only: left alone)
// (2 bits: from M = 65 until round 6 - with 64 x 64 tiles M = 48 / 64 gain 25 - 43 %: profiles/r06/planner_regret_before_fixes.json)
// (overrides of the per-wave kernel - m_tiles, waves, kw, splitk, slabs - mean something else in plan_splitk: a call that sets
// any of them without family = 6 keeps the per-wave / block kernels)
bool splitk_regime(const Call& c) {
    return wave_ovr_max(c.ov) <= 0 && c.bits != 3 && c.M >= 33 && auto_digit_sk(c.bits, c.template_id);
}
// (M <= 64: the table's Stages-5 ids of that bucket were tuned on the per-wave kernel's K split)
bool splitk_stages5(const Call& c) { return splitk_regime(c) && c.t.stages == 5 && c.M > 64; }

// Per-wave MFMA kernel (family 2), 2 / 4 bits: TFLOP/s by batch size (what the block and split-K kernels are priced against)
double wave_tflops(const Call& c) {
    const int M = c.M;
    const bool bf = c.dtype == FLUTE_BF16;
    // (2-bit layers: twice the lookups per byte - the per-wave kernel ran M = 384 on 4096^2 at 316 TFLOP/s where the 4-bit layer runs 503:
    // profiles/r06_planner_regret_between_final.json)
    // (the 2-bit factor holds below M = 128 too - it was once applied above that branch only: 2-bit M = 48 on 4096^2 kept the per-wave kernel
    // x 4 K slices, 15.0 us, where 64 x 64 tiles x 4 slices run 11.1: profiles/r06_planner_regret_final_tree_between.json)
    const double b2 = c.bits == 2 ? 0.65 : 1.0;
    // below M = 128 (measured fp16, tools/time_cases.py): 220 .. 280 TFLOP/s at M = 48, 270 .. 350 at M = 64 .. 96 on layers up to
    // 14336 columns; 490 .. 570 on 28672 columns (two slabs per wave, every CU busy)
    if (M < 128) return std::min(300.0, 5.5 * M) * (bf ? 0.8 : 1.0) * (c.N >= 16384 ? 1.8 : 1.0) * b2;
    // 128 <= M < 512 (end of round 6, profiles/r06/planner_regret_bits_4_2_m128_to_512_end_of_round.json: measured 295 / 345 at M = 160 / 192
    // on 11008 x 4096, 426 / 493 at M = 320 / 384 on 4096^2 - the "520 at M = 256, 465 below" it replaces kept the per-wave kernel at M = 160 /
    // 192 / 320 on 11008 x 4096, 14336 x 4096, 14336 x 3584, 3584 x 14336, 3584 x 8192 where split-K tiles run 30 - 70 % faster)
    if (M < 512) return (300.0 + 0.75 * (M - 128)) * (bf ? 0.8 : 1.0) * b2;
    // from M = 512: 520 (bf16 400) TFLOP/s at M = 256, + 55 per doubling of M, up to 730 (560)
    int dbl = 0;
    for (int m = M; m >= 512; m >>= 1) ++dbl;
    return (bf ? std::min(560.0, 400.0 + 55.0 * dbl) : std::min(730.0, 520.0 + 55.0 * dbl)) * b2;
}
double flop_us(const Call& c, double tflops) { return 2.0 * c.M * (double)c.N * c.K / (tflops * 1e6); }

// Block-tiled prefill kernels (qgemm_block2.h: 256 x 256 or 128 x 256 blocks, a wave owns all rows and 32
// columns, 4- and 2-bit layers; qgemm_block3.h: the same for 3 bits, 128-row blocks); scale rows in
// whole 16-B granules.  No K split for 2 / 4 bits (qgemm_splitk.h serves that regime; 3 bits: priced below), so what decides is
// how many blocks the output has.  Cost model fitted to tools/block_lab.py (MI355X, K = 4096; us per block,
// running alone / with the whole chip busy - the chip clocks down under a full MFMA load):
//   256-row block fp16 100 / 126, bf16 104 / 129;  128-row block fp16 72 / 81, bf16 80 / 89 (round 2);
//   round 4 (2- / 4-bit blocks: whole-line activation pieces, one whole-line weight request per step):
//   256-row 97 / 120, bf16 101 / 124;  128-row 62 / 74, bf16 70 / 78 (profiles/r04/splitk_lab_run7*.jsonl);
//   per-wave MFMA kernel (family 2): wave_tflops.
// The choice: block configuration (flute_plan::m_block of family 3, -1: none), the grid K split the cost model chose with it
// (3 bits, 0: none), and the modelled time of the best other MFMA kernel (-1: not priced).
struct BlockChoice { int cfg, sk; double alt_us; };
BlockChoice choose_block(const Call& c) {
    const int bits = c.bits, M = c.M, N = c.N, K = c.K, lg = c.lg, units = c.units, num_sms = c.num_sms;
    const Ovr& ov = c.ov;
    BlockChoice b{-1, 0, -1.0};
    const int blk_units = 256 / c.J;                  // units of a 256-column block (4-bit: 64, 2-bit: 32, 3-bit: 16)
    const bool b3_ok = bits != 3 || (size_t)3 * (N >> 4) * K * 2 < (size_t)0xfffffff0u;   // one descriptor over Q
    const bool x32_ok = (size_t)(M + 256) * K * 2 < (size_t)0xfffffff0u;       // activation byte offsets are 32-bit voffsets
    const bool s32_ok = (size_t)N * (K >> lg) * 2 < (size_t)0xfffffff0u;       // ... and so are the scale offsets (one descriptor over S)
    if (!b3_ok || !x32_ok || !s32_ok || (K >> lg) % 8 || units % blk_units) return b;
    const long tiles256 = (long)ceil_div(M, 256) * (units / blk_units), tiles128 = (long)ceil_div(M, 128) * (units / blk_units);
    if (ov.family == kFamilyBlock) {
        b.cfg = (ov.m_tiles == 4) ? 5 : 4;               // 128- / 256-row blocks of qgemm_block2.h
        if (bits == 3 && ov.m_tiles != 8) b.cfg = 5;     // 3-bit layers: 128-row blocks of qgemm_block3.h unless 256 rows are asked for ...
        if (bits == 3 && ov.m_block > 0 && block_fn(c, 8 + ov.m_block))
            b.cfg = 8 + ov.m_block;                      // ... or its skinny blocks of m_block row tiles (1, 2, 4)
    } else if (bits == 3 && M > 32 && M <= 64 && (size_t)N * K >= ((size_t)56 << 20) &&
               (M > 48 || skinny3_fills(M, units / blk_units, K, lg, num_sms))) {    // (14336 x 3584, 51 M weights: 29.5 against 26.4 us on the per-wave kernel)
        // 3-bit skinny blocks (64 rows, grid K split): measured against the per-wave kernel at M = 64 - 8192^2 31.6 vs
        // 38.5 us, 28672x8192 86.9 vs 105.7, 4096x14336 31.8 vs 35.4; slower below M = 33 and on 4096^2 (fixed
        // costs of ~8 us per call: prologue, fp32 slabs, reduce launch)
        b.cfg = 12;
    } else if (M >= 256 || (bits == 3 && M > 64) || (bits != 3 && M > 128)) {          // (3 bits from M = 65: the K-split candidates below; 2 / 4 bits from M = 129: 128-row blocks on the
        // widest layers - 2-bit 28672 x 8192 at M = 192 ran 210 us on the per-wave kernel, 125 on 128-row blocks, profiles/r06/planner_regret_bits_4_2_m96_to_768_unswept_batch_sizes.json)
        const bool bf = c.dtype == FLUTE_BF16;
        auto block_us = [&](long tiles, double alone, double busy) {
            const long whole = tiles / num_sms, rest = tiles % num_sms;       // full rounds + a last partial one
            const double last = rest == 0 ? 0.0 : (rest * 4 >= (long)num_sms * 3 ? busy : alone);
            return ((double)whole * busy + last) * (double)K / 4096.0 + 3.0;
        };
        // 3-bit layers (qgemm_block3.h): 128-row blocks 78 / 85 us alone, 85 / 90 busy; 256-row blocks (round 3) 108 / 118
        // alone, 124 / 128 busy (profiles/r03/block_lab_w3_256_row_blocks.jsonl); the per-wave kernel runs them at
        // 330-380 TFLOP/s
        const double t256 = (bits == 3) ? block_us(tiles256, bf ? 118.0 : 108.0, bf ? 128.0 : 124.0)
                                        : block_us(tiles256, bf ? 101.0 : 97.0, bf ? 124.0 : 120.0);
        const double t128 = (bits == 3) ? block_us(tiles128, bf ? 85.0 : 78.0, bf ? 90.0 : 85.0)
                                        : block_us(tiles128, bf ? 70.0 : 62.0, bf ? 78.0 : 74.0);
        // (3 bits, round 4: 14336 x 3584 M = 256 runs at 305, modelled 370 kept it off the 128-row blocks: 86.4 against 70.3 us; round 5's
        // regret sweep, fp16: 3584 x 8192 M = 256 293, 14336 x 3584 M = 128 276, 8192^2 M = 96 253 - fewer rows, fewer MFMAs per lookup)
        const double wave_tf = (bits == 3) ? (bf ? 290.0 : 300.0) * (M >= 256 ? 1.0 : 0.6 + 0.4 * M / 256.0) : wave_tflops(c);
        const double wave_us = flop_us(c, wave_tf);
        if (t256 <= t128 && t256 < wave_us) b.cfg = 4;
        else if (t128 < t256 && t128 < wave_us) b.cfg = 5;
        b.alt_us = std::min(wave_us, std::min(t256, t128));
        if (bits == 3) {
            // 3-bit layers have no split-K block kernel of their own (qgemm_splitk.h: 2 / 4 bits): where whole blocks leave
            // CUs idle, 128- or 64-row blocks of qgemm_block3.h with a grid K split (fp32 slabs + the reduce pass) fill
            // them.  One round of workgroups; a block costs ~4 us + its K share of (128 rows: 78 / 85 us alone, 85 / 90 busy;
            // 64 rows: 66 / 72 - the lookups of a block's 256 columns dominate, the rows are nearly free), the slabs 0.25 us
            // per MB + the reduce launch.  Measured (bf16, profiles/r04/w3_mid_m_forced_plans.jsonl; before -> after):
            // M = 1024 x 4096^2 84.9 -> 56.4 us, M = 512 x 8192^2 160.5 -> 95.6, M = 512 x 4096^2 54.5 -> 45.4
            const double base = b.cfg == 4 ? t256 : (b.cfg == 5 ? t128 : wave_us);
            double best = 0.95 * base;                      // a K-split plan has to beat the unsplit best by 5 %; among themselves: the cheapest
            const int align_k = std::max(64, 8 << lg);
            for (int rows = 128; rows >= 64; rows >>= 1) {
                const long tiles = (long)ceil_div(M, rows) * (units / blk_units);
                const double alone = rows == 128 ? (bf ? 85.0 : 78.0) : (bf ? 72.0 : 66.0);
                const double busy = rows == 128 ? (bf ? 90.0 : 85.0) : (bf ? 72.0 : 70.0);
                for (int sk = (rows == 128 ? 2 : 1); sk <= 4; sk *= 2) {
                    const long wgs = tiles * sk;
                    // slices of kps k, the last one shorter where K is no multiple (K = 3584: 2048 + 1536, or 3 x 1024 + 512 - round 5:
                    // 14336 x 3584 M = 128 47.6 -> 33.9 us, M = 256 61.7 -> 49.3; until then only equal slices were priced)
                    const int kps = round_up(ceil_div(K, sk), align_k);
                    if (sk > 1 && (wgs > (long)num_sms || ceil_div(K, kps) != sk || kps < 1024 ||
                                   (size_t)sk * tiles * rows * 1024 > slab_room(c.workspace_bytes))) continue;
                    double us;
                    if (sk == 1) us = block_us(tiles, alone, busy);
                    else us = 4.0 + ((wgs * 4 >= (long)num_sms * 3 ? busy : alone) - 4.0) * (double)kps / 4096.0 +
                              (rows == 128 ? 2.0 : 5.0) +              // (128-row blocks: combined in the launch, round 5; else the reduce launch)
                              0.25 * (double)sk * M * N * 4.0 / 1e6;
                    if (us < best) { best = us; b.cfg = rows == 128 ? 5 : 12; b.sk = sk; }
                }
            }
            b.alt_us = std::min(b.alt_us, b.sk > 0 ? best : base);
        }
    }
    if (b.cfg >= 0 && !block_fn(c, b.cfg)) b.cfg = -1;     // a configuration that is not built is no choice
    return b;
}

// Split-K block kernel, automatic (the template's default Stages and SMs_Multiple): taken when its modelled time is
// 8 % under the best of the per-wave kernel and the block kernels (alt_us; the per-wave kernel alone where the block cost model did not run).
// Measured (tools/splitk_lab.py, us, automatic plan of round 3 -> this kernel): M = 256 x 4096 x 11008 44.5 -> 38.1,
// 4096 x 14336 47.2 -> 40.2, 8192^2 49.0 -> 44.2; M = 1024 x 4096^2 49.6 -> 41.8 (torch.mm 46.9), M = 512 29.0 -> 27.4;
// not taken: M = 256 x 4096^2 (24.9 against 20.1: the seam of four slices), M = 128 x 4096^2, K = 14336.
bool splitk_auto(const Call& c) { return splitk_regime(c) && c.t.stages == 2 && c.t.sms_multiple == 1; }
bool splitk_auto_taken(const Call& c, const flute_plan& q, double sk_us, double alt_us) {
    // (one round of workgroups only: multi-round launches are left to the tuner's Stages-5 ids until measured)
    // (round 6: 64 x 64 tiles - four K parts per workgroup - that fill at least half the chip are priced against the per-wave kernel
    // WITH its fixed part, which the TFLOP/s model lacks: measured - modelled 3.2 .. 5.7 us on 4096-wide layers, 10 on
    // 2048 x 8192; profiles/r06/call17_automatic_plan_vs_forced.log: M = 128 on 4096^2 13.1 against 14.9 us, M = 192 15.1 / 18.8, M = 512 on
    // 2048 x 4096 15.8 / 19.9, M = 256 on 2048 x 8192 18.0 / 26.6, M = 48 on 3584 x 14336 16.7 / 21.6, M = 33 on 8192^2 17.7 / 26.1)
    // (2-bit layers up to M = 64: also two rounds - 28672 x 8192 M = 33 / 48 / 64: 448 workgroups of 64 x 128 tiles x 2 slices 46.6 / 47.8 / 49.3 us
    // against the per-wave kernel's 61.3 / 61.5 / 62.3, profiles/r06/planner_regret_b2_m33_96_after_2bit_rate_fix.json)
    return sk_us < ((q.kw == 4 && (long)q.grid * 2 >= (long)c.num_sms) ? alt_us + 4.0 : 0.92 * alt_us) &&
           (long)q.grid <= (c.bits == 2 && c.M <= 64 ? 2L : 1L) * (long)c.num_sms && q.lds_bytes <= (size_t)kMaxLds;
}

// Decode kernels (family 0).  Three of them: the one-shot kernel (qgemm_oneshot.h: non-persistent workgroups, every request up
// front) and the persistent ring kernel (qgemm_stream.h).  Forced by override (one_shot 1 / 0; an explicit
// ring depth or grid K split means the ring kernel) or by the template (4-bit QuantMapMode digit 1, 2:
// one-shot with 4 / 8 pieces per wave, 3: ring; 2- / 3-bit SMs_Multiple 4: one-shot, 2: ring); automatic:
// one-shot for layers up to 64 M weights that give at least half the CUs a workgroup; one or two rows on larger layers:
// the persistent one-shot kernel (qgemm_persist.h; override one_shot = 3, as flute_plan reports it, or 2).
// Tried in order: lean one-row kernel -> persistent one-shot -> one-shot -> ring.
int plan_decode(const Call& c, Planned* out) {
    const int bits = c.bits, lg = c.lg, M = c.M, N = c.N, K = c.K, num_sms = c.num_sms, template_id = c.template_id;
    const flute_template_info& t = c.t;
    const Ovr& ov = c.ov;
    // a fused Hadamard rotation prefers 8-wave workgroups (4096x3584 M = 1: 5.5 us with 8 waves, 6.5 with
    // the 4-wave shape the plain product takes)
    Ovr ovd = ov;
    if (ov.had8 && ovd.waves < 0 && ovd.kw < 0 && ovd.one_shot != 0) ovd.waves = 8;
    int want = ov.one_shot == 3 ? 2 : ov.one_shot;       // 3 = flute_plan's code for the persistent kernel (2 kept from ABI v4)
    if (want < 0 && (ov.depth > 0 || ov.splitk > 1)) want = 0;
    if (want < 0 && bits == 4) { const int q = template_id % 4; want = (q == 3) ? 0 : ((q == 1 || q == 2) ? 1 : -1); }
    if (want < 0 && bits != 4) want = (t.sms_multiple == 2) ? 0 : (t.sms_multiple == 4 ? 1 : -1);
    // lean one-row kernel (qgemm_fast.h): by override (one_shot = 4), or automatically for the ids whose last digit leaves the choice
    // to the planner and whose Stages digit asks for the planner's first or second shape (4-bit QuantMapMode digit 0, Stages 2 / 3,
    // SMs_Multiple 1: ids 0 / 4 - TileP 64 - and 16 / 20 - TileP 32), on K = 2048 / 4096 layers up to 48 M weights that give at
    // least half the CUs a workgroup - measured against the persistent and the round-4 one-shot kernel (us, persistent / lean /
    // one-shot): 4096^2 4.42 / 4.05 / 4.14, 5120 4.96 / 4.90 / 5.88, 8192 5.51 / 5.46 / 5.91, 11008 7.54 / 6.86 / 8.04; not taken:
    // 14336 7.85 / 8.27 / 8.43, 28672 13.6 / 13.9 / 14.6, more than three workgroups per CU (16384 x 2048: 5.97 against 5.49 on the
    // one-shot kernel; 8192 x 2048 3.77 / 4.05 is taken), K = 8192 (8192^2 8.42 against 10.42, 4096 x 8192 5.71 / 5.97: by
    // override only).  Two to four rows (dot products per row on the same lookups): while ONE round of workgroups covers the layer
    // (4096^2: M = 2 5.04 -> 4.29 us, M = 3, 4 6.25 -> 5.03; 4096 x 2048: 3.87 -> 3.25, 4.65 -> 3.71; beyond, the persistent kernel
    // (M = 2) and the skinny MFMA kernel (M = 3, 4) win: 8192 x 4096 5.79 against 7.12, 8.69 against 8.98).  Never for a call that
    // fuses the Hadamard rotation.  K = 8192 (shape (8, 2, 8)), round 5's last call series: one row a tie with the one-shot kernel
    // (3584 x 8192: 5.33 / 5.40 us, 4096 x 8192: 5.57 / 5.51), TWO rows on layers that give >= 80 % of the CUs a workgroup 6.11 against
    // 6.78 and 6.33 against 6.82 - taken; narrower layers (2048, 1024 columns: 128 / 64 workgroups) lose 13 - 17 % and are not.
    // K = 2048, two rows: up to two rounds (6144 x 2048 4.34 -> 3.79 us, 8192 x 2048 4.38 -> 4.01; four rows lose there: 5.14 / 5.76)
    if ((want == 4 || (want < 0 && auto_lean_id(c) && t.stages <= 3 && ov.waves < 0)) && !ov.had8 && ov.kw < 0) {
        Planned q{};
        if (plan_fast(c, std::max(0, t.stages - 2), want == 4 ? ov.waves : -1, &q.p, &q.oa) == FLUTE_OK &&
            (want == 4 || ((K != 8192 || (M == 2 && (long)q.p.grid * 5 >= (long)num_sms * 4)) &&
                           (size_t)N * K <= ((size_t)48 << 20) && (long)q.p.grid * 2 >= (long)num_sms &&
                           (long)q.p.grid <= (M == 1 ? 3L : (M == 2 && K == 2048 ? 2L : 1L)) * num_sms))) {
            *out = q;
            return lds_fits(out->p);
        }
    }
    if (want == 4) want = -1;
    // persistent one-shot kernel: by override, or automatically (one or two rows; four rows measured 1.7x the one-row
    // time - no faster than the MFMA kernel, profiles/r03/decode_lab_persist_rows.jsonl) on layers of >= 40 M weights that give
    // every CU six whole unit rows (below that the in-workgroup K split of the other two kernels wins:
    // profiles/r03/persist_lab.txt; round 4: from 40 M weights / 6 unit rows per CU - 6144 x 4096 M = 2 6.8 -> 6.0 us, 2-bit
    // 10240 x 8192 M = 1 10.8 -> 9.8)
    const bool auto_digit = (bits == 4) ? (template_id % 4) == 0 : t.sms_multiple == 1;
    const bool persist_auto = want < 0 && ov.one_shot < 0 && ov.depth <= 0 && ov.splitk <= 1 && auto_digit &&
                              (size_t)N * K >= ((size_t)24 << 20) && (long)c.units >= 4L * num_sms;
    if (want == 2 || persist_auto) {
        Planned q{};
        if (plan_persist(c, ovd, &q.p, &q.oa) == FLUTE_OK) { *out = q; return lds_fits(out->p); }
        if (want == 2) want = 0;
    }
    if (want != 0) {
        Planned q{};
        if (plan_oneshot(c, ovd, &q.p, &q.oa) == FLUTE_OK &&
            (want == 1 || ((size_t)N * K <= ((size_t)64 << 20) && (long)q.p.grid * 2 >= (long)num_sms))) {
            *out = q;
            return lds_fits(out->p);
        }
    }
    Planned q{};
    const int rc = plan_stream(c.dtype, bits, lg, M, N, K, num_sms, t, ovd, slab_room(c.workspace_bytes), &q.p, &q.sa);
    if (rc) return rc;
    q.p.workspace_needed = split_slabs(q.p.splitk, M, N);
    *out = q;
    return lds_fits(out->p);
}

// Block kernels (family 3) in configuration b.cfg, K split b.sk (0: the planner's own).
int plan_block(const Call& c, const BlockChoice& b, Planned* out) {
    const int bits = c.bits, M = c.M, N = c.N, K = c.K, lg = c.lg;
    const Ovr& ov = c.ov;
    const int bm = block_rows(b.cfg), tm = bm / 32;
    const int tiles_m = ceil_div(M, bm), tiles_n = c.units / (256 / c.J);
    const int align_k = std::max(64, 8 << lg);
    int splitk = (ov.splitk > 0) ? ov.splitk : (b.sk > 0 ? b.sk : 1);
    if (b.cfg >= 8 && ov.splitk <= 0 && b.sk == 0)   // skinny blocks: the K split fills the chip
        while ((long)tiles_m * tiles_n * splitk * 2 <= (long)c.num_sms && K / (splitk * 2) >= std::max(256, align_k)) splitk *= 2;
    int kps = round_up(ceil_div(K, splitk), align_k);
    splitk = ceil_div(K, kps);
    while (splitk > 1 && (size_t)splitk * M * N * 4 > slab_room(c.workspace_bytes)) {
        splitk >>= 1;
        kps = round_up(ceil_div(K, splitk), align_k);
        splitk = ceil_div(K, kps);
    }
    if (splitk == 1) kps = K;
    Planned q{};
    flute_plan& p = q.p;
    p.family = kFamilyBlock;
    p.m_block = b.cfg; p.m_tiles = tm; p.slabs_per_wave = 1; p.waves = 8; p.kw = 1;
    p.splitk = splitk; p.k_per_split = kps;
    p.grid = (unsigned)((long)tiles_m * tiles_n * splitk);
    p.block = 512;
    p.workspace_needed = split_slabs(splitk, M, N);
    // 3-bit 128-row blocks x 2 / 4 K slices (round 5): the slices of a block meet inside the launch (xwg.h, E form; slabs in
    // fragment order, whole blocks: tiles x 128 x 256 x 4 B per slice) - no reduce launch.  Measured against the reduce launch
    // (bf16, us, profiles/r05/call24_w3_inlaunch_and_line_planes.log): M = 1024 x 4096^2 56.3 -> 53.0 (fp16 53.4 -> 50.1),
    // M = 256 x 8192^2 56.0 -> 54.4, M = 512 x 8192^2 95.3 -> 92.7, M = 96 x 28672 x 8192 92.1 -> 89.0, M = 512 x 4096^2 a tie; NOT for
    // the skinny blocks (64 rows x 4 slices 46.7 -> 47.8; 8 slices, L form - the last arriver reads seven partials - 30.5 -> 32.6)
    if (bits == 3 && (splitk == 2 || splitk == 4) && bm == 128 && (long)tiles_m * tiles_n <= (long)kXwgMaxTiles) {
        const size_t slabs = (size_t)splitk * tiles_m * tiles_n * bm * 1024;
        if (slabs <= slab_room(c.workspace_bytes) && slabs < ((size_t)1 << 31)) { p.splitk_mode = 1; p.workspace_needed = slabs + kXwgFlagBytes; }
    }
    // pair table + three activation stages + per wave: two scale blocks and a sink
    // (3-bit 256-row blocks: + 18 KB, the second / third plane pieces of waves 6 and 7)
    p.lds_bytes = (size_t)((128 << (2 * bits)) + 3 * (bm / 16) * 2 * 1024 + 8 * 3 * 1024 + ((bits == 3 && bm == 256) ? 18 * 1024 : 0));
    p.lut_copies = 32;
    *out = q;
    return lds_fits(out->p);
}

// Per-wave MFMA kernel (qgemm_tile.h; families 1 / 2).  MT 16-row tiles per wave (1 for M <= 16),
// R lanes share a unit: pick the smallest R whose slab x row-tile count fills the chip; the
// rest of the parallelism is the in-workgroup K split, a grid-level split only for very
// narrow layers.
int plan_tile(const Call& c, Planned* out) {
    const int bits = c.bits, M = c.M, N = c.N, K = c.K, units = c.units, num_sms = c.num_sms, template_id = c.template_id;
    const flute_template_info& t = c.t;
    const Ovr& ov = c.ov;
    int mt = (M <= 16) ? 1 : (M <= 32 ? 2 : 4);
    const int mt_cap = (bits == 3) ? 2 : 4;
    if (mt > mt_cap) mt = mt_cap;
    if (t.tile_m / 16 < mt && M > 16) mt = t.tile_m / 16 >= 2 ? t.tile_m / 16 : mt;
    // SMs_Multiple = "more, smaller workgroups": halves / quarters the row tiles per wave (and,
    // below, raises the slab count the choice of R aims for)
    for (int m2 = t.sms_multiple; m2 > 1 && mt > 1; m2 >>= 1) mt >>= 1;
    if (ov.m_tiles == 1 || ov.m_tiles == 2 || ov.m_tiles == 4) mt = ov.m_tiles;
    if (mt > mt_cap) mt = mt_cap;
    // built (R, MT), one slab per wave (inst_tile_b*.hip: (J/R)*MT <= 16 accumulator tiles)
    auto combo_ok = [&](int r, int m) { return tile_fn(c, r, m, 1) != nullptr; };
    while (mt > 1 && !combo_ok(1, mt) && !combo_ok(2, mt)) mt >>= 1;
    const int mtiles = ceil_div(M, mt * 16);
    int R = 1;
    while (!combo_ok(R, mt)) R *= 2;
    // Every workgroup pulls its rows of X through one CU, so lane sharing (R-fold more, narrower slabs) multiplies the
    // activation traffic: it pays only while the workgroups leave more than ~45 % of the CUs idle (round 3,
    // profiles/r03/tile_lab_sw2_m16.jsonl, tile_lab_sw2_m32_m128.jsonl: 10240 x 8192 M = 16, 160 slabs: R = 1 22.2 us,
    // R = 2 26.8; M = 64: 36.7 / 49.9; 4096 x 11008 M = 64: 21.4 / 29.1; but 8192^2 M = 32, 128 slabs: R = 2 16.2, R = 1 19.3)
    auto fills = [&](long wgs) { return wgs * 20 >= 11L * num_sms * t.sms_multiple; };
    // ... and not at all where the grid K split can fill the chip instead (round 5's regret sweep, the in-launch seam of xwg.h being
    // cheap now): deep layers - K >= 10240: two slices, K >= 12288: four - stop sharing lanes as soon as that split fills.
    // 4096 x 11008 (N x K) M = 4: four lanes per unit 16.6 us, two lanes x 2 slices 14.8 (2 bits: 14.2 -> 12.5), M = 16 16.9 -> 15.4;
    // 3584 x 14336 M = 48: two lanes x 2 slices 26.4, no sharing x 4 slices 21.6 (profiles/r05_planner_regret_*.json)
    const long deep_split = (bits != 3 && (bits != 4 || (template_id % 4) == 0) && ov.splitk < 0) ? (K >= 12288 ? 4 : (K >= 10240 ? 2 : 1)) : 1;
    while (combo_ok(R * 2, mt) && !fills((long)units * R / 16 * mtiles) &&
           !(deep_split > 1 && fills((long)units * R / 16 * mtiles * deep_split))) R *= 2;
    // QuantMapMode digit 1 (4-bit ids): no lane sharing above M = 16 - the chip is filled by the grid K split
    // instead (8192^2 M = 64: R = 1, MT = 4, split 2 26.2 us against R = 2, MT = 2 30.3; 4096^2 prefers R = 2:
    // the tuner decides)
    if (bits == 4 && (template_id % 4) == 1 && combo_ok(1, mt)) R = 1;       // (M <= 16: with two slabs per wave, below)
    // QuantMapMode digit 3 above M = 16 (round 5): no lane sharing AND two slabs per wave, the chip filled by the grid K split - the
    // plan round 4's regret sweep wanted on 8192 x 28672 and could not reach through an id (M = 64: 72.6 -> 55.3 us, M = 48 65.0 ->
    // 52.8, M = 32 52.4 -> 45.2).  The automatic digit takes it by itself on layers that deep (K >= 16384: a slice keeps >= 4096 k) whose halved slab count x four slices fills the chip
    const bool deep_sw2 = M > 16 && tile_fn(c, 1, mt, 2) && (units / 16) % 2 == 0 && ov.m_block <= 0 &&
                          ((template_id % 4) == 3 || ((template_id % 4) == 0 && K >= 16384 && !fills((long)(units / 16) * mtiles) && fills((long)(units / 32) * mtiles * 4)));
    if (deep_sw2) R = 1;
    // (m_block = 3 at MT = 1 is not built; the rule this lookup replaced let it plan, and it keeps planning until that is fixed: resolve_kernel)
    if (ov.m_block > 0 && (combo_ok(ov.m_block, mt) || (bits != 3 && ov.m_block == 3 && mt == 1))) R = ov.m_block;
    // SW = 2 slabs per wave (where built - inst_tile_b4.hip: 4-bit, no lane sharing, fp16 up to MT = 4 / bf16 up to MT = 2: the bf16 path
    // keeps a second accumulator set): every activation fragment then serves 8 column tiles and the
    // texture-path traffic per MFMA drops by 40 %.  Worth it once halving the slab count still leaves a
    // workgroup for every CU; QuantMapMode (the last template digit) lets the tuner force either.
    const bool sw_ok = tile_fn(c, R, mt, 2) && (units / 16) % 2 == 0;
    int sw = 1;
    // ... as soon as the halved slab count still fills 55 % of the CUs (28672 x 8192 M = 16: 448 workgroups 43.4 us, 224
    // workgroups 37.1; M = 64: 73.4 -> 54.2; 4096 x 14336 M = 128: 38.2 -> 28.2) - or, at M <= 16, on the tuner's request (digit 1)
    if (sw_ok && (fills((long)(units / 32) * mtiles) || (mt == 1 && M <= 16 && (template_id % 4) == 1))) sw = 2;
    if (sw_ok && bits == 4 && ((template_id % 4) == 3 || deep_sw2)) sw = 2;
    if (bits == 4 && (template_id % 4) == 2) sw = 1;
    if (sw_ok && ov.slabs == 2) sw = 2;
    if (ov.slabs == 1) sw = 1;
    const int slabs = units * R / 16 / sw;                    // wave-sized column groups
    int nw = (t.threads >= 1024) ? 8 : 4;                     // Threads 1024 / 512 templates
    if (ov.waves > 0 && ov.waves <= 8) nw = floor_pow2(ov.waves);
    while (nw > 1 && tile_geom(bits, R, mt, sw, nw, kMaxLds).depth < 2) nw >>= 1;   // ring of >= 2 slots per wave
    int kw = nw;
    while (kw > 1 && K / kw < 256) kw >>= 1;
    // enough workgroups already: keep more of K per wave (fewer partial tiles to reduce)
    while (kw > 1 && (long)slabs * mtiles / (nw / kw) >= 2L * num_sms * t.sms_multiple && K / kw < 1024) kw >>= 1;
    if (t.stages == 3 && kw > 1) kw >>= 1;                    // the tuner's handle on the K split
    if (t.stages == 4 && kw < nw) kw <<= 1;
    if (t.stages == 5 && kw > 2) kw >>= 2;
    if (ov.kw > 0 && ov.kw <= nw) kw = floor_pow2(ov.kw);
    while (nw % kw) kw >>= 1;
    while (slabs % (nw / kw)) kw <<= 1;
    const long wgs = (long)slabs / (nw / kw) * mtiles;
    int splitk = 1;
    // 3-bit layers have no lane-sharing variants (a wave = 16 units x 16 fields = 256 columns): the grid-level K
    // split is their only way to fill the chip, down to 64 k per wave (4096^2 M = 16: 20.5 -> 14.5 us,
    // 4096x14336: 30.8 -> 20.2 us)
    const int k_min = (bits == 3) ? 64 : 256;
    while (wgs * splitk * 2 <= (long)num_sms && K / (splitk * 2 * kw) >= k_min) splitk *= 2;
    if (ov.splitk > 0) splitk = ov.splitk;
    int kps = round_up(ceil_div(K, splitk), 32 * kw);
    splitk = ceil_div(K, kps);
    while (splitk > 1 && (size_t)splitk * M * N * 4 > slab_room(c.workspace_bytes)) {
        splitk >>= 1;
        kps = round_up(ceil_div(K, splitk), 32 * kw);
        splitk = ceil_div(K, kps);
    }
    if (splitk == 1) kps = K;
    Planned q{};
    flute_plan& p = q.p;
    p.family = 2;
    p.m_block = R; p.m_tiles = mt; p.slabs_per_wave = sw; p.waves = nw; p.kw = kw; p.splitk = splitk;
    p.k_per_split = kps;
    // round 4: the K slices of a (slab group, row tile) meet inside the launch (xwg.h, L form) while the slabs are small -
    // the reduce launch it replaces costs >= 2 us; beyond kTileInLaunchMax (4 MB) of slabs the all-CU reduce pass reads them
    // faster than the last arrivers would
    if (splitk > 1 && wgs <= kXwgMaxTiles && (size_t)splitk * M * N * 4 <= kTileInLaunchMax) p.splitk_mode = 1;
    p.grid = (unsigned)(wgs * splitk);
    p.block = (unsigned)(nw * 64);
    p.lds_bytes = (size_t)tile_geom(bits, R, mt, sw, nw, kMaxLds).total;
    p.lut_copies = 32;
    p.workspace_needed = split_slabs(splitk, M, N);
    *out = q;
    return lds_fits(out->p);
}

// The choice of a plan: route a forced family to its planner, else try the automatic candidates in their order.
int choose_plan(const Call& c, Planned* out) {
    const int bits = c.bits, M = c.M, N = c.N, K = c.K;
    const size_t workspace_bytes = c.workspace_bytes;
    const Ovr& ov = c.ov;
    const int fam = ov.family;

    // forced: the family's planner; families 6 and 8 refuse a call they do not fit, the others fall back to the per-wave
    // kernel (family 0: above M = 4, and where the scales outgrow the decode kernels' descriptor)
    if (fam == kFamilyPersistM)
        return plan_persistm(c, ov.slabs, ov.m_tiles, ov.one_shot, &out->p, &out->oa);
    if (fam == kFamilySplitK) {
        const int rc = plan_splitk(bits, c.lg, M, N, K, c.num_sms, ov, workspace_bytes, &out->p);
        return rc ? rc : lds_fits(out->p);
    }
    if (fam == kFamilyFastM) {
        Planned q{};
        if (plan_fastm(c, ov.slabs, &q.p, &q.oa) == FLUTE_OK) { *out = q; return FLUTE_OK; }
    }
    if (fam == kFamilySkinny) {
        Planned q{};
        if (plan_skinny(c, ov, &q.p, &q.oa) == FLUTE_OK) { *out = q; return FLUTE_OK; }
    }
    if (fam == 0 && M <= 4 && decode_fits(c)) return plan_decode(c, out);
    if (fam == kFamilyBlock) {
        const BlockChoice b = choose_block(c);
        if (b.cfg >= 0) return plan_block(c, b, out);
    }
    if (fam >= 0) return plan_tile(c, out);

    // automatic: persistent MFMA decode -> lean MFMA decode -> decode kernels -> skinny (split) -> split-K Stages 5 ->
    // split-K priced against the block / per-wave cost models -> block -> per-wave
    if (persistm_auto(c)) {
        Planned q{};
        if (plan_persistm(c, -1, -1, -1, &q.p, &q.oa) == FLUTE_OK && persistm_taken(c, q.p)) { *out = q; return FLUTE_OK; }
    }
    if (fastm_auto(c)) {
        Planned q{};
        if (plan_fastm(c, -1, &q.p, &q.oa) == FLUTE_OK) { *out = q; return FLUTE_OK; }
    }
    if (decode_auto(c)) return plan_decode(c, out);
    if (const int sk5 = skinny_split_auto(c); sk5 || skinny_auto(c)) {
        Ovr o5 = ov;
        if (sk5) o5.splitk = sk5;
        Planned q{};
        if (plan_skinny(c, o5, &q.p, &q.oa) == FLUTE_OK) { *out = q; return FLUTE_OK; }
    }
    if (splitk_stages5(c)) {
        Planned q{};
        const int rank = c.t.sms_multiple == 1 ? 0 : (c.t.sms_multiple == 2 ? 1 : 2);
        if (plan_splitk(bits, c.lg, M, N, K, c.num_sms, ov, workspace_bytes, &q.p, rank) == FLUTE_OK) { *out = q; return FLUTE_OK; }
    }
    const BlockChoice b = choose_block(c);
    if (splitk_auto(c)) {
        const double alt_us = b.alt_us >= 0.0 ? b.alt_us : flop_us(c, wave_tflops(c));
        double sk_us = 0.0;
        Planned q{};
        if (plan_splitk(bits, c.lg, M, N, K, c.num_sms, ov, workspace_bytes, &q.p, 0, &sk_us) == FLUTE_OK && splitk_auto_taken(c, q.p, sk_us, alt_us)) {
            *out = q;
            return FLUTE_OK;
        }
    }
    return b.cfg >= 0 ? plan_block(c, b, out) : plan_tile(c, out);
}

// The kernel of a plan, from the lookups the planners asked.  A plan whose kernel is not built is refused here, when it is planned:
// FLUTE_ERR_TEMPLATE_ID.
int resolve_kernel(const Call& c, Planned* pl) {
    const flute_plan& p = pl->p;
    const OneArgs& oa = pl->oa;
    const bool decode = p.family == 0;
    pl->fn_had = nullptr;
    if (decode && p.one_shot == 3) { pl->fn = persist_fn(c, p.m_block, oa.depth, oa.nsets, 0); pl->fn_had = persist_fn(c, p.m_block, oa.depth, oa.nsets, 1); }
    else if (decode && p.one_shot == 4) pl->fn = fast_fn(c, p.waves, p.kw, p.ring_depth, p.m_block);
    else if (decode && p.one_shot) { pl->fn = oneshot_fn(c, p.m_block, oa.depth, 0, oa.pipe); pl->fn_had = oneshot_fn(c, p.m_block, oa.depth, 1, oa.pipe); }
    else if (decode) pl->fn = stream_fn(c, p.m_block, p.ring_depth);
    else if (p.family == kFamilySkinny) pl->fn = skinny_fn(c, oa.depth);
    else if (p.family == kFamilyFastM) pl->fn = fastm_fn(c, p.waves, p.ring_depth, oa.lg, p.slabs_per_wave);
    else if (p.family == kFamilyPersistM) pl->fn = persistm_fn(c, oa.lg, p.slabs_per_wave, p.k_chunks, p.waves, p.one_shot);
    else if (p.family == kFamilySplitK) pl->fn = splitk_fn(c, p.m_tiles, p.kw);
    else if (p.family == kFamilyBlock) pl->fn = block_fn(c, p.m_block);
    else pl->fn = tile_fn(c, p.m_block, p.m_tiles, p.slabs_per_wave);
    // the one plan that has no kernel: the per-wave kernel under an override m_block = 3 (plan_tile).  As before, the plan is
    // returned and flute_qgemm_ex refuses to launch it
    if (!pl->fn && p.family == 2 && p.m_block == 3) return FLUTE_OK;
    const bool two = decode && p.one_shot >= 1 && p.one_shot <= 3;      // the kernels whose rotating member is a second instantiation
    return pl->fn && (!two || pl->fn_had) ? FLUTE_OK : FLUTE_ERR_TEMPLATE_ID;
}

// The planner: validate, choose the plan, resolve its kernel.
int make_plan_uncached(int dtype, int bits, int group, int M, int N, int K, int template_id, int num_sms,
                       size_t workspace_bytes, const Ovr& ov, Planned* out) {
    if (dtype != 0 && dtype != 1) return FLUTE_ERR_DTYPE;
    // override families: -1 automatic, 0 decode, 1 / 2 per-wave MFMA kernel, 3 block kernels, 5 skinny MFMA kernel,
    // 6 split-K block kernel, 7 lean MFMA decode kernel, 8 persistent MFMA decode kernel; anything else is a caller error (round 1's family 4 is gone)
    if (ov.family < -1 || ov.family == 4 || ov.family > 8) return FLUTE_ERR_SHAPE;
    Call c;
    const int lrc = check_layer(bits, group, template_id, N, K, std::max(64, group), &c);
    if (lrc) return lrc;
    if (M < 1) return FLUTE_ERR_SHAPE;
    c.dtype = dtype; c.M = M; c.N = N; c.K = K; c.template_id = template_id;
    c.num_sms = num_sms < 1 ? 256 : num_sms; c.workspace_bytes = workspace_bytes; c.ov = ov;
    const int rc = choose_plan(c, out);
    return rc ? rc : resolve_kernel(c, out);
}

// make_plan is a pure function of its arguments and runs on every call of the operator (ranking the decode
// shapes costs a few microseconds of host time - as much as the kernel it plans): memoise the last results
// per host thread.  thread_local, so there is still no shared mutable state.
struct PlanKey {
    int dtype, bits, group, M, N, K, template_id, num_sms;
    size_t workspace_bytes;
    Ovr ov;
    bool operator==(const PlanKey& o) const { return memcmp(this, &o, sizeof(PlanKey)) == 0; }
};
struct PlanEntry { PlanKey key; int rc; Planned plan; bool valid; };     // the plan with its kernel pointers

int make_plan(int dtype, int bits, int group, int M, int N, int K, int template_id, int num_sms,
              size_t workspace_bytes, const Ovr& ov, Planned* out) {
    constexpr int kEntries = 32;
    thread_local PlanEntry cache[kEntries] = {};
    thread_local int next = 0;
    PlanKey key;
    memset(&key, 0, sizeof(key));
    key.dtype = dtype; key.bits = bits; key.group = group; key.M = M; key.N = N; key.K = K;
    key.template_id = template_id; key.num_sms = num_sms; key.workspace_bytes = workspace_bytes; key.ov = ov;
    for (int i = 0; i < kEntries; ++i) {
        const PlanEntry& e = cache[i];
        if (e.valid && e.key == key) {
            if (e.rc == FLUTE_OK) *out = e.plan;
            return e.rc;
        }
    }
    PlanEntry& e = cache[next];
    next = (next + 1) % kEntries;
    e.valid = false;
    e.key = key;
    e.plan = Planned{};
    e.rc = make_plan_uncached(dtype, bits, group, M, N, K, template_id, num_sms, workspace_bytes, ov, &e.plan);
    e.valid = true;
    if (e.rc == FLUTE_OK) *out = e.plan;
    return e.rc;
}

// ---- launching a plan ---------------------------------------------------------------------------------------

// (device, kernel) pairs already granted > 64 KB of dynamic LDS: the attribute is per device, and one
// process may drive several GPUs (accelerate-style sharded inference)
struct BigLds { int dev; const void* fn; };
BigLds g_big_lds[512];
int g_big_lds_n = 0;
std::mutex g_big_lds_mu;                       // flute_qgemm may be called from several host threads

int ensure_lds(const void* fn, size_t bytes) {
    if (bytes <= 65536) return 0;
    std::lock_guard<std::mutex> lock(g_big_lds_mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return FLUTE_ERR_LAUNCH; }
    for (int i = 0; i < g_big_lds_n; ++i)
        if (g_big_lds[i].fn == fn && g_big_lds[i].dev == dev) return 0;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess) {
        (void)hipGetLastError();
        return FLUTE_ERR_LAUNCH;
    }
    if (g_big_lds_n < 512) g_big_lds[g_big_lds_n++] = BigLds{dev, fn};
    return 0;
}

// One launch of a plan's kernel (resolve_kernel; the one plan without a kernel does not come this far): its grid, block and
// dynamic LDS (granted first where it exceeds 64 KB).
int launch(const void* f, const flute_plan& p, void** kargs, hipStream_t st) {
    if (ensure_lds(f, p.lds_bytes)) return FLUTE_ERR_LAUNCH;
    if (hipLaunchKernel(f, dim3(p.grid), dim3(p.block), kargs, p.lds_bytes, st) != hipSuccess) {
        (void)hipGetLastError();
        return FLUTE_ERR_LAUNCH;
    }
    return FLUTE_OK;
}

// FLUTE_STAMPS builds: per-wave phase timestamps (128 B a wave) at byte `offset` of the workspace, where they fit; else none.
// Bytes [0, kXwgFlagBytes) hold the xwg state words, which must stay zero between calls.
uint64_t* stamps_at(void* workspace, size_t workspace_bytes, size_t offset, const flute_plan& p) {
#ifdef FLUTE_STAMPS
    if (workspace && workspace_bytes >= offset + (size_t)p.grid * p.waves * 128)
        return reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + offset);
#endif
    (void)workspace; (void)workspace_bytes; (void)offset; (void)p;
    return nullptr;
}

// The decode kernels can rotate the activations while staging them - every workgroup rotates ALL rows for itself, so the
// fused form costs ~0.33 us per 1024 elements of M x K (measured, profiles/r04/hadamard_fused_vs_separate.json: M = 1
// K = 4096 +1.1 us, M = 1 K = 14336 +4.9, M = 4 K = 3584 +4.5) against ~3.1 us for the separate flute_hadamard launch:
// fused only up to 8192 elements (or when the caller forces the decode family: tests, A/B runs).
bool hadamard_worth_fusing(int M, int K, bool forced) { return forced || (size_t)M * K <= 8192; }
bool hadamard_fusable(const flute_plan& p, int hadamard_size, int M, int K, bool forced) {
    return p.family == 0 && p.one_shot != 4 && hadamard_size >= 2 && hadamard_size <= 512 &&
           (hadamard_size & (hadamard_size - 1)) == 0 && K % hadamard_size == 0 && hadamard_worth_fusing(M, K, forced);
}

}  // namespace

extern "C" {

int flute_abi_version(void) { return FLUTE_AMD_ABI_VERSION; }

const char* flute_strerror(int status) {
    switch (status) {
        case FLUTE_OK: return "ok";
        case FLUTE_ERR_NUM_BITS: return "Unsupported num_bits value";
        case FLUTE_ERR_GROUP_SIZE: return "Unsupported group_size value";
        case FLUTE_ERR_TEMPLATE_ID: return "Unsupported template_id value";
        case FLUTE_ERR_SHAPE: return "Unsupported shape: need N % (16/num_bits*TileP) == 0 (N % 512 for 3 bits), K % 64 == 0, K % group_size == 0";
        case FLUTE_ERR_WORKSPACE: return "workspace too small";
        case FLUTE_ERR_LAUNCH: return "CUDA error: invalid argument (HIP kernel launch failed)";   // flute/tune.py:160 string-matches this prefix
        case FLUTE_ERR_DTYPE: return "Unsupported dtype (fp16 / bf16 only)";
        case FLUTE_ERR_HADAMARD_SIZE: return "Only power of two Hadamard sizes up to 2^15 are supported";
        case FLUTE_ERR_NULL: return "null pointer argument";
        default: return "unknown flute_amd status";
    }
}

int flute_num_templates(int num_bits) {
    if (num_bits == 4) return 144;
    if (num_bits == 2 || num_bits == 3) return 36;
    return 0;
}

int flute_get_template_info(int num_bits, int template_id, flute_template_info* out) {
    if (!out) return FLUTE_ERR_NULL;
    if (num_bits != 2 && num_bits != 3 && num_bits != 4) return FLUTE_ERR_NUM_BITS;
    return decode_template(num_bits, template_id, out) ? FLUTE_OK : FLUTE_ERR_TEMPLATE_ID;
}

int flute_qgemm_plan_ex(int dtype, int num_bits, int group_size, int M, int N, int K, int template_id,
                        int num_sms, size_t workspace_bytes, const flute_overrides* ovr, flute_plan* out) {
    if (!out) return FLUTE_ERR_NULL;
    Planned pl;
    const int rc = make_plan(dtype, num_bits, group_size, M, N, K, template_id, num_sms, workspace_bytes, ovr_of(ovr), &pl);
    if (rc == FLUTE_OK) *out = pl.p;
    return rc;
}

int flute_qgemm_plan(int dtype, int num_bits, int group_size, int M, int N, int K,
                     int template_id, int num_sms, size_t workspace_bytes, flute_plan* out) {
    return flute_qgemm_plan_ex(dtype, num_bits, group_size, M, N, K, template_id, num_sms, workspace_bytes,
                               nullptr, out);
}

int flute_qgemm(int dtype, int num_bits, int group_size, int M, int N, int K, int P,
                const void* A, const void* Q, void* D, const void* S, const void* QM,
                const void* QM2, void* workspace, size_t workspace_bytes, int template_id,
                int num_sms, void* stream) {
    return flute_qgemm_ex(dtype, num_bits, group_size, 0, M, N, K, P, A, Q, D, S, QM, QM2, nullptr,
                          workspace, workspace_bytes, template_id, num_sms, nullptr, stream);
}

// Calls that will fuse the rotation prefer 8-wave workgroups: the rotation is done by the workgroup's waves, 512 k each - 8 waves
// rotate a 4096-k row in one pass (4096x3584 M = 1: 5.5 us with 8 waves, 6.5 with the 4-wave shape the plain product prefers).
// (Applied inside the decode planner only: plan_decode.  Round 3 also forced the four-row decode
// kernel at M = 3, 4 to keep the rotation fused: measured again in round 4, the fused form loses there - above.)
static Ovr hadamard_ovr(Ovr o, int hadamard_size, int M, int K) {
    if (hadamard_size > 1 && hadamard_size <= 512 && M <= 4 && hadamard_worth_fusing(M, K, o.family == 0)) o.had8 = 1;
    return o;
}

int flute_qgemm_hadamard_fused(int dtype, int num_bits, int group_size, int hadamard_size, int M,
                               int N, int K, int template_id, int num_sms, size_t workspace_bytes) {
    Planned pl;
    if (make_plan(dtype, num_bits, group_size, M, N, K, template_id, num_sms, workspace_bytes,
                  hadamard_ovr(ovr_of(nullptr), hadamard_size, M, K), &pl))
        return 0;
    return hadamard_fusable(pl.p, hadamard_size, M, K, false) ? 1 : 0;
}

int flute_qgemm_hadamard(int dtype, int num_bits, int group_size, int hadamard_size, int M, int N,
                         int K, int P, const void* A, const void* Q, void* D, const void* S,
                         const void* QM, const void* QM2, void* x_scratch, void* workspace,
                         size_t workspace_bytes, int template_id, int num_sms, void* stream) {
    return flute_qgemm_ex(dtype, num_bits, group_size, hadamard_size, M, N, K, P, A, Q, D, S, QM, QM2,
                          x_scratch, workspace, workspace_bytes, template_id, num_sms, nullptr, stream);
}

int flute_qgemm_ex(int dtype, int num_bits, int group_size, int hadamard_size, int M, int N, int K, int P,
                   const void* A, const void* Q, void* D, const void* S, const void* QM,
                   const void* QM2, void* x_scratch, void* workspace, size_t workspace_bytes,
                   int template_id, int num_sms, const flute_overrides* ovr, void* stream) {
    (void)QM;   // single-code table: unused, the kernel reads only the pair table (as the reference)
    if (M == 0) return FLUTE_OK;
    if (hadamard_size > 1 && (hadamard_size & (hadamard_size - 1))) return FLUTE_ERR_HADAMARD_SIZE;
    // everything is validated before anything is enqueued
    Planned pl;
    if (!workspace) workspace_bytes = 0;
    const int rc = make_plan(dtype, num_bits, group_size, M, N, K, template_id, num_sms, workspace_bytes,
                             hadamard_ovr(ovr_of(ovr), hadamard_size, M, K), &pl);
    if (rc) return rc;
    if (P != num_bits * (N / 16)) return FLUTE_ERR_SHAPE;
    if (!A || !Q || !D || !S || !QM2) return FLUTE_ERR_NULL;
    const flute_plan& p = pl.p;
    const OneArgs& oa = pl.oa;
    if (p.splitk > 1 && (!workspace || p.workspace_needed > workspace_bytes)) return FLUTE_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    int had_log = 0;
    if (hadamard_size > 1) {
        if (hadamard_fusable(p, hadamard_size, M, K, ovr && ovr->family == 0)) {
            had_log = ilog2(hadamard_size);              // rotated inside the decode kernel's staging
        } else {
            // two launches (qgemm.cpp:201-244): rotate into the caller's scratch, then the plain product
            if (!x_scratch) return FLUTE_ERR_NULL;
            const int hrc = hadamard_dispatch(dtype, A, x_scratch, (size_t)M * K, (uint32_t)hadamard_size, st);
            if (hrc) return hrc;
            A = x_scratch;
        }
    }
    float had_scale = 1.0f / sqrtf((float)(1 << had_log));     // as flute_hadamard: bit-identical results
    const void* fn = had_log > 0 && pl.fn_had ? pl.fn_had : pl.fn;      // the plan's kernel; what follows packs its arguments

    const uint32_t* q32 = reinterpret_cast<const uint32_t*>(Q);
    const uint32_t* qm2 = reinterpret_cast<const uint32_t*>(QM2);
    // workspace: the xwg state words, the fp32 slabs behind them
    uint32_t* state = reinterpret_cast<uint32_t*>(workspace);
    float* partial = workspace ? reinterpret_cast<float*>(static_cast<char*>(workspace) + kXwgFlagBytes) : nullptr;
    // slabs a launch left for the reduce pass (grid K split not combined inside the launch)
    auto then_reduce = [&](int lrc) {
        if (lrc || p.splitk == 1 || p.splitk_mode == 1) return lrc;
        return splitk_reduce_dispatch(dtype, partial, D, (size_t)M * N, p.splitk, st);
    };

    if (p.family == 0 && p.one_shot == 3) {              // persistent one-shot kernel
        uint32_t geo = PersistGeo::pack(oa.lg, p.waves, oa.nch, oa.ipw, had_log, oneshot_x_in_holes(num_bits, p.m_block, K) ? 1 : 0, M);
        int nvis = oa.nvis, nwg = oa.nwg;
        void* kargs[] = {&q32, &S, &A, &qm2, &K, &N, &geo, &nvis, &D, &had_scale, &nwg};
        return launch(fn, p, kargs, st);
    }
    if (p.family == 0 && p.one_shot == 4) {              // lean one-row kernel
        int lg = oa.lg;
        uint64_t* stamps = stamps_at(workspace, workspace_bytes, kXwgFlagBytes, p);
        void* kargs[] = {&q32, &S, &A, &qm2, &D, &N, &lg, &M, &stamps};
        return launch(fn, p, kargs, st);
    }
    if (p.family == 0 && p.one_shot) {                   // one-shot kernel
        uint32_t geo = OneGeo::pack(oa.lg, oa.lkw, oa.upw, oa.pk, oa.ipw, had_log, oneshot_x_in_holes(num_bits, p.m_block, K) ? 1 : 0);
        uint64_t* stamps = stamps_at(workspace, workspace_bytes, kXwgFlagBytes, p);
        void* kargs[] = {&q32, &S, &A, &qm2, &K, &N, &geo, &M, &D, &had_scale, &stamps};
        return launch(fn, p, kargs, st);
    }
    if (p.family == 0) {                                 // ring kernel
        StreamArgs sa = pl.sa;
        sa.A = A; sa.Q = q32; sa.D = D; sa.S = S; sa.QM2 = qm2;
        sa.partial = partial;
        sa.had_log = had_log; sa.had_scale = had_scale; sa.m0 = 0;
        void* kargs[] = {&sa};
        return then_reduce(launch(fn, p, kargs, st));
    }
    if (p.family == kFamilySkinny) {
        uint32_t geo = SkinnyGeo::pack(oa.lg, oa.lkw, oa.ipw, p.splitk);
        uint64_t* stamps = stamps_at(workspace, workspace_bytes, p.workspace_needed ? p.workspace_needed : kXwgFlagBytes, p);   // behind the slabs
        void* kargs[] = {&q32, &S, &A, &qm2, &K, &N, &geo, &M, &D, &stamps, &partial, &state};
        return launch(fn, p, kargs, st);
    }
    if (p.family == kFamilyFastM) {
        uint64_t* stamps = stamps_at(workspace, workspace_bytes, kXwgFlagBytes, p);
        void* kargs[] = {&q32, &S, &A, &qm2, &D, &N, &M, &stamps};
        return launch(fn, p, kargs, st);
    }
    if (p.family == kFamilyPersistM) {
        int nsets = ceil_div(N / 16, p.slabs_per_wave);
        void* kargs[] = {&q32, &S, &A, &qm2, &D, &N, &K, &M, &nsets};
        return launch(fn, p, kargs, st);
    }
    if (p.family == kFamilySplitK) {
        SplitKArgs b;
        memset(&b, 0, sizeof(b));
        b.A = A; b.Q = q32; b.D = D; b.S = S; b.QM2 = qm2;
        b.state = state;
        b.partial = partial;
        b.M = M; b.N = N; b.K = K; b.G = K / group_size; b.lg = ilog2(group_size);
        b.tiles_m = ceil_div(M, p.m_tiles * 16);
        b.splitk = p.splitk; b.k_per_split = p.k_per_split;
        b.pair_lg = -1; b.pair_c8 = 0; b.pair_e = 0;
        const int tile_cols = 256 / p.kw;                      // kw = K parts per workgroup: 128- / 64-column tiles
        // m_block = E: the E row tiles of a column tile that run as consecutive blocks of ONE XCD (0 / 1: natural order)
        const int E = p.m_block;
        if (p.splitk == 1 && E >= 2 && b.tiles_m % E == 0 && ((b.tiles_m / E) & (b.tiles_m / E - 1)) == 0) {
            b.pair_e = ilog2(E);
            b.pair_lg = ilog2(b.tiles_m / E);
            b.pair_c8 = ((b.tiles_m / E) * (N / tile_cols)) & ~7;
        }
        void* kargs[] = {&b};
        return launch(fn, p, kargs, st);
    }
    if (p.family == kFamilyBlock) {
        BlockArgs b;
        memset(&b, 0, sizeof(b));
        b.A = A; b.Q = q32; b.D = D; b.S = S; b.QM2 = qm2;
        b.partial = partial;
        b.M = M; b.N = N; b.K = K; b.G = K / group_size; b.lg = ilog2(group_size);
        const int bm = block_rows(p.m_block);
        b.tiles_m = ceil_div(M, bm); b.tiles_n = N / 256;
        b.splitk = p.splitk; b.k_per_split = p.k_per_split;
        // XCD x (block id % 8) owns a contiguous range of row blocks (their activations then stay in its L2
        // while the weights stream through), else of column blocks
        b.order = (b.tiles_m % 8 == 0) ? 1 : ((b.tiles_n % 8 == 0) ? 2 : 0);
        b.state = (p.splitk > 1 && p.splitk_mode == 1) ? state : nullptr;
        void* kargs[] = {&b};
        return then_reduce(launch(fn, p, kargs, st));
    }

    QGemmArgs a;                                         // per-wave MFMA kernel
    a.A = A; a.Q = q32; a.D = D; a.S = S; a.QM2 = qm2;
    a.partial = partial;
    a.M = M; a.N = N; a.K = K; a.G = K / group_size;
    a.lg = ilog2(group_size);
    a.units = N / ((num_bits == 3) ? 16 : 16 / num_bits);
    a.splitk = p.splitk; a.k_per_split = p.k_per_split; a.kw = p.kw; a.m0 = 0;
    a.lut_shift = 0;
    a.lds_budget = kMaxLds;
    a.lkw = ilog2(p.kw);
    a.state = (p.splitk > 1 && p.splitk_mode == 1) ? state : nullptr;
    a.had_log = had_log;
    a.had_scale = had_scale;
    for (int i = 0; i < 10; ++i) a.geo[i] = 0;
    {
        const TileGeom g = tile_geom(num_bits, p.m_block, p.m_tiles, p.slabs_per_wave, p.waves, kMaxLds);
        a.geo[0] = g.depth; a.geo[1] = g.scale_bytes; a.geo[2] = g.slot_bytes; a.geo[3] = g.wave_bytes;
        a.geo[4] = ceil_div(M, p.m_tiles * 16);
        // slab groups a multiple of the 8 XCDs: row tiles of one slab share an XCD (qgemm_tile.h) - as long
        // as the activations (which every XCD then reads in full) are the smaller operand
        a.geo[5] = (((int)p.grid / p.splitk / a.geo[4]) % 8 == 0 && (long)M * 32 <= (long)num_bits * N) ? 1 : 0;
    }
    void* kargs[] = {&a};
    if (!fn) return FLUTE_ERR_TEMPLATE_ID;               // override m_block = 3 (resolve_kernel)
    return then_reduce(launch(fn, p, kargs, st));
}

int flute_hadamard(int dtype, const void* in, void* out, size_t numel, uint32_t had_size,
                   void* stream) {
    if (!in || !out) return numel == 0 ? FLUTE_OK : FLUTE_ERR_NULL;
    return hadamard_dispatch(dtype, in, out, numel, had_size, reinterpret_cast<hipStream_t>(stream));
}

int flute_unpack(int num_bits, int template_id, int N, int K, const void* Q, void* W,
                 void* stream) {
    Layer l;
    const int rc = check_layer(num_bits, 0, template_id, N, K, 2, &l);
    if (rc) return rc;
    if (!Q || !W) return FLUTE_ERR_NULL;
    return unpack_dispatch(num_bits, l.t.tile_p, N, K, Q, W, reinterpret_cast<hipStream_t>(stream));
}

int flute_dequantize(int dtype, int num_bits, int group_size, int N, int K, int P, int k_begin, int k_count,
                     const void* Q, const void* S, const void* QM2, void* W, int template_id, void* stream) {
    if (!Q || !S || !QM2 || !W) return FLUTE_ERR_NULL;
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    Layer l;
    const int rc = check_layer(num_bits, group_size, template_id, N, K, std::max(64, group_size), &l);
    if (rc) return rc;
    if (P != num_bits * (N / 16)) return FLUTE_ERR_SHAPE;
    if (k_begin < 0 || k_count < 0 || k_begin % 64 || k_count % 64 || k_count > K - k_begin) return FLUTE_ERR_SHAPE;
    if (k_count == 0) return FLUTE_OK;
    return dequant_dispatch(dtype, num_bits, l.t.tile_p, N, K, l.lg, k_begin, k_count, Q, S, QM2, W,
                            reinterpret_cast<hipStream_t>(stream));
}

// flute_qgemm_scale_grad (dT2 null) and _table_grad behind their null-pointer checks: the refusals they share, in their order, and the launch
static int dense_param_grad(int dtype, int num_bits, int group_size, int M, int N, int K, int P, int template_id, const void* dY,
                            const void* X, const void* Q, const void* S, const void* QM2, float* dT2, void* dS, void* scratch,
                            size_t scratch_bytes, int num_sms, void* stream) {
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    Layer l;
    const int rc = check_layer(num_bits, group_size, template_id, N, K, std::max(64, group_size), &l);
    if (rc) return rc;
    if (!group_size) return FLUTE_ERR_GROUP_SIZE;
    if (P != num_bits * (N / 16)) return FLUTE_ERR_SHAPE;
    if (M < 1) return FLUTE_ERR_SHAPE;
    if (dT2 && scratch_bytes < table_grad_scratch_bytes(num_bits, l.lg, M, N, K, dS != nullptr, num_sms)) return FLUTE_ERR_WORKSPACE;
    const ParamGrad a = {dtype, num_bits, l.t.tile_p, l.lg, 1, M, N, K, P, dY, X, nullptr, Q, S, QM2, nullptr, dT2, dS,
                         scratch, scratch_bytes, num_sms};
    return param_grad_dispatch(a, reinterpret_cast<hipStream_t>(stream));
}

int flute_qgemm_scale_grad(int dtype, int num_bits, int group_size, int M, int N, int K, int P, int template_id,
                           const void* dY, const void* X, const void* Q, const void* QM2, void* dS,
                           void* scratch, size_t scratch_bytes, int num_sms, void* stream) {
    if (!dY || !X || !Q || !QM2 || !dS) return FLUTE_ERR_NULL;
    return dense_param_grad(dtype, num_bits, group_size, M, N, K, P, template_id, dY, X, Q, nullptr, QM2, nullptr, dS,
                            scratch_bytes ? scratch : nullptr, scratch ? scratch_bytes : 0, num_sms, stream);
}

int flute_qgemm_table_grad(int dtype, int num_bits, int group_size, int M, int N, int K, int P, int template_id,
                           const void* dY, const void* X, const void* Q, const void* S, const void* QM2, float* dT2,
                           void* dS, void* scratch, size_t scratch_bytes, int num_sms, void* stream) {
    if (!dY || !X || !Q || !S || !dT2 || !scratch || (dS && !QM2)) return FLUTE_ERR_NULL;
    return dense_param_grad(dtype, num_bits, group_size, M, N, K, P, template_id, dY, X, Q, S, QM2, dT2, dS, scratch,
                            scratch_bytes, num_sms, stream);
}

// what both scratch queries refuse (0): the bit width, the group size and the block's shape
static bool grad_scratch_args_ok(int num_bits, int group_size, int N, int K) {
    if (num_bits != 2 && num_bits != 3 && num_bits != 4) return false;
    if (group_size != 32 && group_size != 64 && group_size != 128 && group_size != 256) return false;
    return N >= 1 && K >= 1 && N % 128 == 0 && K % std::max(64, group_size) == 0;
}

size_t flute_qgemm_table_grad_scratch_bytes(int num_bits, int group_size, int M, int N, int K, int want_dS,
                                            int num_sms) {
    if (!grad_scratch_args_ok(num_bits, group_size, N, K) || M < 1) return 0;
    return table_grad_scratch_bytes(num_bits, ilog2(group_size), M, N, K, want_dS != 0, num_sms);
}

// the refusals flute_qgemm_grouped, _glu and _weighted share, in their order: dtype, the layer, the zero group size, then P and the
// negative counts (N: the stack's output columns, rows: T or R)
static int check_grouped(int dtype, int num_bits, int group_size, int template_id, int E, int rows, int N, int K, int P,
                         Layer* l) {
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    const int rc = check_layer(num_bits, group_size, template_id, N, K, std::max(64, group_size), l);
    if (rc) return rc;
    if (!group_size) return FLUTE_ERR_GROUP_SIZE;
    if (P != num_bits * (N / 16) || E < 0 || rows < 0) return FLUTE_ERR_SHAPE;
    return FLUTE_OK;
}

// The two forms of the grouped forward launches (include/flute_amd.h, flute_qgemm_grouped_form): rows = qgemm_grouped.h, blocks =
// qgemm_grouped_blocks.h.  The automatic rule reads host-known quantities only, never `offsets`: the block form where it is
// eligible (grouped_blocks_eligible) and the mean rows per expert, rows / E, reach a threshold - 32 where the experts' column
// blocks alone, E * N / 256 workgroups, fill the chip, 64 where they do not.  Why two: the row form's time grows with the passes
// of 32 rows, the block form's is flat until the 128-row blocks are full, and flat at a higher level where part of the chip idles.
// Read from profiles/grouped_moe_prefill.json ("threshold sweep": W4G64 fp16, us of rows / blocks at even counts, rows / E = 16, 32,
// 48, 64, 96): Mixtral gate / up (448 workgroups) 134 / 121, 177 / 124, 272 / 127, 311 / 131, 446 / 141; E 64 2048 x 2048 (512)
// 116 / 65, 136 / 68, 209 / 72, 226 / 78, 318 / 88; Mixtral down (E 8, N 4096, K 14336: 128 workgroups) 96 / 197, 121 / 198,
// 195 / 198, 221 / 200, 319 / 203 - the routed draws say the same.  On every line from 32 on the rule is within the line's spread
// of the better form.  The crossovers lie lower - below 16 where the chip is full, near 48 where it is not -; the rule stays at
// the lowest values of the sweep that every stack of its kind confirmed, and below them the launch is the row form's, grid included.
static int grouped_blocks_min_mean_rows(int E, int N, int num_sms) {
    const long long sms = num_sms >= 1 ? num_sms : 256;
    return (long long)E * (N / 256) >= sms ? FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS : FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS_PARTIAL;
}
static int grouped_form_auto(int mode, int num_bits, int lg, int E, int rows, int N, int K, int num_sms) {
    if (!grouped_blocks_eligible(mode, num_bits, lg, E, rows, N, K)) return FLUTE_GROUPED_FORM_ROWS;
    return (long long)rows >= (long long)grouped_blocks_min_mean_rows(E, N, num_sms) * E ? FLUTE_GROUPED_FORM_BLOCKS
                                                                                        : FLUTE_GROUPED_FORM_ROWS;
}
// the form a launch takes (1 rows / 2 blocks) for the caller's `form`, or a negative refusal: an unknown form, or blocks forced
// where the block form is not eligible (FLUTE_ERR_SHAPE; after the refusals of check_grouped, before the null pointers)
static int resolve_grouped_form(int form, int mode, int num_bits, int lg, int E, int rows, int N, int K, int num_sms) {
    if (form == FLUTE_GROUPED_FORM_AUTO) return grouped_form_auto(mode, num_bits, lg, E, rows, N, K, num_sms);
    if (form == FLUTE_GROUPED_FORM_ROWS) return form;
    if (form == FLUTE_GROUPED_FORM_BLOCKS && grouped_blocks_eligible(mode, num_bits, lg, E, rows, N, K)) return form;
    return FLUTE_ERR_SHAPE;
}
int flute_qgemm_grouped_form(int mode, int dtype, int num_bits, int group_size, int E, int rows, int N, int K, int template_id,
                             int num_sms) {
    if (mode != FLUTE_GROUPED_PLAIN && mode != FLUTE_GROUPED_GLU && mode != FLUTE_GROUPED_WEIGHTED) return FLUTE_ERR_SHAPE;
    Layer l;
    const int rc = check_grouped(dtype, num_bits, group_size, template_id, E, rows, N, K, num_bits * (N / 16), &l);
    if (rc) return rc;
    return grouped_form_auto(mode, num_bits, l.lg, E, rows, N, K, num_sms);
}

// the refusals of the GLU launches after check_grouped: Tsrc and its relation to `rows` (compared with null, never looked behind)
static int check_glu_rows(int R, int Tsrc, bool has_rows) {
    if (Tsrc < 0) return FLUTE_ERR_SHAPE;
    if (has_rows ? (R > 0 && Tsrc < 1) : Tsrc != R) return FLUTE_ERR_SHAPE;
    return FLUTE_OK;
}

// flute_qgemm_grouped_ex, _glu_ex and _weighted_ex behind their signatures: the operands by name (a mode's own left null by the
// others, one stack in both slots), and the one sequence - check_grouped, the GLU-only Tsrc / rows refusals, the form, the empty
// launch, the null pointers, the dispatch.  (Through these entries the GLU mode has no block form: automatic is the row form at
// every row count, and forcing blocks is refused; its block form is an entry of its own, flute_qgemm_grouped_glu_blocks below.)
static int grouped_forward(GroupedForward g, int group_size, int template_id, int form, void* stream) {
    const bool glu = g.mode == FLUTE_GROUPED_GLU;
    Layer l;
    const int rc = check_grouped(g.dtype, g.num_bits, group_size, template_id, g.E, g.R, g.N, g.K, g.P, &l);
    if (rc) return rc;
    if (glu) {
        const int rows_rc = check_glu_rows(g.R, g.Tsrc, g.rows != nullptr);
        if (rows_rc) return rows_rc;
    }
    g.tile_p = l.t.tile_p;
    g.lg = l.lg;
    g.form = resolve_grouped_form(form, g.mode, g.num_bits, g.lg, g.E, g.R, g.N, g.K, g.num_sms);
    if (g.form < 0) return g.form;
    if (g.E == 0 || g.R == 0) return FLUTE_OK;
    if (!g.X || !g.offsets || !g.Q[0] || !g.S[0] || !g.QM2[0] || !g.Y) return FLUTE_ERR_NULL;
    if (glu && (!g.Q[1] || !g.S[1] || !g.QM2[1])) return FLUTE_ERR_NULL;
    if (g.mode == FLUTE_GROUPED_WEIGHTED && !g.row_weight) return FLUTE_ERR_NULL;
    return qgemm_grouped_dispatch(g, reinterpret_cast<hipStream_t>(stream));
}

int flute_qgemm_grouped_ex(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P, int template_id,
                           const void* X, const void* offsets, const void* Q, const void* S, const void* QM2, void* Y,
                           int num_sms, void* stream, int form) {
    GroupedForward g{};
    g.mode = FLUTE_GROUPED_PLAIN; g.dtype = dtype; g.num_bits = num_bits;
    g.E = E; g.R = T; g.Tsrc = T; g.N = N; g.K = K; g.P = P;
    g.X = X; g.offsets = offsets; g.Y = Y; g.num_sms = num_sms;
    g.Q[0] = g.Q[1] = Q; g.S[0] = g.S[1] = S; g.QM2[0] = g.QM2[1] = QM2;
    return grouped_forward(g, group_size, template_id, form, stream);
}

int flute_qgemm_grouped(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P, int template_id,
                        const void* X, const void* offsets, const void* Q, const void* S, const void* QM2, void* Y,
                        int num_sms, void* stream) {
    return flute_qgemm_grouped_ex(dtype, num_bits, group_size, E, T, N, K, P, template_id, X, offsets, Q, S, QM2, Y, num_sms,
                                  stream, FLUTE_GROUPED_FORM_AUTO);
}

int flute_qgemm_grouped_glu(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K, int P,
                            int template_id, const void* Xsrc, const void* rows, const void* offsets, const void* Qgate,
                            const void* Sgate, const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up,
                            void* H, int num_sms, void* stream) {
    return flute_qgemm_grouped_glu_ex(dtype, num_bits, group_size, E, R, Tsrc, F, K, P, template_id, Xsrc, rows, offsets, Qgate,
                                      Sgate, QM2gate, Qup, Sup, QM2up, H, num_sms, stream, FLUTE_GROUPED_FORM_AUTO);
}

int flute_qgemm_grouped_glu_ex(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K, int P,
                               int template_id, const void* Xsrc, const void* rows, const void* offsets, const void* Qgate,
                               const void* Sgate, const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up,
                               void* H, int num_sms, void* stream, int form) {
    GroupedForward g{};
    g.mode = FLUTE_GROUPED_GLU; g.dtype = dtype; g.num_bits = num_bits;
    g.E = E; g.R = R; g.Tsrc = Tsrc; g.N = F; g.K = K; g.P = P;
    g.X = Xsrc; g.rows = rows; g.offsets = offsets; g.Y = H; g.num_sms = num_sms;
    g.Q[0] = Qgate; g.S[0] = Sgate; g.QM2[0] = QM2gate;
    g.Q[1] = Qup; g.S[1] = Sup; g.QM2[1] = QM2up;
    return grouped_forward(g, group_size, template_id, form, stream);
}

// The block form of the GLU launch behind its own entry (include/flute_amd.h; qgemm_block2.h GM = 3).  What it serves:
// grouped_glu_blocks_eligible and nothing else, asked with an empty launch's E / R / Tsrc raised to 1 - the shape of the layer is
// what is refused, and an empty launch of a served layer returns FLUTE_OK as everywhere.  The query's thresholds are the plain form's
// rule (grouped_blocks_min_mean_rows' split by E * (F / 256) against num_sms) on constants of their own,
// FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS / _PARTIAL = 16 / 48: each the smallest swept mean from which the block launch is not slower
// on any swept stack of its kind (the policy of 3.3m / 3.3n).  The sweep (profiles/grouped_moe_glu_blocks.json, "glu threshold sweep":
// W4G64 fp16, us of row form / block form at even counts, rows / E = 16, 32, 48, 64, 96, 128; the row form pays two K passes per 32
// rows, so its crossover lies lower than the plain launch's): Mixtral gate / up pair (448 workgroups per row block) 254 / 245,
// 329 / 253, 527 / 256, 600 / 266, 872 / 292, 1140 / 307; E 64 2048 x 2048 pair (512) 220 / 134, 255 / 140, 412 / 147, 440 / 153,
// 622 / 169, 804 / 182; E 8 4096 x 4096 pair (128 workgroups: does not fill the chip) 77 / 119, 97 / 120, 154 / 122, 174 / 123,
// 252 / 125, 329 / 128 - the routed draws say the same (at 32 on the last stack 121 / 121, a tie).
static bool grouped_glu_blocks_serves(int num_bits, int lg, int E, int R, int Tsrc, int F, int K) {
    return grouped_glu_blocks_eligible(num_bits, lg, std::max(E, 1), std::max(R, 1), std::max(Tsrc, 1), F, K);
}

int flute_qgemm_grouped_glu_blocks_form(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K,
                                        int template_id, int num_sms) {
    Layer l;
    int rc = check_grouped(dtype, num_bits, group_size, template_id, E, R, F, K, num_bits * (F / 16), &l);
    if (rc) return rc;
    if (Tsrc < 0) return FLUTE_ERR_SHAPE;
    if (E < 1 || R < 1 || !grouped_glu_blocks_eligible(num_bits, l.lg, E, R, Tsrc, F, K)) return FLUTE_GROUPED_FORM_ROWS;
    const long long sms = num_sms >= 1 ? num_sms : 256;
    const int thr = (long long)E * (F / 256) >= sms ? FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS
                                                    : FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS_PARTIAL;
    return (long long)R >= (long long)thr * E ? FLUTE_GROUPED_FORM_BLOCKS : FLUTE_GROUPED_FORM_ROWS;
}

int flute_qgemm_grouped_glu_blocks(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K, int P,
                                   int template_id, const void* Xsrc, const void* rows, const void* offsets, const void* Qgate,
                                   const void* Sgate, const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up,
                                   void* H, int num_sms, void* stream) {
    Layer l;
    int rc = check_grouped(dtype, num_bits, group_size, template_id, E, R, F, K, P, &l);
    if (rc) return rc;
    rc = check_glu_rows(R, Tsrc, rows != nullptr);
    if (rc) return rc;
    if (!grouped_glu_blocks_serves(num_bits, l.lg, E, R, Tsrc, F, K)) return FLUTE_ERR_SHAPE;
    if (E == 0 || R == 0) return FLUTE_OK;
    if (!Xsrc || !offsets || !Qgate || !Sgate || !QM2gate || !Qup || !Sup || !QM2up || !H) return FLUTE_ERR_NULL;
    GroupedForward g{};
    g.mode = FLUTE_GROUPED_GLU; g.form = FLUTE_GROUPED_FORM_BLOCKS; g.dtype = dtype; g.num_bits = num_bits;
    g.tile_p = l.t.tile_p; g.lg = l.lg;
    g.E = E; g.R = R; g.Tsrc = Tsrc; g.N = F; g.K = K; g.P = P;
    g.X = Xsrc; g.rows = rows; g.offsets = offsets; g.Y = H; g.num_sms = num_sms;
    g.Q[0] = Qgate; g.S[0] = Sgate; g.QM2[0] = QM2gate;
    g.Q[1] = Qup; g.S[1] = Sup; g.QM2[1] = QM2up;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return num_bits == 4 ? qgemm_grouped_glu_blocks_unit_b4(g, st) : qgemm_grouped_glu_blocks_unit_b2(g, st);
}

int flute_qgemm_grouped_weighted(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P,
                                 int template_id, const void* X, const void* offsets, const void* Q, const void* S,
                                 const void* QM2, const float* row_weight, void* Y, int num_sms, void* stream) {
    return flute_qgemm_grouped_weighted_ex(dtype, num_bits, group_size, E, T, N, K, P, template_id, X, offsets, Q, S, QM2,
                                           row_weight, Y, num_sms, stream, FLUTE_GROUPED_FORM_AUTO);
}

int flute_qgemm_grouped_weighted_ex(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P,
                                    int template_id, const void* X, const void* offsets, const void* Q, const void* S,
                                    const void* QM2, const float* row_weight, void* Y, int num_sms, void* stream, int form) {
    GroupedForward g{};
    g.mode = FLUTE_GROUPED_WEIGHTED; g.dtype = dtype; g.num_bits = num_bits;
    g.E = E; g.R = T; g.Tsrc = T; g.N = N; g.K = K; g.P = P;
    g.X = X; g.offsets = offsets; g.row_weight = row_weight; g.Y = Y; g.num_sms = num_sms;
    g.Q[0] = g.Q[1] = Q; g.S[0] = g.S[1] = S; g.QM2[0] = g.QM2[1] = QM2;
    return grouped_forward(g, group_size, template_id, form, stream);
}

int flute_qgemm_grouped_input_grad_row_block(void) { return FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK; }

// The two forms of the grouped input gradient (include/flute_amd.h): slabs = qgemm_grouped_input_grad.h, blocks =
// qgemm_grouped_input_grad_blocks.h.  The automatic rule reads host-known quantities only, never `offsets`: the block form where
// it is eligible (grouped_input_grad_blocks_eligible) and the mean rows per expert, R / E, reach a threshold - 32 where one row
// block per expert, E * K / 256 workgroups, already fills the chip, 128 where it does not.  Why two: a block-form workgroup
// walks all of N for 256 k, so with one block per expert the launch takes one workgroup's time however few rows the block
// holds, and where those workgroups are fewer than the compute units the slab form's E * K / 128 fill the chip better until its
// passes over N outnumber that.  Read from profiles/grouped_moe_input_grad_blocks.json ("threshold sweep": W4G64 fp16, us of
// slabs / blocks at even counts, R / E = 16, 32, 48, 64, 96, 128): Mixtral down (E 8, N 4096, K 14336: 448 workgroups)
// 141 / 158, 166 / 160, 206 / 162, 259 / 164, 369 / 201, 481 / 209; E 64 2048 x 2048 (512)
// 76 / 84, 88 / 86, 107 / 88, 136 / 90, 191 / 109, 248 / 116; Mixtral gate / up (E 8, N 14336, K 4096: 128)
// 191 / 262, 215 / 263, 241 / 265, 264 / 268, 322 / 330, 420 / 336 - the
// routed draws say the same.  The constants are the lowest means of the sweep from which blocks is not slower on any stack of
// its kind, on even and on routed counts.  The two forms give equal bits, so the rule decides the time of a launch and nothing else.
static int grouped_input_grad_form_auto(int num_bits, int E, int R, int N, int K, int num_sms) {
    if (!grouped_input_grad_blocks_eligible(num_bits, E, R, N, K)) return FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS;
    const long long sms = num_sms >= 1 ? num_sms : 256;
    const long long mean = (long long)E * (K / kGroupedIgBlockK) >= sms ? FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS
                                                                        : FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS_PARTIAL;
    return (long long)R >= mean * E ? FLUTE_GROUPED_INPUT_GRAD_FORM_BLOCKS : FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS;
}

int flute_qgemm_grouped_input_grad_form(int pair, int dtype, int num_bits, int group_size, int E, int R, int N, int K,
                                        int template_id, int num_sms) {
    (void)pair;                                                    // the pair form is eligible where the single form is
    Layer l;
    const int rc = check_grouped(dtype, num_bits, group_size, template_id, E, R, N, K, num_bits * (N / 16), &l);
    if (rc) return rc;
    return grouped_input_grad_form_auto(num_bits, E, R, N, K, num_sms);
}

int flute_qgemm_grouped_input_grad_ex(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                      int template_id, const void* dY, const void* offsets, const void* Q, const void* S,
                                      const void* QM2, const float* row_weight, const void* dY2, const void* Q2,
                                      const void* S2, const void* QM22, void* dX, int num_sms, void* stream, int form) {
    Layer l;
    const int rc = check_grouped(dtype, num_bits, group_size, template_id, E, R, N, K, P, &l);
    if (rc) return rc;
    const bool pair = dY2 || Q2 || S2 || QM22;
    if (pair && row_weight) return FLUTE_ERR_SHAPE;               // the pair form takes no row weight
    int f = form;
    if (f == FLUTE_GROUPED_INPUT_GRAD_FORM_AUTO) f = grouped_input_grad_form_auto(num_bits, E, R, N, K, num_sms);
    else if (f == FLUTE_GROUPED_INPUT_GRAD_FORM_BLOCKS ? !grouped_input_grad_blocks_eligible(num_bits, E, R, N, K)
                                                       : f != FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS)
        return FLUTE_ERR_SHAPE;                                    // an unknown form, or blocks forced where they do not serve
    if (R == 0) return FLUTE_OK;
    if (!dX) return FLUTE_ERR_NULL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (E == 0)                                                    // no expert serves any row: zeros, as the kernel writes them
        return hipMemsetAsync(dX, 0, (size_t)R * (size_t)K * 2, st) == hipSuccess ? FLUTE_OK : FLUTE_ERR_LAUNCH;
    if (!dY || !offsets || !Q || !S || !QM2 || (pair && (!dY2 || !Q2 || !S2 || !QM22))) return FLUTE_ERR_NULL;
    GroupedInputGrad g{};                                          // (either grid follows from the shapes alone)
    g.form = f; g.dtype = dtype; g.num_bits = num_bits; g.tile_p = l.t.tile_p; g.lg = l.lg;
    g.E = E; g.R = R; g.N = N; g.K = K; g.P = P; g.pair = pair;
    g.dY[0] = dY; g.Q[0] = Q; g.S[0] = S; g.QM2[0] = QM2;
    g.dY[1] = pair ? dY2 : dY; g.Q[1] = pair ? Q2 : Q; g.S[1] = pair ? S2 : S; g.QM2[1] = pair ? QM22 : QM2;
    g.offsets = offsets; g.row_weight = row_weight; g.dX = dX;
    return qgemm_grouped_input_grad_dispatch(g, st);
}

int flute_qgemm_grouped_input_grad(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                   int template_id, const void* dY, const void* offsets, const void* Q, const void* S,
                                   const void* QM2, const float* row_weight, const void* dY2, const void* Q2,
                                   const void* S2, const void* QM22, void* dX, int num_sms, void* stream) {
    return flute_qgemm_grouped_input_grad_ex(dtype, num_bits, group_size, E, R, N, K, P, template_id, dY, offsets, Q, S, QM2,
                                             row_weight, dY2, Q2, S2, QM22, dX, num_sms, stream,
                                             FLUTE_GROUPED_INPUT_GRAD_FORM_AUTO);
}

// flute_qgemm_grouped_scale_grad (table false: S, dT2 and the scratch null) and _table_grad behind their signatures.  The refusals after
// check_grouped: the layout, and the kernel's limits - the workgroup's block is 128 n, the grid's z (the reduce's y) is the expert, a row
// index plus one 32-row step stays an int.  (num_sms plays no part: the grid is (N / 128, ceil(K / 256), E), from the shapes alone.)
static int grouped_param_grad(bool table, int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P, int template_id,
                              const void* dY, const void* X, const void* offsets, const void* Q, const void* S, const void* QM2,
                              const float* row_weight, float* dT2, void* dS, void* scratch, size_t scratch_bytes, int num_sms,
                              void* stream) {
    Layer l;
    const int rc = check_grouped(dtype, num_bits, group_size, template_id, E, R, N, K, P, &l);
    if (rc) return rc;
    if (l.t.tile_p != 32 && l.t.tile_p != 64) return FLUTE_ERR_TEMPLATE_ID;
    if (N % 128 || E > 65535 || R > 0x7fffffff - 64) return FLUTE_ERR_SHAPE;
    if (E == 0) return FLUTE_OK;                                   // dT2 and dS have no element
    if (table ? (!dT2 || !scratch || (dS && !QM2)) : !dS) return FLUTE_ERR_NULL;
    if (table && scratch_bytes < table_grad_grouped_scratch_bytes(num_bits, E, N, K)) return FLUTE_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (R == 0) {                                                  // no expert has a row: zeros, as the kernels write them
        if (table && hipMemsetAsync(dT2, 0, (size_t)E * ((size_t)2 << (2 * num_bits)) * 4, st) != hipSuccess) return FLUTE_ERR_LAUNCH;
        if (dS && hipMemsetAsync(dS, 0, (size_t)E * (size_t)N * (size_t)(K >> l.lg) * 2, st) != hipSuccess) return FLUTE_ERR_LAUNCH;
        return FLUTE_OK;
    }
    if (!dY || !X || !offsets || !Q || (table ? !S : !QM2)) return FLUTE_ERR_NULL;
    const ParamGrad a = {dtype, num_bits, l.t.tile_p, l.lg, E, R, N, K, P, dY, X, offsets, Q, S, QM2, row_weight, dT2, dS,
                         scratch, scratch_bytes, num_sms};
    return param_grad_dispatch(a, st);
}

int flute_qgemm_grouped_scale_grad(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                   int template_id, const void* dY, const void* X, const void* offsets, const void* Q,
                                   const void* QM2, const float* row_weight, void* dS, int num_sms, void* stream) {
    return grouped_param_grad(false, dtype, num_bits, group_size, E, R, N, K, P, template_id, dY, X, offsets, Q, nullptr, QM2,
                              row_weight, nullptr, dS, nullptr, 0, num_sms, stream);
}

int flute_qgemm_grouped_table_grad(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                   int template_id, const void* dY, const void* X, const void* offsets, const void* Q,
                                   const void* S, const void* QM2, const float* row_weight, float* dT2, void* dS,
                                   void* scratch, size_t scratch_bytes, int num_sms, void* stream) {
    return grouped_param_grad(true, dtype, num_bits, group_size, E, R, N, K, P, template_id, dY, X, offsets, Q, S, QM2, row_weight,
                              dT2, dS, scratch, scratch_bytes, num_sms, stream);
}

size_t flute_qgemm_grouped_table_grad_scratch_bytes(int num_bits, int group_size, int E, int N, int K) {
    if (!grad_scratch_args_ok(num_bits, group_size, N, K) || E < 1 || E > 65535) return 0;
    return table_grad_grouped_scratch_bytes(num_bits, E, N, K);
}

// the shapes every routing entry point serves (the workspace query asks nothing else)
static bool moe_route_shape_ok(int T, int k, int E) {
    return T >= 0 && k >= 0 && E >= 0 && E <= FLUTE_MOE_ROUTE_MAX_EXPERTS && (long long)T * k < FLUTE_MOE_ROUTE_MAX_PAIRS;
}
// the refusals flute_moe_route and flute_moe_route_wide share, in their order: the two dtypes, then the shapes
static int check_moe_route(int id_dtype, int weight_dtype, int T, int k, int E) {
    if (id_dtype != FLUTE_I32 && id_dtype != FLUTE_I64) return FLUTE_ERR_DTYPE;
    if (weight_dtype != FLUTE_F16 && weight_dtype != FLUTE_BF16 && weight_dtype != FLUTE_F32) return FLUTE_ERR_DTYPE;
    return moe_route_shape_ok(T, k, E) ? FLUTE_OK : FLUTE_ERR_SHAPE;
}

int flute_moe_route(int id_dtype, int weight_dtype, int T, int k, int E, const void* ids, const void* weights,
                    int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* stream) {
    const int rc = check_moe_route(id_dtype, weight_dtype, T, k, E);
    if (rc) return rc;
    const int P = T * k;
    if (P == 0 && !offsets) return FLUTE_OK;                    // no pair and nowhere to write the E + 1 zeros
    if (P > 0 && (!ids || !perm || !rows || !pos || (weights && !row_weight))) return FLUTE_ERR_NULL;
    if (!offsets) return FLUTE_ERR_NULL;
    return moe_route_dispatch(id_dtype, weight_dtype, P, k, E, ids, weights, offsets, perm, rows, row_weight, pos,
                              reinterpret_cast<hipStream_t>(stream));
}

// the refusals the four gating entry points share, in their order: dtype, scoring and (g non-null: the group-limited forms) group_score,
// then the shapes, then the groups'
static int check_moe_gate(int logit_dtype, int T, int E, int k, const GateGroups* g, int scoring) {
    if (logit_dtype != FLUTE_F16 && logit_dtype != FLUTE_BF16 && logit_dtype != FLUTE_F32) return FLUTE_ERR_DTYPE;
    if (scoring != FLUTE_GATE_SOFTMAX && scoring != FLUTE_GATE_SIGMOID) return FLUTE_ERR_DTYPE;
    if (g && g->group_score != FLUTE_GATE_GROUP_MAX && g->group_score != FLUTE_GATE_GROUP_TOP2SUM) return FLUTE_ERR_DTYPE;
    if (T < 0 || k < 1 || k > E || k > FLUTE_MOE_GATE_MAX_TOPK || E > FLUTE_MOE_ROUTE_MAX_EXPERTS) return FLUTE_ERR_SHAPE;
    if ((long long)T * k >= FLUTE_MOE_ROUTE_MAX_PAIRS) return FLUTE_ERR_SHAPE;
    if (!g) return FLUTE_OK;
    if (g->n_group < 1 || g->n_group > FLUTE_MOE_GATE_MAX_GROUPS) return FLUTE_ERR_SHAPE;
    if (E % g->n_group) return FLUTE_ERR_SHAPE;
    if (g->topk_group < 1 || g->topk_group > g->n_group) return FLUTE_ERR_SHAPE;
    const int gs = E / g->n_group;
    if (k > g->topk_group * gs) return FLUTE_ERR_SHAPE;         // topk_group gs <= E <= 1024
    if (g->group_score == FLUTE_GATE_GROUP_TOP2SUM && gs < 2) return FLUTE_ERR_SHAPE;
    return FLUTE_OK;
}

// the standalone form behind flute_moe_gate (g null) and flute_moe_gate_limited
static int moe_gate_alone(int logit_dtype, int T, int E, int k, const GateGroups* g, int scoring, int renormalize, float scale,
                          const void* logits, const float* bias, int32_t* ids, float* weights, void* stream) {
    const int rc = check_moe_gate(logit_dtype, T, E, k, g, scoring);
    if (rc) return rc;
    if (T == 0) return FLUTE_OK;
    if (!logits || !ids || !weights) return FLUTE_ERR_NULL;
    return moe_gate_dispatch(logit_dtype, T, E, k, g, scoring, renormalize, scale, logits, bias, ids, weights, nullptr, nullptr,
                             nullptr, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

// whether one of the pointers every routed gating entry reads or writes when there is a token is null (offsets: asked on its own)
static bool routed_outputs_null(const void* logits, const int32_t* ids, const float* weights, const int32_t* perm,
                                const int32_t* rows, const float* row_weight, const int32_t* pos) {
    return !logits || !ids || !weights || !perm || !rows || !row_weight || !pos;
}

// the routed form behind flute_moe_gate_route (g null) and flute_moe_gate_route_limited
static int moe_gate_routed(int logit_dtype, int T, int E, int k, const GateGroups* g, int scoring, int renormalize, float scale,
                           const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* offsets, int32_t* perm,
                           int32_t* rows, float* row_weight, int32_t* pos, void* stream) {
    const int rc = check_moe_gate(logit_dtype, T, E, k, g, scoring);
    if (rc) return rc;
    if (T == 0 && !offsets) return FLUTE_OK;                    // no token and nowhere to write the E + 1 zeros
    if (T > 0 && routed_outputs_null(logits, ids, weights, perm, rows, row_weight, pos)) return FLUTE_ERR_NULL;
    if (!offsets) return FLUTE_ERR_NULL;
    return moe_gate_dispatch(logit_dtype, T, E, k, g, scoring, renormalize, scale, logits, bias, ids, weights, offsets, perm,
                             rows, row_weight, pos, reinterpret_cast<hipStream_t>(stream));
}

int flute_moe_gate(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale, const void* logits,
                   const float* bias, int32_t* ids, float* weights, void* stream) {
    return moe_gate_alone(logit_dtype, T, E, k, nullptr, scoring, renormalize, scale, logits, bias, ids, weights, stream);
}

int flute_moe_gate_route(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale,
                         const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* offsets,
                         int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* stream) {
    return moe_gate_routed(logit_dtype, T, E, k, nullptr, scoring, renormalize, scale, logits, bias, ids, weights, offsets, perm,
                           rows, row_weight, pos, stream);
}

int flute_moe_gate_limited(int logit_dtype, int T, int E, int k, int n_group, int topk_group, int group_score, int scoring,
                           int renormalize, float scale, const void* logits, const float* bias, int32_t* ids, float* weights,
                           void* stream) {
    const GateGroups g = {n_group, topk_group, group_score};
    return moe_gate_alone(logit_dtype, T, E, k, &g, scoring, renormalize, scale, logits, bias, ids, weights, stream);
}

int flute_moe_gate_route_limited(int logit_dtype, int T, int E, int k, int n_group, int topk_group, int group_score, int scoring,
                                 int renormalize, float scale, const void* logits, const float* bias, int32_t* ids,
                                 float* weights, int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos,
                                 void* stream) {
    const GateGroups g = {n_group, topk_group, group_score};
    return moe_gate_routed(logit_dtype, T, E, k, &g, scoring, renormalize, scale, logits, bias, ids, weights, offsets, perm, rows,
                           row_weight, pos, stream);
}

// ---- the routing over many workgroups (moe_route_wide.hip) ----------------------------------------------------------------------
// the automatic chunk, a function of (gated, T, k) alone: gated one token per wave and round, ungated about FLUTE_MOE_ROUTE_WIDE_PAIRS
// pairs; either grows to keep C <= FLUTE_MOE_ROUTE_MAX_CHUNKS
static int route_wide_auto_chunk(bool gated, int T, int k) {
    const int want = gated ? FLUTE_MOE_GATE_ROUTE_WIDE_TOKENS : (FLUTE_MOE_ROUTE_WIDE_PAIRS + (k > 0 ? k : 1) - 1) / (k > 0 ? k : 1);
    const int cap = (T + FLUTE_MOE_ROUTE_MAX_CHUNKS - 1) / FLUTE_MOE_ROUTE_MAX_CHUNKS;
    return want > cap ? want : cap;
}
// C for a checked shape, 0 for a chunk_tokens the entries refuse; chunk_tokens 0 is resolved in place.  No pair: one chunk.
static int route_wide_chunks(bool gated, int T, int k, int* chunk_tokens) {
    if (*chunk_tokens < 0) return 0;
    if (*chunk_tokens == 0) *chunk_tokens = route_wide_auto_chunk(gated, T, k);
    if (T == 0 || k == 0) return 1;
    const int C = (int)(((long long)T + *chunk_tokens - 1) / *chunk_tokens);
    return C <= FLUTE_MOE_ROUTE_MAX_CHUNKS ? C : 0;
}
static size_t route_wide_bytes(int C, int E) { return (size_t)(C + 1) * (size_t)(E + 1) * sizeof(int32_t); }

size_t flute_moe_route_wide_workspace(int T, int k, int E, int chunk_tokens) {
    if (!moe_route_shape_ok(T, k, E)) return 0;
    int ct = chunk_tokens, ctg = chunk_tokens;                     // automatic: enough for either entry's own chunk
    const int Cu = route_wide_chunks(false, T, k, &ct), Cg = route_wide_chunks(true, T, k, &ctg);
    const int C = Cg > Cu ? Cg : Cu;
    return C ? route_wide_bytes(C, E) : 0;
}

int flute_moe_route_wide(int id_dtype, int weight_dtype, int T, int k, int E, const void* ids, const void* weights,
                         int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* workspace,
                         size_t workspace_bytes, int chunk_tokens, void* stream) {
    const int rc = check_moe_route(id_dtype, weight_dtype, T, k, E);
    if (rc) return rc;
    const int C = route_wide_chunks(false, T, k, &chunk_tokens);
    if (C == 0) return FLUTE_ERR_SHAPE;
    const int P = T * k;
    if (P == 0 && !offsets) return FLUTE_OK;
    if (P > 0 && (!ids || !perm || !rows || !pos || (weights && !row_weight))) return FLUTE_ERR_NULL;
    if (!offsets || (C > 1 && !workspace)) return FLUTE_ERR_NULL;
    if (C > 1 && workspace_bytes < route_wide_bytes(C, E)) return FLUTE_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (C == 1) return moe_route_dispatch(id_dtype, weight_dtype, P, k, E, ids, weights, offsets, perm, rows, row_weight, pos, st);
    return moe_route_wide_dispatch(id_dtype, weight_dtype, T, k, E, chunk_tokens, ids, weights, offsets, perm, rows, row_weight, pos,
                                   workspace, st);
}

int flute_moe_gate_route_wide(int logit_dtype, int T, int E, int k, int n_group, int topk_group, int group_score, int scoring,
                              int renormalize, float scale, const void* logits, const float* bias, int32_t* ids, float* weights,
                              int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* workspace,
                              size_t workspace_bytes, int chunk_tokens, void* stream) {
    const GateGroups g = {n_group, topk_group, group_score};
    const int rc = check_moe_gate(logit_dtype, T, E, k, &g, scoring);
    if (rc) return rc;
    const int C = route_wide_chunks(true, T, k, &chunk_tokens);
    if (C == 0) return FLUTE_ERR_SHAPE;
    if (T == 0 && !offsets) return FLUTE_OK;
    if (T > 0 && routed_outputs_null(logits, ids, weights, perm, rows, row_weight, pos)) return FLUTE_ERR_NULL;
    if (!offsets || (C > 1 && !workspace)) return FLUTE_ERR_NULL;
    if (C > 1 && workspace_bytes < route_wide_bytes(C, E)) return FLUTE_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (C == 1)
        return moe_gate_dispatch(logit_dtype, T, E, k, &g, scoring, renormalize, scale, logits, bias, ids, weights, offsets, perm, rows,
                                 row_weight, pos, st);
    return moe_gate_route_wide_dispatch(logit_dtype, T, E, k, &g, scoring, renormalize, scale, chunk_tokens, logits, bias, ids, weights,
                                        offsets, perm, rows, row_weight, pos, workspace, st);
}

int flute_moe_route_form(int gated, int T, int k, int E, int num_sms) {
    if (T < 0 || k < 0 || E < 0 || E > FLUTE_MOE_ROUTE_MAX_EXPERTS) return FLUTE_ERR_SHAPE;
    if (gated && (k < 1 || k > E || k > FLUTE_MOE_GATE_MAX_TOPK)) return FLUTE_ERR_SHAPE;
    if ((long long)T * k >= FLUTE_MOE_ROUTE_MAX_PAIRS) return FLUTE_ERR_SHAPE;
    (void)num_sms;                                                 // the crossovers were measured on a whole part; see the header
    int ct = 0;
    return (long long)T * k >= FLUTE_MOE_ROUTE_WIDE_MIN_PAIRS && route_wide_chunks(gated != 0, T, k, &ct) > 1
               ? FLUTE_MOE_ROUTE_FORM_WIDE
               : FLUTE_MOE_ROUTE_FORM_ONE;
}

int flute_moe_combine(int dtype, int T, int k, int E, int N, const void* Y, const int32_t* pos, const int32_t* offsets,
                      void* out, void* stream) {
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    if (T < 0 || k < 0 || E < 0 || N < 0 || N % 8) return FLUTE_ERR_SHAPE;
    if ((long long)T * k > 0x7fffffffLL || (T > 0 && N > 0 && moe_combine_grid(T, N) == 0)) return FLUTE_ERR_SHAPE;
    if (T == 0 || N == 0) return FLUTE_OK;
    if (!offsets || !out || (k > 0 && (!Y || !pos))) return FLUTE_ERR_NULL;
    return moe_combine_dispatch(dtype, T, k, E, N, Y, pos, offsets, out, reinterpret_cast<hipStream_t>(stream));
}

int flute_swiglu_grad(int dtype, int R, int F, int E, const void* g, const void* u, const void* dh, const int32_t* offsets,
                      void* dg, void* du, void* stream) {
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    if (R < 0 || F < 0 || F % 8 || (offsets && E < 0)) return FLUTE_ERR_SHAPE;
    if (R > 0 && F > 0 && row_stream_grid(R, F) == 0) return FLUTE_ERR_SHAPE;
    if (R == 0 || F == 0) return FLUTE_OK;
    if (!g || !u || !dh || !dg || !du) return FLUTE_ERR_NULL;
    return swiglu_grad_dispatch(dtype, R, F, E, g, u, dh, offsets, dg, du, reinterpret_cast<hipStream_t>(stream));
}

int flute_moe_gather(int dtype, int R, int Tsrc, int K, int E, const void* X, const int32_t* rows, const int32_t* offsets,
                     void* out, void* stream) {
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    if (R < 0 || Tsrc < 0 || K < 0 || K % 8 || (offsets && E < 0)) return FLUTE_ERR_SHAPE;
    if (R > 0 && K > 0 && (Tsrc == 0 || row_stream_grid(R, K) == 0)) return FLUTE_ERR_SHAPE;
    if (R == 0 || K == 0) return FLUTE_OK;
    if (!X || !rows || !out) return FLUTE_ERR_NULL;
    return moe_gather_dispatch(R, Tsrc, K, E, X, rows, offsets, out, reinterpret_cast<hipStream_t>(stream));
}

int flute_moe_weight_grad(int dtype, int R, int K, int E, const void* dHp, const void* H, const float* row_weight,
                          const int32_t* offsets, float* d_row_weight, void* dH, void* stream) {
    if (dtype != FLUTE_F16 && dtype != FLUTE_BF16) return FLUTE_ERR_DTYPE;
    if (R < 0 || K < 0 || K % 8 || (offsets && E < 0)) return FLUTE_ERR_SHAPE;
    if (R == 0 || K == 0) return FLUTE_OK;
    if (!dHp || !H || !d_row_weight || (row_weight != nullptr) != (dH != nullptr)) return FLUTE_ERR_NULL;
    return moe_weight_grad_dispatch(dtype, R, K, E, dHp, H, row_weight, offsets, d_row_weight, dH,
                                    reinterpret_cast<hipStream_t>(stream));
}

int flute_moe_gate_grad(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale, const void* logits,
                        const int32_t* ids, const float* d_weights, const float* d_row_weight, const int32_t* pos, void* d_logits,
                        void* stream) {
    const int rc = check_moe_gate(logit_dtype, T, E, k, nullptr, scoring);
    if (rc) return rc;
    if (T == 0) return FLUTE_OK;
    if (!logits || !ids || !d_logits) return FLUTE_ERR_NULL;
    if ((!d_weights && !d_row_weight && !pos) || (d_row_weight != nullptr) != (pos != nullptr)) return FLUTE_ERR_NULL;
    return moe_gate_grad_dispatch(logit_dtype, T, E, k, scoring, renormalize, scale, logits, ids, d_weights, d_row_weight, pos,
                                  d_logits, reinterpret_cast<hipStream_t>(stream));
}

// ---- the router's auxiliary losses (moe_aux.hip) ----------------------------------------------------------------------------------
// C for a checked T, 0 for a chunk_tokens the entries refuse; chunk_tokens 0 is resolved in place, from T alone
static int aux_chunks(int T, int* chunk_tokens) {
    if (*chunk_tokens < 0) return 0;
    if (*chunk_tokens == 0) {
        const int cap = (T + FLUTE_MOE_AUX_AUTO_CHUNKS - 1) / FLUTE_MOE_AUX_AUTO_CHUNKS;
        *chunk_tokens = cap > FLUTE_MOE_AUX_CHUNK_TOKENS ? cap : FLUTE_MOE_AUX_CHUNK_TOKENS;
    }
    const long long C = ((long long)T + *chunk_tokens - 1) / *chunk_tokens;
    return C <= FLUTE_MOE_ROUTE_MAX_CHUNKS ? (int)C : 0;
}
static bool aux_shape_ok(int T, int E) {
    return T >= 1 && E >= 1 && E <= FLUTE_MOE_ROUTE_MAX_EXPERTS && T < FLUTE_MOE_ROUTE_MAX_PAIRS;
}

size_t flute_moe_aux_loss_workspace(int T, int E, int chunk_tokens) {
    if (!aux_shape_ok(T, E)) return 0;
    const int C = aux_chunks(T, &chunk_tokens);
    return (size_t)C * (size_t)(2 * E + 1) * sizeof(int32_t);
}

int flute_moe_aux_loss(int logit_dtype, int T, int E, int k, int scoring, int chunk_tokens, const void* logits, const int32_t* ids,
                       void* workspace, int32_t* load, float* importance, float* losses, void* stream) {
    const int rc = check_moe_gate(logit_dtype, T, E, k, nullptr, scoring);
    if (rc) return rc;
    if (T < 1) return FLUTE_ERR_SHAPE;
    const int C = aux_chunks(T, &chunk_tokens);
    if (C == 0) return FLUTE_ERR_SHAPE;
    if (!logits || !ids || !workspace || !load || !importance || !losses) return FLUTE_ERR_NULL;
    return moe_aux_loss_dispatch(logit_dtype, T, E, k, scoring, chunk_tokens, logits, ids, workspace, load, importance, losses,
                                 reinterpret_cast<hipStream_t>(stream));
}

int flute_moe_aux_loss_grad(int logit_dtype, int T, int E, int scoring, const void* logits, const int32_t* load, const float* grads,
                            void* d_logits, void* stream) {
    if (logit_dtype != FLUTE_F16 && logit_dtype != FLUTE_BF16 && logit_dtype != FLUTE_F32) return FLUTE_ERR_DTYPE;
    if (scoring != FLUTE_GATE_SOFTMAX && scoring != FLUTE_GATE_SIGMOID) return FLUTE_ERR_DTYPE;
    if (!aux_shape_ok(T, E)) return FLUTE_ERR_SHAPE;
    if (!logits || !load || !grads || !d_logits) return FLUTE_ERR_NULL;
    return moe_aux_loss_grad_dispatch(logit_dtype, T, E, scoring, logits, load, grads, d_logits,
                                      reinterpret_cast<hipStream_t>(stream));
}

int flute_debug_stream_read(const void* src, void* sink, size_t bytes, int bytes_per_wave,
                            int grid, int block, void* stream) {
    if (!src || !sink || bytes_per_wave < 8192 || bytes_per_wave % 8192) return FLUTE_ERR_SHAPE;
    return stream_read_dispatch(src, sink, bytes, bytes_per_wave, grid, block,
                                reinterpret_cast<hipStream_t>(stream));
}

int flute_debug_timestamp(void* dst, void* stream) {
    if (!dst) return FLUTE_ERR_NULL;
    return timestamp_dispatch(dst, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
