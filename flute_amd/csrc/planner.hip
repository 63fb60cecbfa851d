// Host side of the C ABI, second planner unit: the template table, what every entry point checks of a layer, the automatic
// rules, the block and per-wave planners, the choice of a plan and its kernel, and make_plan with its per-thread cache.  Instead of
// the reference's one Stream-K kernel with 36/144 tile variants there are several kernel families (flute_plan::family: decode
// kernels for a few rows, per-wave / skinny / split-K / block-tiled MFMA kernels above) whose launch geometry is derived from the
// template's knobs and the problem shape.  The kernel lookups and the decode families' shape planners it calls are
// planner_decode.hip's (host.h).  No device code.
#include <algorithm>
#include <string.h>

#include "host.h"
#include "kernels.h"
#include "qgemm_tile.h"

namespace flute_amd::host {

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

namespace {

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

}  // namespace

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

}  // namespace flute_amd::host
