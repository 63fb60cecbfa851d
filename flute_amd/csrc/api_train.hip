// Host side of the C ABI, the training and grouped entry points: the dense and grouped parameter gradients with their scratch
// queries, the grouped forward launches (rows, blocks, GLU blocks) with their form queries, and the grouped input gradient.  Of the
// planner they need the layer check alone (host.h).  No device code.
#include <algorithm>

#include "host.h"
#include "kernels.h"
#include "grouped_rows.h"

using namespace flute_amd;
using namespace flute_amd::host;

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

// what both scratch queries refuse (0): the bit width, the group size and the block's shape
static bool grad_scratch_args_ok(int num_bits, int group_size, int N, int K) {
    if (num_bits != 2 && num_bits != 3 && num_bits != 4) return false;
    if (group_size != 32 && group_size != 64 && group_size != 128 && group_size != 256) return false;
    return N >= 1 && K >= 1 && N % 128 == 0 && K % std::max(64, group_size) == 0;
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

// The threshold of the three automatic form rules below: the block form from a mean of `full` rows per expert where the experts'
// workgroups, wgs_per_expert each, fill the chip, `partial` where they do not
static int min_mean_rows(int wgs_per_expert, int E, int num_sms, int full, int partial) {
    const long long sms = num_sms >= 1 ? num_sms : 256;
    return (long long)E * wgs_per_expert >= sms ? full : partial;
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
    return min_mean_rows(N / 256, E, num_sms, FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS, FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS_PARTIAL);
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

// the operands of a GLU launch by name, as flute_qgemm_grouped_glu_ex and flute_qgemm_grouped_glu_blocks both hand them on (form,
// tile_p and lg are left to the caller)
static GroupedForward glu_operands(int dtype, int num_bits, int E, int R, int Tsrc, int F, int K, int P, const void* Xsrc,
                                   const void* rows, const void* offsets, const void* Qgate, const void* Sgate,
                                   const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up, void* H,
                                   int num_sms) {
    GroupedForward g{};
    g.mode = FLUTE_GROUPED_GLU; g.dtype = dtype; g.num_bits = num_bits;
    g.E = E; g.R = R; g.Tsrc = Tsrc; g.N = F; g.K = K; g.P = P;
    g.X = Xsrc; g.rows = rows; g.offsets = offsets; g.Y = H; g.num_sms = num_sms;
    g.Q[0] = Qgate; g.S[0] = Sgate; g.QM2[0] = QM2gate;
    g.Q[1] = Qup; g.S[1] = Sup; g.QM2[1] = QM2up;
    return g;
}

// The block form of the GLU launch behind its own entry (include/flute_amd.h; qgemm_block2.h GM = 3).  What it serves:
// grouped_glu_blocks_eligible and nothing else, asked with an empty launch's E / R / Tsrc raised to 1 - the shape of the layer is
// what is refused, and an empty launch of a served layer returns FLUTE_OK as everywhere.  The query's thresholds are the plain form's
// rule (min_mean_rows: the split by E * (F / 256) against num_sms) on constants of their own,
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
    const long long mean = min_mean_rows(K / kGroupedIgBlockK, E, num_sms, FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS,
                                         FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS_PARTIAL);
    return (long long)R >= mean * E ? FLUTE_GROUPED_INPUT_GRAD_FORM_BLOCKS : FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS;
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

extern "C" {

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

size_t flute_qgemm_table_grad_scratch_bytes(int num_bits, int group_size, int M, int N, int K, int want_dS,
                                            int num_sms) {
    if (!grad_scratch_args_ok(num_bits, group_size, N, K) || M < 1) return 0;
    return table_grad_scratch_bytes(num_bits, ilog2(group_size), M, N, K, want_dS != 0, num_sms);
}

int flute_qgemm_grouped_form(int mode, int dtype, int num_bits, int group_size, int E, int rows, int N, int K, int template_id,
                             int num_sms) {
    if (mode != FLUTE_GROUPED_PLAIN && mode != FLUTE_GROUPED_GLU && mode != FLUTE_GROUPED_WEIGHTED) return FLUTE_ERR_SHAPE;
    Layer l;
    const int rc = check_grouped(dtype, num_bits, group_size, template_id, E, rows, N, K, num_bits * (N / 16), &l);
    if (rc) return rc;
    return grouped_form_auto(mode, num_bits, l.lg, E, rows, N, K, num_sms);
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
    const GroupedForward g = glu_operands(dtype, num_bits, E, R, Tsrc, F, K, P, Xsrc, rows, offsets, Qgate, Sgate, QM2gate, Qup, Sup,
                                          QM2up, H, num_sms);
    return grouped_forward(g, group_size, template_id, form, stream);
}

int flute_qgemm_grouped_glu_blocks_form(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K,
                                        int template_id, int num_sms) {
    Layer l;
    int rc = check_grouped(dtype, num_bits, group_size, template_id, E, R, F, K, num_bits * (F / 16), &l);
    if (rc) return rc;
    if (Tsrc < 0) return FLUTE_ERR_SHAPE;
    if (E < 1 || R < 1 || !grouped_glu_blocks_eligible(num_bits, l.lg, E, R, Tsrc, F, K)) return FLUTE_GROUPED_FORM_ROWS;
    const int thr = min_mean_rows(F / 256, E, num_sms, FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS,
                                  FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS_PARTIAL);
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
    GroupedForward g = glu_operands(dtype, num_bits, E, R, Tsrc, F, K, P, Xsrc, rows, offsets, Qgate, Sgate, QM2gate, Qup, Sup, QM2up,
                                    H, num_sms);
    g.form = FLUTE_GROUPED_FORM_BLOCKS; g.tile_p = l.t.tile_p; g.lg = l.lg;
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

}  // extern "C"
