// Host side of the C ABI, the mixture-of-experts entry points: routing, gating, the routing over many workgroups, combine, the
// SwiGLU gradient, gather, the router's gradients and its auxiliary losses.  Nothing of the planner.  No device code.
#include "kernels.h"

using namespace flute_amd;

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

extern "C" {

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

}  // extern "C"
