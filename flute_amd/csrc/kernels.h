// Kernel lookups defined by the instantiation units (inst_*.hip), one row list per family and unit: the entry point of a
// shape, nullptr where that shape is not built.  planner_decode.hip asks them while it plans (which shapes exist) and once more when
// the plan is made (resolve_kernel: a plan without a built kernel is refused there, FLUTE_ERR_TEMPLATE_ID); a launch looks nothing up.
#pragma once
#include "common.h"
#include "../../include/flute_amd.h"

namespace flute_amd {

typedef void (*QGemmKernel)(const QGemmArgs);

// streaming decode kernel (qgemm_stream.h): mb rows per pass (1/2/4), depth = ring slots (2/4; b=3: 2)
struct StreamArgs;
typedef void (*StreamKernel)(const StreamArgs);
StreamKernel stream_kernel_b4(int dtype, int tile_p, int mb, int depth);
StreamKernel stream_kernel_b3(int dtype, int tile_p, int mb, int depth);
StreamKernel stream_kernel_b2(int dtype, int tile_p, int mb, int depth);
// one-shot decode kernel (qgemm_oneshot.h): mb rows per pass (1/2/4; b=3: 1/2), depth = pieces per wave (4/8; b=3: 2/4), had = fused
// Hadamard pre-rotation, pipe = software-pipelined lookup groups (every wave of the launch holds `depth` whole pieces)
typedef void (*OneKernel)(const uint32_t*, const void*, const void*, const uint32_t*, int, int, uint32_t, int, void*, float, uint64_t*);
OneKernel oneshot_kernel_b4_f16(int tile_p, int mb, int depth, int had, int pipe);
OneKernel oneshot_kernel_b4_bf16(int tile_p, int mb, int depth, int had, int pipe);
OneKernel oneshot_kernel_b2_f16(int tile_p, int mb, int depth, int had, int pipe);
OneKernel oneshot_kernel_b2_bf16(int tile_p, int mb, int depth, int had, int pipe);
OneKernel oneshot_kernel_b3(int dtype, int tile_p, int mb, int depth, int had, int pipe);
// lean decode kernel (qgemm_fast.h): 4 bits, K = 512 * depth * kw; waves per workgroup, waves per unit row, pieces per wave, rows per pass (1/2/4)
typedef void (*FastKernel)(const uint32_t*, const void*, const void*, const uint32_t*, void*, int, int, int, uint64_t*);
FastKernel fast_kernel_b4(int dtype, int tile_p, int waves, int kw, int depth, int mb);
// lean MFMA decode kernel (qgemm_fastm.h): 4 bits, M <= 16, a workgroup = 4 unit rows x all of K = 128 * nm * waves; lg = log2(group size)
typedef void (*FastMKernel)(const uint32_t*, const void*, const void*, const uint32_t*, void*, int, int, uint64_t*);
FastMKernel fastm_kernel_b4(int dtype, int tile_p, int waves, int nm, int lg, int ng);   // ng: column groups (4 unit rows each) per workgroup, 1 .. 3
// persistent MFMA decode kernel (qgemm_persistm.h): 4 / 2 bits, M <= 16, K % 128 == 0; lg = log2(group size) (6 / 7), ng: column groups per set (1 .. 3),
// xr: activation requests per macro-step (1, 2, 4: M <= 4 xr)
typedef void (*PersistMKernel)(const uint32_t*, const void*, const void*, const uint32_t*, void*, int, int, int, int);
PersistMKernel persistm_kernel_b4_f16(int tile_p, int lg, int ng, int xr, int waves, int xres);    // waves: 8; xres: activations resident in LDS (K * xr <= 8192; (ng, xr) in (1..2, 1), (1..3, 2))
PersistMKernel persistm_kernel_b4_bf16(int tile_p, int lg, int ng, int xr, int waves, int xres);
PersistMKernel persistm_kernel_b2_f16(int tile_p, int lg, int ng, int xr, int waves, int xres);     // 2-bit member (a group = two unit rows of eight columns)
PersistMKernel persistm_kernel_b2_bf16(int tile_p, int lg, int ng, int xr, int waves, int xres);
// persistent one-shot decode kernel (qgemm_persist.h): mb rows per pass (1/2), depth = pieces per segment, nsets = register sets
typedef void (*PersistKernel)(const uint32_t*, const void*, const void*, const uint32_t*, int, int, uint32_t, int, void*, float, int);
PersistKernel persist_kernel_b4(int dtype, int tile_p, int mb, int depth, int nsets, int had);
PersistKernel persist_kernel_b2(int dtype, int tile_p, int mb, int depth, int nsets, int had);
PersistKernel persist_kernel_b3(int dtype, int tile_p, int mb, int depth, int nsets, int had);
// skinny MFMA kernel (qgemm_skinny.h): 4-bit, M <= 16, depth = k-steps per wave (4/8/16)
typedef void (*SkinnyKernel)(const uint32_t*, const void*, const void*, const uint32_t*, int, int, uint32_t, int, void*, uint64_t*, float*, uint32_t*);
SkinnyKernel skinny_kernel_b4(int dtype, int tile_p, int depth);
// block-tiled prefill kernels (qgemm_block2.h / qgemm_block3.h): cfg 4 = 256 x 256 block, cfg 5 = 128 x 256, 8 + RT = skinny 3-bit blocks
struct BlockArgs;
typedef void (*BlockKernel)(const BlockArgs);
BlockKernel block_kernel_b4(int dtype, int tile_p, int cfg);
BlockKernel block_kernel_b2(int dtype, int tile_p, int cfg);
BlockKernel block_kernel_b3(int dtype, int tile_p, int cfg);
// split-K block kernel (qgemm_splitk.h): 128 x 128 tiles, K split over workgroups, combined in the launch (xwg.h)
struct SplitKArgs;
typedef void (*SplitKKernel)(const SplitKArgs);
SplitKKernel splitk_kernel(int bits, int dtype, int tile_p, int rt, int kp);   // rt: row tiles per workgroup (8 / 4), kp: K parts per workgroup (2; 4 with rt 4)
// MFMA kernel (qgemm_tile.h): r lanes share one unit's words (1, 2, 4; b=3: 1), mt 16-row tiles per wave
QGemmKernel tile_kernel_b4(int dtype, int tile_p, int r, int mt, int sw);   // sw: slabs per wave (1, 2)
QGemmKernel tile_kernel_b3(int dtype, int tile_p, int r, int mt);
QGemmKernel tile_kernel_b2(int dtype, int tile_p, int r, int mt);

int hadamard_dispatch(int dtype, const void* in, void* out, size_t numel, uint32_t h,
                      hipStream_t stream);
int unpack_dispatch(int num_bits, int tile_p, int N, int K, const void* Q, void* W,
                    hipStream_t stream);
// dense dequantized weight [N, k_count] (dequant.hip); lg = log2(group size)
int dequant_dispatch(int dtype, int num_bits, int tile_p, int N, int K, int lg, int k_begin, int k_count,
                     const void* Q, const void* S, const void* QM2, void* W, hipStream_t stream);
// the parameter gradients of a packed layer or of a stack of E (param_grad.hip states what they compute): with dT2 the table gradient
// [E][4^b][2] fp32, with dS the scale gradient [E][N, K / g] T, or both from one main launch.  offsets null: the dense form over
// rows [0, rows), which splits the rows through the scratch when the blocks do not fill the chip (a scale-only call takes what
// scratch it is given, a null one included).  offsets [E + 1] int32, read on the device only: expert e over the rows the table
// gives it, row_weight [rows] fp32 or null, the grid from the shapes alone.  With dT2 the scratch holds table_grad_scratch_bytes or
// table_grad_grouped_scratch_bytes, the only places its size is computed.  S is read with dT2, QM2 with dS.
struct ParamGrad {
    int dtype, num_bits, tile_p, lg;
    int E, rows, N, K, P;                             // (E and P: the grouped form's)
    const void *dY, *X, *offsets, *Q, *S, *QM2, *row_weight;
    float* dT2;
    void* dS;
    void* scratch;
    size_t scratch_bytes;                             // (read by the dense scale-only form)
    int num_sms;
};
int param_grad_dispatch(const ParamGrad& a, hipStream_t stream);
size_t table_grad_scratch_bytes(int num_bits, int lg, int M, int N, int K, int want_dS, int num_sms);
size_t table_grad_grouped_scratch_bytes(int num_bits, int E, int N, int K);
// One grouped forward launch over E stacked layers and rows sorted by expert (what every grouped kernel reads out of offsets [E + 1],
// int32, device only: grouped_rows.h).  api_train.hip fills it by name; a unit fills its kernel's argument struct from it.
struct GroupedForward {
    int mode;                                         // FLUTE_GROUPED_PLAIN / _GLU / _WEIGHTED
    int form;                                         // resolved: FLUTE_GROUPED_FORM_ROWS (qgemm_grouped.h) / _BLOCKS (qgemm_grouped_blocks.h)
    int dtype, num_bits, tile_p, lg;
    int E, R, Tsrc, N, K, P;                          // R sorted rows; Tsrc rows of X (Glu with `rows`; else R)
    const void *X, *rows, *offsets;                   // rows [R] int32 or null: Glu only
    const void *Q[2], *S[2], *QM2[2];                 // the stack (Glu: gate, up; else both slots hold the one stack)
    const float* row_weight;                          // [R]: Weighted only
    void* Y;                                          // [R, N]
    int num_sms;
};
// the row form, one unit per mode (inst_grouped_plain.hip, _glu.hip, _weighted.hip: H = silu32(gate) * up over rows read through an
// optional index; Y = row_weight * (X @ W^T) with the rows past offsets[E] written as zeros)
int qgemm_grouped_plain_unit(const GroupedForward& g, hipStream_t stream);
int qgemm_grouped_glu_unit(const GroupedForward& g, hipStream_t stream);
int qgemm_grouped_weighted_unit(const GroupedForward& g, hipStream_t stream);
// the block form of the plain and weighted modes for experts with many rows (what it serves: grouped_blocks_eligible, grouped_rows.h;
// inst_grouped_blocks_b*.hip, one unit per bit width); the grid follows from (E, R, N) alone
int qgemm_grouped_blocks_unit_b4(const GroupedForward& g, hipStream_t stream);
int qgemm_grouped_blocks_unit_b2(const GroupedForward& g, hipStream_t stream);
// the block form of the Glu mode (flute_qgemm_grouped_glu_blocks; what it serves: grouped_glu_blocks_eligible, grouped_rows.h;
// inst_grouped_glu_blocks_b*.hip): the same grid from (E, R, F) alone.  Its own entry: qgemm_grouped_dispatch never takes it.
int qgemm_grouped_glu_blocks_unit_b4(const GroupedForward& g, hipStream_t stream);
int qgemm_grouped_glu_blocks_unit_b2(const GroupedForward& g, hipStream_t stream);
// the unit of a launch: the one ladder over form, bit width and mode
inline int qgemm_grouped_dispatch(const GroupedForward& g, hipStream_t stream) {
    if (g.form == FLUTE_GROUPED_FORM_BLOCKS)
        return g.num_bits == 4 ? qgemm_grouped_blocks_unit_b4(g, stream) : qgemm_grouped_blocks_unit_b2(g, stream);
    if (g.mode == FLUTE_GROUPED_GLU) return qgemm_grouped_glu_unit(g, stream);
    return g.mode == FLUTE_GROUPED_WEIGHTED ? qgemm_grouped_weighted_unit(g, stream) : qgemm_grouped_plain_unit(g, stream);
}
// One launch of the input gradient of the grouped qgemm: dX [R, K] from dY [R, N]; pair: both products summed in fp32 (the single form
// fills both slots with its one stack); rows past offsets[E] written as zeros
struct GroupedInputGrad {
    int form;                                         // resolved: FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS (qgemm_grouped_input_grad.h) / _BLOCKS (.._blocks.h)
    int dtype, num_bits, tile_p, lg;
    int E, R, N, K, P;
    bool pair;
    const void *dY[2], *offsets;
    const void *Q[2], *S[2], *QM2[2];
    const float* row_weight;                          // [R] or null (single form only)
    void* dX;
};
// the slab form (inst_grouped_input_grad_b*.hip, one unit per bit width) and the block form for experts with many rows (one workgroup
// per 128-row block of an expert x 256 k; what it serves: grouped_input_grad_blocks_eligible; inst_grouped_input_grad_blocks_b*.hip):
// same operands, same bits; either grid follows from the shapes alone
int qgemm_grouped_input_grad_unit_b4(const GroupedInputGrad& g, hipStream_t stream);
int qgemm_grouped_input_grad_unit_b3(const GroupedInputGrad& g, hipStream_t stream);
int qgemm_grouped_input_grad_unit_b2(const GroupedInputGrad& g, hipStream_t stream);
int qgemm_grouped_input_grad_blocks_unit_b4(const GroupedInputGrad& g, hipStream_t stream);
int qgemm_grouped_input_grad_blocks_unit_b2(const GroupedInputGrad& g, hipStream_t stream);
inline int qgemm_grouped_input_grad_dispatch(const GroupedInputGrad& g, hipStream_t stream) {
    if (g.form == FLUTE_GROUPED_INPUT_GRAD_FORM_BLOCKS)
        return g.num_bits == 4 ? qgemm_grouped_input_grad_blocks_unit_b4(g, stream) : qgemm_grouped_input_grad_blocks_unit_b2(g, stream);
    if (g.num_bits == 4) return qgemm_grouped_input_grad_unit_b4(g, stream);
    return g.num_bits == 3 ? qgemm_grouped_input_grad_unit_b3(g, stream) : qgemm_grouped_input_grad_unit_b2(g, stream);
}
// the routing of a mixture-of-experts step (moe_route.hip): a stable counting sort of the P = T k (token, slot) pairs by expert in one
// workgroup, which holds (16 + 1) (E + 1) ints of LDS; ids int32 / int64, weights T / fp32 or null, everything read on the device only
int moe_route_dispatch(int id_dtype, int weight_dtype, int P, int k, int E, const void* ids, const void* weights,
                       int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, hipStream_t stream);
// the gating in front of it (moe_gate.hip): logits [T, E] -> ids [T, k] int32, weights [T, k] fp32, one wave per token; with offsets non-null
// the routed form: one workgroup of 16 waves gates every token and then runs moe_route's counting sort on what it wrote.  groups non-null:
// group-limited selection (n_group groups of E / n_group experts, the topk_group best by group_score allowed); the caller has checked the
// shapes; topk_group == n_group is served by the kernels without the group stage, as groups == null is
struct GateGroups {
    int n_group, topk_group, group_score;
};
int moe_gate_dispatch(int logit_dtype, int T, int E, int k, const GateGroups* groups, int scoring, int renormalize, float scale,
                      const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* offsets, int32_t* perm,
                      int32_t* rows, float* row_weight, int32_t* pos, hipStream_t stream);
// the same routing over many workgroups (moe_route_wide.hip): chunks of chunk_tokens tokens, C = ceil(T / chunk_tokens) > 1 of them, in
// three launches - count (gated: moe_gate_count_dispatch, moe_gate.hip, which gates each chunk's tokens first), scan, place; workspace:
// (C + 1) (E + 1) int32, every word the later launches read written by the earlier ones.  The caller has checked shapes and sizes.
int moe_route_wide_dispatch(int id_dtype, int weight_dtype, int T, int k, int E, int chunk_tokens, const void* ids,
                            const void* weights, int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos,
                            void* workspace, hipStream_t stream);
int moe_gate_route_wide_dispatch(int logit_dtype, int T, int E, int k, const GateGroups* groups, int scoring, int renormalize,
                                 float scale, int chunk_tokens, const void* logits, const float* bias, int32_t* ids, float* weights,
                                 int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* workspace,
                                 hipStream_t stream);
int moe_gate_count_dispatch(int logit_dtype, int T, int E, int k, const GateGroups* groups, int scoring, int renormalize, float scale,
                            int chunk_tokens, const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* hist,
                            hipStream_t stream);
// its end (moe_combine.hip): out[t] = round_T(fp32 sum over the slots of Y[pos[t, j]]), positions outside [0, clamp(offsets[E])) skipped;
// the grid is tokens x chunks of 1024 columns (0: it does not fit)
unsigned moe_combine_grid(int T, int N);
int moe_combine_dispatch(int dtype, int T, int k, int E, int N, const void* Y, const int32_t* pos, const int32_t* offsets,
                         void* out, hipStream_t stream);
// the two streams of the fused SwiGLU launch's backward (swiglu_grad.hip): dg, du [R, F] from g, u, dh in fp32 (flute_swiglu_grad's
// formula) and out[r] = X[clamp(rows[r])], a copy; offsets null: every row served, else the rows from clamp(offsets[E]) on are zeros
// and nothing of theirs is read.  One grid rule for both: rows x chunks of 1024 columns (0: it does not fit)
unsigned row_stream_grid(int R, int width);
int swiglu_grad_dispatch(int dtype, int R, int F, int E, const void* g, const void* u, const void* dh, const int32_t* offsets,
                         void* dg, void* du, hipStream_t stream);
int moe_gather_dispatch(int R, int Tsrc, int K, int E, const void* X, const int32_t* rows, const int32_t* offsets, void* out,
                        hipStream_t stream);
// the router's backward (router_grad.hip): d_row_weight [R] fp32 = the row sums of dHp * H and dH = round_T(row_weight dHp) in one
// launch, one workgroup of 256 lanes per row (dH and row_weight null together: the sums only; offsets as swiglu_grad's); and the
// gate's backward, d_logits [T, E] from the gradients of its weights [T, k] and / or of row_weight through pos, one wave per token
int moe_weight_grad_dispatch(int dtype, int R, int K, int E, const void* dHp, const void* H, const float* row_weight,
                             const int32_t* offsets, float* d_row_weight, void* dH, hipStream_t stream);
int moe_gate_grad_dispatch(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale, const void* logits,
                           const int32_t* ids, const float* d_weights, const float* d_row_weight, const int32_t* pos,
                           void* d_logits, hipStream_t stream);
// the router's auxiliary losses (moe_aux.hip): partials per chunk of chunk_tokens tokens into the workspace - psum [C][E] fp32, pcnt
// [C][E] int32, pz [C] fp32, every word written - then one workgroup that sums the chunks in ascending order in fp64 into load [E],
// importance [E] and losses [2] = (balance, z); and their backward, d_logits [T, E] from load and grads [2] on the device, one wave
// per token.  The caller has checked shapes and sizes.
int moe_aux_loss_dispatch(int logit_dtype, int T, int E, int k, int scoring, int chunk_tokens, const void* logits,
                          const int32_t* ids, void* workspace, int32_t* load, float* importance, float* losses, hipStream_t stream);
int moe_aux_loss_grad_dispatch(int logit_dtype, int T, int E, int scoring, const void* logits, const int32_t* load,
                               const float* grads, void* d_logits, hipStream_t stream);
int stream_read_dispatch(const void* src, void* sink, size_t bytes, int bytes_per_wave, int grid,
                         int block, hipStream_t stream);
int timestamp_dispatch(void* dst, hipStream_t stream);
int splitk_reduce_dispatch(int dtype, const float* partial, void* D, size_t mn, int splitk,
                           hipStream_t stream);

}  // namespace flute_amd
