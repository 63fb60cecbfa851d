/* flute_amd C ABI - the drop-in boundary of the MI355X (gfx950) qgemm path.
 *
 * Plain pointers and sizes only (no torch types).  Every entry point is what a
 * binding for the reference's hot path would call; the reference interface it
 * replaces is cited on each declaration (paths relative to HanGuo97/flute
 * v0.4.2).  All functions return 0 on success or a negative flute_status;
 * flute_strerror() maps a status to the message prefix the reference raises
 * (the reference's tuner string-matches those, flute/tune.py:160-167).
 *
 * Device pointers must be valid on the current HIP device, contiguous and 16-B
 * aligned (torch allocations are).  A contiguous torch VIEW need not be (buf[1:1 + n]
 * is 2 bytes off): the Python entry points (flute_amd/ops.py) and the torch binding
 * (csrc/torch_binding.cpp) realign such views - a fresh copy - before they pass a
 * pointer; a caller of this C ABI does that itself.  Nothing here allocates, synchronises or
 * touches the host after enqueue: every call is stream-ordered on `stream`
 * (a hipStream_t) and hipGraph-capturable, like the reference's launch on
 * at::cuda::getCurrentCUDAStream() (flute/csrc/qgemm.cpp:101-105).
 */
#ifndef FLUTE_AMD_H
#define FLUTE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9: flute_dequantize; flute_qgemm_scale_grad; flute_qgemm_table_grad and its scratch query; flute_qgemm_grouped;
 *    flute_qgemm_grouped_glu and flute_qgemm_grouped_weighted; flute_moe_route and flute_moe_combine with FLUTE_F32 / flute_index_dtype;
 *    flute_moe_gate and flute_moe_gate_route with flute_gate_scoring; flute_moe_gate_limited and flute_moe_gate_route_limited with
 *    flute_gate_group_score; flute_qgemm_grouped_input_grad and flute_qgemm_grouped_input_grad_row_block;
 *    flute_qgemm_grouped_scale_grad; flute_qgemm_grouped_table_grad and its scratch query;
 *    the block form of the grouped forward launches: flute_qgemm_grouped_ex, flute_qgemm_grouped_glu_ex, flute_qgemm_grouped_weighted_ex
 *    (the old entries with a trailing `form`), flute_qgemm_grouped_form, flute_grouped_form_t, flute_grouped_mode_t;
 *    the block form of the grouped input gradient: flute_qgemm_grouped_input_grad_ex (the old entry with a trailing `form`),
 *    flute_qgemm_grouped_input_grad_form, flute_grouped_input_grad_form_t;
 *    the block form of the fused SwiGLU launch behind its own entry: flute_qgemm_grouped_glu_blocks, flute_qgemm_grouped_glu_blocks_form
 *    the two streams of the fused SwiGLU launch's backward: flute_swiglu_grad, flute_moe_gather
 *    the router's backward: flute_moe_weight_grad, flute_moe_gate_grad
 *    the routing over many workgroups: flute_moe_route_wide, flute_moe_gate_route_wide, flute_moe_route_wide_workspace, flute_moe_route_form
 *    the router's auxiliary losses: flute_moe_aux_loss, flute_moe_aux_loss_grad, flute_moe_aux_loss_workspace
 *    (additive: no existing entry point changed its signature or its refusals, so the number stays)
 * 8 (round 6, late): same structs; family 8 = persistent MFMA decode kernel (qgemm_persistm.h) in flute_plan.family / flute_overrides.family -
 *    slabs_per_wave = column groups per set (1 .. 3), visits = sets per workgroup (override: m_tiles), k_chunks = activation requests per macro-step
 * 7 (round 6): same structs; flute_plan.kw / m_block of family 6 = K parts per workgroup (2 / 4) / row tiles per XCD group, flute_plan.slabs_per_wave
 *    of family 7 = column groups per workgroup (1 .. 3), and the overrides of the same names select them; family 6 refuses waves = 8
 * 6 (round 5): flute_plan.one_shot / flute_overrides.one_shot value 4 (lean decode kernel, qgemm_fast.h), flute_debug_timestamp */
#define FLUTE_AMD_ABI_VERSION 9

/* FLUTE_F32: the routing weights of flute_moe_route and the router logits of flute_moe_gate / flute_moe_gate_route only; every
 * other entry point refuses it (FLUTE_ERR_DTYPE) */
enum flute_dtype { FLUTE_F16 = 0, FLUTE_BF16 = 1, FLUTE_F32 = 2 };
/* the width of flute_moe_route's expert ids */
enum flute_index_dtype { FLUTE_I32 = 0, FLUTE_I64 = 1 };
/* how flute_moe_gate / flute_moe_gate_route turn a router logit into a score */
enum flute_gate_scoring { FLUTE_GATE_SOFTMAX = 0, FLUTE_GATE_SIGMOID = 1 };
/* how flute_moe_gate_limited / flute_moe_gate_route_limited rank a group of experts: by its largest key (DeepSeek-V2), or by the sum
 * of its two largest biased scores (DeepSeek-V3) */
enum flute_gate_group_score { FLUTE_GATE_GROUP_MAX = 0, FLUTE_GATE_GROUP_TOP2SUM = 1 };

enum flute_status {
    FLUTE_OK = 0,
    FLUTE_ERR_NUM_BITS = -1,      /* "Unsupported num_bits value"    qgemm.cpp:171 */
    FLUTE_ERR_GROUP_SIZE = -2,    /* "Unsupported group_size value"  qgemm.cpp:153 */
    FLUTE_ERR_TEMPLATE_ID = -3,   /* "Unsupported template_id value" qgemm_kernel_raw_generated.cu:205 */
    FLUTE_ERR_SHAPE = -4,         /* shape / divisibility precondition (ops.py:40-49) */
    FLUTE_ERR_WORKSPACE = -5,     /* split-K needs more workspace than given */
    FLUTE_ERR_LAUNCH = -6,        /* HIP launch failed: message starts "CUDA error: invalid argument" (tune.py:160) */
    FLUTE_ERR_DTYPE = -7,
    FLUTE_ERR_HADAMARD_SIZE = -8, /* hadamard_transform.cpp:23-25 */
    FLUTE_ERR_NULL = -9
};

/* One row of the gfx950 template table.  Same fields as the reference's
 * TEMPLATE_CONFIGS entries (flute/codegen_utils.py:110-152,
 * data/qgemm_kernel_raw_generated_configs.pth) and the same id -> TileP map, so
 * weights packed by the reference for template id X decode correctly here under
 * the same id.  Meaning of the knobs on gfx950:
 *   sms_multiple  decode: weight-ring depth (1: 4 pieces, 2/4: 2 pieces in flight per wave); MFMA kernel:
 *                 more, smaller workgroups
 *   threads       upper bound of the decode kernel's workgroup size (1024 / 512); MFMA kernel: 8 / 4 waves
 *   tile_m        rows per wave of the MFMA kernel (16/32/64)
 *   tile_k        64 (granularity of K)
 *   tile_p        packed-layout parameter (32/64) - fixes the wire format
 *   stages        decode: which of the planner's ranked (waves, K split) shapes to launch (2 = best,
 *                 3/4/5 = the next ones); MFMA kernel: the neighbouring in-workgroup K splits
 *   lut_copies    the reference's QuantMapMode slot (1/32/16/8): MFMA kernel, 4-bit: automatic / no lane sharing
 *                 above M = 16 (the grid K split fills the chip instead) / one / two slabs per wave (above M = 16 the
 *                 last one also means no lane sharing: two slabs per wave x the grid K split).  The kernels
 *                 always replicate the pair table 32x in LDS.
 * The decode kernel applies the group scale in fp32 to an 8-k partial sum: exact on
 * one-hot inputs, within 2^-11 relative per term of the reference's round_T(lut * s) otherwise. */
typedef struct flute_template_info {
    int num_bits, template_id;
    int sms_multiple, threads, tile_m, tile_k, tile_p, stages, lut_copies;
} flute_template_info;

/* Launch plan chosen for a problem (host logic only, no GPU needed). */
typedef struct flute_plan {
    int family;          /* 0 = decode (GEMV kernels, M<=4; 3 bits: M<=2; see one_shot), 2 = MFMA kernel with
                            LDS-DMA staged operands (every larger M), 3 = block-tiled prefill kernel
                            (enough 128 / 256 x 256 output blocks to fill the chip; 3-bit layers from M = 65 also 128- or
                            64-row blocks x splitk K slices - m_block 5 / 12; 128-row blocks x 2 / 4 slices meet inside the launch (splitk_mode 1), the others through fp32 slabs + the reduce pass), 5 = skinny MFMA kernel
                            (qgemm_skinny.h: 4-bit, 3 <= M <= 16, K = 32 x ring_depth x waves, layers whose 64-column
                            slabs fill 55..100 % of the CUs; weights and activations straight to registers),
                            6 = split-K block kernel (qgemm_splitk.h: 2- / 4-bit, m_tiles x 16 rows (128 or 64) x 256 / kw columns
                            (128; 64 with kw = 4 K parts per workgroup, 64-row tiles only - round 6) output tiles x splitk K slices,
                            one workgroup of 8 compute + 4 loader waves each, partial tiles combined inside the launch; automatic
                            from M = 33 (2 and 4 bits) where its modelled time is 8 % under the other MFMA kernels' (64-column
                            tiles that fill half the chip: under the per-wave kernel's time + 4 us) and one round of workgroups
                            covers the output (2-bit layers up to M = 64: two rounds),
                            7 = lean MFMA decode kernel (qgemm_fastm.h, round 5: 4 bits, 5 <= M <= 16, K in {2048, 4096}, a
                            workgroup = 4 unit rows x all of K, N / 16 workgroups of 8 waves between half a round and one
                            round of the CUs, 32 KB + 32 copies x 4 KB of LDS = 160 KB; what it cannot take falls back),
                            8 = persistent MFMA decode kernel (qgemm_persistm.h, round 6: 4 or 2 bits, 3 <= M <= 16, K % 128 == 0, group size
                            64 / 128; `grid` workgroups of 8 waves stream `visits` sets of slabs_per_wave column groups (16 columns each) x
                            all of K, k_chunks = 1 / 2 / 4 activation requests per 128-k macro-step for M <= 4 / 8 / 16; automatic under the
                            ids that leave the choice to the planner for layers above 16 M weights with K >= 6144, K >= 3584 at M <= 8 or
                            where K is neither 2048 nor 4096) */
    int m_block;         /* decode: rows per pass (1/2/4); family 2: R (lanes sharing a unit); family 3: block shape
                            (4 / 5: 256- / 128-row blocks; 8 + rt: 3-bit blocks of rt = 1, 2, 4 row tiles); family 6: row tiles of a
                            column tile that run as consecutive blocks of ONE XCD when K is not split (1 = natural order, 2, 4, 8);
                            families 7, 8: 16 */
    int m_tiles;         /* family 2: 16-row tiles per wave (1/2/4); family 6: row tiles per output tile (8 / 4) */
    int slabs_per_wave;  /* family 2: 16-unit column slabs per wave (1/2); family 7: column groups per workgroup; family 8: per set (1 .. 3) */
    int waves;           /* waves per workgroup (decode: any count up to 16, not only powers of two) */
    int kw;              /* waves of a workgroup sharing one unit (in-workgroup K split); family 6: K parts per workgroup (2 / 4) */
    int splitk;          /* grid-level K split (fp32 slabs in the workspace; see splitk_mode) */
    int k_per_split;
    int lut_copies;
    unsigned grid, block;
    size_t lds_bytes;
    size_t workspace_needed;
    int ring_depth;      /* decode: 1-KiB weight pieces in flight per wave (ring kernel 2/4; one-shot kernels: pieces per wave
                            4/8, 3 bits 2/4; persistent one-shot kernel: pieces per segment); skinny MFMA kernel: k-steps per wave */
    int visits;          /* decode: unit groups the busiest workgroup streams; family 8: sets the busiest workgroup streams */
    int k_chunks;        /* decode: passes over K when the activations do not fit in LDS at once; family 8: activation requests per macro-step */
    int one_shot;        /* family 8: 1 = the activations resident in LDS (4 k_chunks rows x K within 64 KB), 0 = through the wave-private rings;
                            decode: 0 = persistent ring kernel (qgemm_stream.h); 1 = one-shot kernel (qgemm_oneshot.h:
                            non-persistent workgroups, every request issued by the prologue, ring_depth = pieces per
                            wave), 2 = the same with the software-pipelined piece loop, 3 = persistent one-shot kernel
                            (qgemm_persist.h: table / activations staged once, every wave walks `visits` units of
                            `k_chunks` segments of ring_depth pieces, the next segment requested ahead), 4 = lean decode
                            kernel (qgemm_fast.h, round 5: 4 bits, M <= 4, K = 512 * ring_depth * kw in {2048, 3584, 4096, 8192}
                            a compile-time constant, m_block rows per pass) */
    int splitk_mode;     /* splitk > 1: 0 = fp32 slabs in the workspace + a second (reduce) launch, 1 = combined inside the
                            launch (csrc/xwg.h: write-through slabs + one arrival word per output tile) */
} flute_plan;

/* Per-call launch-plan overrides for the offline tuner, the sweeps and the tests; every field -1 (or a
 * NULL pointer) = automatic.  Plain data passed with the call: there is no process-global tuning state.
 *   family          5 skinny MFMA kernel (4-bit, M <= 16; waves 4 / 8 picks the in-workgroup K split);
 *                   6 split-K block kernel (splitk picks the K slices per tile; 1 = none; m_tiles 8 / 4: 128- / 64-row
 *                   tiles; kw 2 / 4: K parts per workgroup = 128- / 64-column tiles (4 with 64-row tiles only); m_block 1 / 2 / 4 / 8:
 *                   row tiles per XCD group of the block order; waves must be 12 or automatic - the variant without loader
 *                   waves was dropped in round 6);
 *                   7 lean MFMA decode kernel (4 bits, 5 <= M <= 16, K in {2048, 4096}; falls back where it does not apply);
 *                   8 persistent MFMA decode kernel (4 / 2 bits, M <= 16, K % 128 == 0, K >= 1024, group size 64 / 128; slabs_per_wave 1 .. 3:
 *                   column groups per set, m_tiles: sets per workgroup, one_shot 0: activation rings also where the activations could be resident;
 *                   refused - FLUTE_ERR_SHAPE - where it does not apply);
 *                   0 decode kernels also at M = 3, 4 (2- / 4-bit; automatic: M <= 2, and M <= 4 for
 *                   small layers called with a Hadamard size, to keep the rotation fused), 1 / 2 per-wave MFMA
 *                   kernel, 3 block-tiled prefill kernel (m_tiles 8 / 4: 256 / 128-row block); 4 and > 8 are rejected
 *                   (FLUTE_ERR_SHAPE).  m_tiles / waves / kw / splitk / slabs_per_wave given WITHOUT family = 6 belong to the
 *                   per-wave kernel: such a call never takes the split-K block kernel automatically
 *   m_block         decode: rows per pass; MFMA: R (lanes sharing a unit)
 *   waves, kw       waves per workgroup / in-workgroup K split
 *   splitk          grid-level K split
 *   m_tiles, slabs_per_wave   MFMA kernel: 16-row tiles per wave (1/2/4), column slabs per wave (1/2)
 *   ring_depth      decode: pieces in flight per wave (ring kernel 2/4; one-shot kernel 4/8, 3-bit 2/4); without
 *                   one_shot = 1 a given depth selects the ring kernel
 *   one_shot        decode: 1 one-shot kernel, 0 persistent ring kernel, 3 persistent one-shot kernel (M <= 2) - the code
 *                   flute_plan.one_shot reports for it; 2, ABI v4's value for the same request, is still accepted; 4 lean decode
 *                   kernel (4 bits, M <= 4, K in {2048, 3584, 4096, 8192}; `waves` 4 / 8 picks its shape; what it cannot take falls back) */
typedef struct flute_overrides {
    int family, m_block, waves, kw, splitk, m_tiles, slabs_per_wave, ring_depth, one_shot;
} flute_overrides;

/* D[M,N] = A[M,K] @ (table2-lookup(Q) * S)   fused LUT-dequant GEMM.
 * Replaces _qgemm_raw<T,TQ,T2,NumBits,GroupSize>  (flute/csrc/qgemm.cpp:15-36,
 * body flute/csrc/qgemm_kernel_raw_generated.cu:15-768 -> qgemm_host,
 * qgemm_kernel.hpp:824-939).
 *   A  [M,K] T row-major          Q  [P,K] int16, P = num_bits*N/16 (flute/utils.py:59-253)
 *   S  [N,K/group_size] T         QM [2^b] T (unused by the kernel, as in the reference)
 *   QM2 [2^b,2^b] pairs of T in one 32-bit word (flute/utils.py:15-33)
 *   workspace: caller-owned scratch, used for split-K slabs; may be NULL when
 *   the plan has splitk == 1 (flute/utils.py:36-56 over-allocates it).
 * Arithmetic, every family: w^ = round_T(lut * s) or the scale applied in fp32 to an fp32 partial sum; fp32
 * accumulation; one IEEE round-to-nearest-even of the output.  No exception at the edges of T (measured on gfx950,
 * tests/test_value_edges_gpu.py): fp16 subnormal weights and activations are multiplied as they are (neither the packed
 * dot instructions nor the matrix unit flush them), a result beyond the largest finite T is +-inf (no saturation), a
 * subnormal result is rounded correctly.  A NaN or Inf in A propagates through its own row only, by IEEE rules (Inf
 * times a zero weight is NaN).  Nothing outside an operand's extent reaches a result, whatever lies next to it in
 * memory.  QM2 (and QM) must hold finite values: a table entry of Inf or NaN is not a supported input (the bf16
 * block kernels form lo * s + hi * 0 per packed table word). */
int flute_qgemm(int dtype, int num_bits, int group_size, int M, int N, int K, int P,
                const void* A, const void* Q, void* D, const void* S, const void* QM,
                const void* QM2, void* workspace, size_t workspace_bytes, int template_id,
                int num_sms, void* stream);

/* flute.qgemm_hadamard (flute/__init__.py:32-50; apply_hadamard + qgemm_raw_simple_hadamard,
 * flute/csrc/qgemm.cpp:201-244): D = (A.reshape(-1, hadamard_size) @ H/sqrt(hadamard_size)).reshape(M,K)
 * @ dequant(Q).  When the launch plan is a decode kernel, hadamard_size <= 512 divides K and M * K <= 8192 elements
 * (every workgroup rotates all M rows for itself: beyond that a separate flute_hadamard launch is cheaper - measured),
 * the rotation is fused into that kernel's activation staging (one launch, no round trip of the
 * rotated activations through HBM; same fp32 butterflies and single rounding as flute_hadamard, so the
 * result is bit-identical to the two-launch form).  Otherwise the rotated activations go to
 * x_scratch ([M,K] T, caller-owned) with flute_hadamard and the plain product follows.
 * flute_qgemm_hadamard_fused returns 1 when x_scratch will not be touched (may then be NULL). */
int flute_qgemm_hadamard(int dtype, int num_bits, int group_size, int hadamard_size, int M, int N,
                         int K, int P, const void* A, const void* Q, void* D, const void* S,
                         const void* QM, const void* QM2, void* x_scratch, void* workspace,
                         size_t workspace_bytes, int template_id, int num_sms, void* stream);
int flute_qgemm_hadamard_fused(int dtype, int num_bits, int group_size, int hadamard_size, int M,
                               int N, int K, int template_id, int num_sms, size_t workspace_bytes);

/* flute_qgemm_hadamard with a per-call plan override (ovr may be NULL): what the offline tuner and the
 * development sweeps call.  hadamard_size 0 = plain flute_qgemm. */
int flute_qgemm_ex(int dtype, int num_bits, int group_size, int hadamard_size, int M, int N, int K, int P,
                   const void* A, const void* Q, void* D, const void* S, const void* QM,
                   const void* QM2, void* x_scratch, void* workspace, size_t workspace_bytes,
                   int template_id, int num_sms, const flute_overrides* ovr, void* stream);

/* The plan flute_qgemm would use (exposed for tests and the offline tuner).  A plan is resolved to its kernel when it is made:
 * FLUTE_OK here (and 1 from flute_qgemm_hadamard_fused) means a kernel that is built, and a shape no kernel is instantiated for
 * is FLUTE_ERR_TEMPLATE_ID here as in flute_qgemm - no GPU needed.  (One exception, kept as it was: the override m_block = 3 of
 * the per-wave MFMA kernel plans, and the launch refuses it with FLUTE_ERR_TEMPLATE_ID.) */
int flute_qgemm_plan(int dtype, int num_bits, int group_size, int M, int N, int K,
                     int template_id, int num_sms, size_t workspace_bytes, flute_plan* out);
int flute_qgemm_plan_ex(int dtype, int num_bits, int group_size, int M, int N, int K,
                        int template_id, int num_sms, size_t workspace_bytes,
                        const flute_overrides* ovr, flute_plan* out);

/* out = in.reshape(-1, had_size) @ (H/sqrt(had_size)), Sylvester order.
 * Replaces run_fht<dtype>(a, out, numel, had_size, stream)
 * (flute/csrc/hadamard_transform_cuda.cu:701-748; wrapper hadamard_transform.cpp:17-56;
 * used by apply_hadamard, qgemm.cpp:201-211).  in == out is allowed. */
int flute_hadamard(int dtype, const void* in, void* out, size_t numel, uint32_t had_size,
                   void* stream);

/* Q[P,K] -> integer codes W[K,N] uint8 on the device.  Native replacement for
 * flute.utils.unpack, which runs qgemm on an identity matrix
 * (flute/utils.py:347-407). */
int flute_unpack(int num_bits, int template_id, int N, int K, const void* Q, void* W,
                 void* stream);

/* The dense dequantized weight W[N, k_count] (row-major T, the nn.Linear weight layout) of columns
 * [k_begin, k_begin + k_count) of K: W[n, k - k_begin] = round_T(QM2-pair-lookup(Q)[k, n] * S[n, k / group_size]),
 * the lookup and the one rounding of the qgemm kernels, so W equals qgemm(identity) element by element.  QM is not
 * read (HIGGS pair codebooks dequantize as they multiply).  k_begin and k_count are multiples of 64 and group_size
 * divides K; k_count == 0 is a no-op.  The product is rounded as IEEE rounds it: an fp16 subnormal lut * s is kept (no
 * flush) and a product beyond the largest finite T is +-inf, not 65504 (tests/test_grad_edges_gpu.py).  Same layer checks as flute_qgemm; FLUTE_ERR_SHAPE also for a bad k range or
 * P != num_bits * N / 16.  Null pointers are refused (FLUTE_ERR_NULL) before anything else. */
int flute_dequantize(int dtype, int num_bits, int group_size, int N, int K, int P, int k_begin, int k_count,
                     const void* Q, const void* S, const void* QM2, void* W, int template_id, void* stream);

/* The gradient of a layer's scales, dS[n, j] = round_T(sum_{m < M} sum_{j*g <= k < (j+1)*g} dY[m, n] * X[m, k] * L[k, n]),
 * L[k, n] the value the qgemm kernels multiply by the scale (the QM2 pair lookup of Q, as flute_dequantize; QM is not
 * read).  dY [M, N] and X [M, K] row-major T, dS [N, K / group_size] T: fp32 products and sums, one rounding to T.  X is
 * the activation the weight multiplies (for a Hadamard layer the rotated input).  Non-finite inputs propagate by IEEE
 * rules to exactly the outputs the formula connects them to: a NaN or Inf at X[m, k] reaches dS[:, k / group_size] only, one
 * at dY[m, n] reaches dS[n, :] only (Inf: +-inf by the signs of the factors it meets, NaN where one is zero or both signs
 * meet), split or unsplit; rows past M are not loaded, never multiplied by zero.  Subnormal dY and X are multiplied as
 * they are and dS rounds to +-inf, not to 65504 (tests/test_grad_edges_gpu.py).  M >= 1; group_size in {32, 64, 128,
 * 256}; same layer checks as flute_dequantize, in its order (FLUTE_ERR_NULL for a null dY / X / Q / QM2 / dS first).
 * `scratch` (scratch_bytes, may be null / 0) lets small layers split M across workgroups: fp32 partials
 * [splits][N][K / group_size] summed in split order by a second launch.  The number of splits follows from M, N, K,
 * num_sms (< 1: 256) and scratch_bytes alone, so equal arguments give equal bits; too little scratch only means fewer
 * splits, never an error.  Do not pass the qgemm workspace (its leading state words must stay zero). */
int flute_qgemm_scale_grad(int dtype, int num_bits, int group_size, int M, int N, int K, int P, int template_id,
                           const void* dY, const void* X, const void* Q, const void* QM2, void* dS,
                           void* scratch, size_t scratch_bytes, int num_sms, void* stream);

/* The gradient of a layer's lookup table with the codes fixed, for the pair codebook the kernels read:
 *   dT2[c][e] = sum over (kappa, n) whose pair index code(2 kappa) << b | code(2 kappa + 1) is c of
 *               G[2 kappa + e][n] * S[n][2 kappa / group_size],   G[k][n] = sum_{m < M} X[m][k] * dY[m][n],
 * dT2 [4^b][2] fp32 (e = 0: the low half of the 32-bit pair word), written whole.  For a scalar table the caller folds
 * it: dtable[i] = sum_j dT2[i 2^b + j][0] + sum_j dT2[j 2^b + i][1].  dY, X, Q as flute_qgemm_scale_grad; S [N, K /
 * group_size] T.  The table is not read.  With dS non-null the same launch also writes the scale gradient, bit for bit
 * what flute_qgemm_scale_grad returns for the same layer and M given its full scratch (what
 * flute_amd.qgemm_scale_grad passes); QM2 is needed then and only then.  fp32 products and sums inside a workgroup, fp64
 * across workgroups, one rounding to fp32; no atomics on global memory: equal arguments give equal bits.
 * Non-finite inputs propagate by IEEE rules to exactly the bins the formula connects them to: a NaN or Inf at X[m, k]
 * reaches the bins (c, e = k & 1) whose pair index occurs at pair row k >> 1, one at dY[m, n] the bins of column n's pairs;
 * every other bin keeps its bits.  dS follows flute_qgemm_scale_grad's rule and rounds to +-inf, not to 65504.
 * Refusals in flute_qgemm_scale_grad's order: FLUTE_ERR_NULL first (dY / X / Q / S / dT2 / scratch, QM2 with a dS),
 * then dtype, the layer checks, P and M.  `scratch` must hold flute_qgemm_table_grad_scratch_bytes(...) bytes for the
 * same num_bits, group_size, M, N, K, num_sms and want_dS = (dS != NULL): less is FLUTE_ERR_WORKSPACE (more changes
 * nothing).  The query takes no template_id: it is 0 for a num_bits / group_size / shape no template accepts (N % 128,
 * K % max(64, group_size), M < 1) and may be non-zero for arguments one template's own checks still refuse.  Everything
 * is refused before anything is enqueued. */
int flute_qgemm_table_grad(int dtype, int num_bits, int group_size, int M, int N, int K, int P, int template_id,
                           const void* dY, const void* X, const void* Q, const void* S, const void* QM2, float* dT2,
                           void* dS, void* scratch, size_t scratch_bytes, int num_sms, void* stream);
size_t flute_qgemm_table_grad_scratch_bytes(int num_bits, int group_size, int M, int N, int K, int want_dS,
                                            int num_sms);

/* Grouped qgemm for mixture-of-experts layers: Y[r, :] = X[r, :] @ W_e^T for every row r in [offsets[e], offsets[e + 1]),
 * e = 0 .. E - 1, in ONE launch.  X [T, K] T holds the rows sorted by expert; offsets [E + 1] int32 in DEVICE memory,
 * offsets[0] = 0, non-decreasing, offsets[E] = T; Q [E, P, K] int16, S [E, N, K / group_size] T and QM2 [E, 2^b, 2^b] pair
 * words are E layers packed exactly as flute_qgemm takes one (one num_bits, group_size and template_id for all); Y [T, N] T.
 * Arithmetic as flute_dequantize and the MFMA kernels: w^ = round_T(QM2-pair-lookup * scale), fp32 accumulation in the
 * matrix core, one rounding of the output.  K is split among the waves of one workgroup only and combined through LDS
 * in a fixed order (no atomics, no split across workgroups): equal arguments give equal bits.
 * Non-finite inputs propagate by IEEE rules to exactly the outputs the formula connects them to: a NaN or Inf in row r of X
 * reaches row r of Y only (Inf: +-inf by the sign of the weight it meets, NaN at a zero weight), whichever expert's rows
 * share its 16-row tile - rows outside an expert's range are not loaded, never multiplied by zero.  fp16 subnormal
 * weights and activations are multiplied as they are, and Y rounds to +-inf, not to 65504 (tests/test_grouped_edges_gpu.py).
 * The host never reads `offsets`: the grid follows from (E, N, num_bits, num_sms) alone, so
 * the launch can be captured in a hipGraph and a replay serves whatever the table then holds.  A workgroup whose expert
 * has no rows requests nothing.  Every row index is clamped to [0, T]: a malformed table cannot read or write outside
 * X / Y; rows no expert covers are left unwritten, rows that overlapping ranges name twice have unspecified contents.
 * Two forms serve the launch (flute_qgemm_grouped_ex chooses; this entry is the automatic choice).  The ROW form is the one
 * described so far: experts with many rows stream their weights once per pass of 32 rows (3 bits: 16) - correct for any
 * count, the fast one for decode-sized counts.  The BLOCK form serves prefill and training counts: 128-row x 256-column
 * blocks of the dense prefill kernel, a weight dequantised once per 128 rows, all of K in one fp32 accumulator of the
 * matrix core (no K split at all), one rounding; equal arguments give equal bits.  Its bits may differ from the row form's,
 * whose summation order differs, except on exactly representable inputs.  Its grid follows from (E, T, N, num_bits)
 * alone - floor((T + 127 E) / 128) row blocks, the most a table over T rows can own, times N / 256 - never from
 * `offsets`: capture and replay on another table of the same T hold as for the row form.  A block past the table's total
 * requests nothing.  In the block form the rows of a block past its expert's end are read as zeros through the bounds of
 * the activation descriptor (no address outside the expert's rows is formed) and are never stored, whatever the weights
 * hold: a NaN or Inf in row r still reaches row r of Y only.  A malformed table stays memory-safe in both forms; in the
 * block form a table whose clamped ranges own more blocks than the grid holds (decreasing entries can) leaves the rows of
 * the blocks past the grid unwritten, and rows that overlapping ranges name twice have unspecified contents.
 * The block form serves: num_bits 4 / 2, (K / group_size) % 8 == 0, N a multiple of 256, (T + 256) * K * 2 and one expert's
 * scale bytes N * (K / group_size) * 2 below 2^32 - 16, the plain and weighted launches.  The automatic rule takes it where
 * it is eligible and the mean rows per expert, T / E, is at least FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS - or
 * FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS_PARTIAL where E * (N / 256) is below num_sms - (measured: csrc/api_train.hip);
 * below that the launch is the row form's, grid included.  flute_qgemm_grouped_glu has no block form: it runs the row form at every count
 * (the block form of that launch is an entry of its own, flute_qgemm_grouped_glu_blocks).
 * Refusals, before anything is enqueued: FLUTE_ERR_DTYPE, then the layer checks of flute_dequantize (num_bits 2 / 3 / 4,
 * group_size 32 / 64 / 128 / 256, the template id - 3 bits: TileP 32 only -, N a multiple of the template's column block,
 * K % max(64, group_size) == 0), FLUTE_ERR_SHAPE for P != num_bits * N / 16 or a negative E / T; E == 0 or T == 0 returns
 * FLUTE_OK without a launch; then FLUTE_ERR_NULL for a null pointer.  num_sms < 1: 256. */
int flute_qgemm_grouped(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P, int template_id,
                        const void* X, const void* offsets, const void* Q, const void* S, const void* QM2,
                        void* Y, int num_sms, void* stream);

/* The form of a grouped forward launch, and the three launches as flute_qgemm_grouped_form names them. */
typedef enum { FLUTE_GROUPED_FORM_AUTO = 0, FLUTE_GROUPED_FORM_ROWS = 1, FLUTE_GROUPED_FORM_BLOCKS = 2 } flute_grouped_form_t;
typedef enum { FLUTE_GROUPED_PLAIN = 0, FLUTE_GROUPED_GLU = 1, FLUTE_GROUPED_WEIGHTED = 2 } flute_grouped_mode_t;
#define FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS 32            /* E * (N / 256) >= num_sms: the experts' column blocks fill the chip */
#define FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS_PARTIAL 64    /* fewer workgroups than compute units */

/* flute_qgemm_grouped, flute_qgemm_grouped_glu and flute_qgemm_grouped_weighted with the form chosen by the caller
 * (flute_grouped_form_t; the old entries pass FLUTE_GROUPED_FORM_AUTO).  Everything else is the old entry's.  One more
 * refusal, after the old entry's shape refusals and before E == 0 / T == 0 and the null pointers, so before anything is
 * enqueued or dereferenced: FLUTE_ERR_SHAPE for a form outside the enum, or FLUTE_GROUPED_FORM_BLOCKS where the block form is
 * not eligible (the list above; the GLU launch always, E == 0 or T == 0 included). */
int flute_qgemm_grouped_ex(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P, int template_id,
                           const void* X, const void* offsets, const void* Q, const void* S, const void* QM2,
                           void* Y, int num_sms, void* stream, int form);
int flute_qgemm_grouped_glu_ex(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K, int P,
                               int template_id, const void* Xsrc, const void* rows, const void* offsets, const void* Qgate,
                               const void* Sgate, const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up,
                               void* H, int num_sms, void* stream, int form);
int flute_qgemm_grouped_weighted_ex(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P,
                                    int template_id, const void* X, const void* offsets, const void* Q, const void* S,
                                    const void* QM2, const float* row_weight, void* Y, int num_sms, void* stream, int form);

/* The form the automatic rule takes for a launch: FLUTE_GROUPED_FORM_ROWS or FLUTE_GROUPED_FORM_BLOCKS, or the negative error
 * the launch itself would refuse the shape with (mode outside flute_grouped_mode_t: FLUTE_ERR_SHAPE).  Host only: no pointers,
 * nothing is enqueued.  rows is T (GLU: R), N the stack's output columns (GLU: F); P is taken as num_bits * N / 16. */
int flute_qgemm_grouped_form(int mode, int dtype, int num_bits, int group_size, int E, int rows, int N, int K,
                             int template_id, int num_sms);

/* The gated half of a mixture-of-experts MLP in ONE launch, on flute_qgemm_grouped's kernel geometry:
 *   H[r, :] = round_T( silu32(g) * u ),   g = Xsrc[rows[r], :] @ Wgate_e^T,   u = Xsrc[rows[r], :] @ Wup_e^T
 * for every row r in [offsets[e], offsets[e + 1]), e = 0 .. E - 1.  g and u are the fp32 sums of the matrix core after the
 * K reduction inside the workgroup (w^ = round_T(QM2-pair-lookup * scale) exactly as flute_qgemm_grouped), the product is
 * formed in fp32 and there is ONE rounding to T, at the store; nothing intermediate reaches global memory.
 *   silu32(g) = g / (1 + exp(-g)), evaluated in fp32 as written: expf (within 1 ulp = 2^-23 relative), one correctly
 *   rounded addition and one correctly rounded division (2^-24 each).  An error of the exponential enters the sum 1 + t
 *   scaled by t / (1 + t) < 1, so silu32 is within 2^-23 + 2 * 2^-24 = 2^-22 (to first order) of g / (1 + e^-g) for
 *   every |g| <= 88 (e^88 is finite in fp32; e^-88 vanishes against the 1); with the fp32 product by u (2^-24):
 *   eps_s = 2^-21 bounds the relative error of silu32(g) * u before the store, well below the rounding to T.
 *   Outside that range the form saturates as written: for g >= 18 the sum 1 + exp(-g) is 1 in fp32 and silu32(g) = g
 *   exactly; for g <= -90 exp(-g) is +inf and silu32(g) = -0; neither branch yields a NaN (g e^g / (1 + e^g) would).
 *   Non-finite inputs propagate by IEEE rules to exactly the rows the formula connects them to - every sorted row whose
 *   source row holds the NaN or Inf, in whichever expert: g = +inf gives +inf times u, g = -inf gives -inf / inf = NaN.
 *   H rounds to +-inf, not to 65504.
 * Xsrc [Tsrc, K] T; rows [R] int32 in DEVICE memory or null.  Null: row r of Xsrc is r, and Tsrc must equal R.  Otherwise
 * each entry is clamped to [0, Tsrc) before it forms an address (Tsrc >= 1 then), and the activation load is the only use
 * of it: no gathered copy of Xsrc is needed.  offsets [E + 1] as flute_qgemm_grouped, clamped to [0, R].  Gate and up are
 * two stacks Q [E, P, K] / S [E, F, K / group_size] / QM2 [E, 2^b, 2^b] of one shape, num_bits, group_size and
 * template_id, each with its own tables and scales; H [R, F] T.  A workgroup serves the same column slab of both stacks
 * for the same rows: no atomics, no split across workgroups, equal arguments give equal bits.  The host reads neither
 * offsets nor rows; the grid follows from (E, F, num_bits, num_sms) alone (hipGraph-capturable, a replay serves what
 * the arrays then hold); an expert without rows requests nothing; rows no expert covers are left unwritten.
 * Refusals as flute_qgemm_grouped, in its order, before anything is enqueued: dtype, the layer checks, FLUTE_ERR_SHAPE
 * (P, a negative E / R / Tsrc, Tsrc != R without rows, Tsrc == 0 with rows and R > 0); E == 0 or R == 0 returns FLUTE_OK
 * without a launch; then FLUTE_ERR_NULL for a null pointer other than rows.  num_sms < 1: 256. */
int flute_qgemm_grouped_glu(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K, int P,
                            int template_id, const void* Xsrc, const void* rows, const void* offsets, const void* Qgate,
                            const void* Sgate, const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up,
                            void* H, int num_sms, void* stream);

/* flute_qgemm_grouped_glu on the block form's geometry, for prefill and training row counts: the same operands, the same
 * formula - H[r, :] = round_T( silu32(g) * u ), w^ = round_T(QM2-pair-lookup * scale), silu32 the one function above - on the
 * 128-row x 256-column blocks of the dense prefill kernel: a workgroup runs all of K for the gate stack and then all of K
 * for the up stack into two fp32 accumulators of the matrix core (no K split at all), forms the product in fp32 and rounds
 * once, at the store; nothing intermediate reaches global memory, no gathered copy of Xsrc is made.  An entry of its own:
 * flute_qgemm_grouped_glu, flute_qgemm_grouped_glu_ex and flute_qgemm_grouped_form keep their behaviour (the GLU launch
 * there is the row form at every count and refuses FLUTE_GROUPED_FORM_BLOCKS); a caller opts in by calling this one.
 * Equal arguments give equal bits.  Its bits may differ from flute_qgemm_grouped_glu's, whose summation order differs,
 * except on exactly representable inputs (g and u exact in fp32), where they are equal.
 * Grid: floor((R + 127 E) / 128) row blocks, the most a table over R rows can own, times F / 256 - from (E, R, F) alone.
 * The host reads neither offsets nor rows: the launch can be captured in a hipGraph, and a replay serves whatever
 * offsets, rows and Xsrc then hold (same R and Tsrc).  A block past the table's total requests nothing.
 * offsets: every entry clamped to [0, R]; a malformed table (decreasing, overlapping, a last entry past R) cannot read
 * or write outside Xsrc / H: rows it names twice have unspecified contents (one of the naming experts' results), a table
 * whose clamped ranges own more blocks than the grid holds leaves the rows of the surplus blocks unwritten.  Rows no expert
 * serves are left unwritten (no zero fill).  rows: each entry read only for a sorted row inside its expert's range and
 * clamped to [0, Tsrc) before it forms an address - a negative or too large entry reads source row 0 or Tsrc - 1.  The rows
 * of a block at or past its expert's end read no index and no activation (zeros through the bounds of the descriptor over
 * Xsrc) and are never stored: a NaN or Inf in a source row reaches exactly the sorted rows that name it.
 * It serves: num_bits 4 / 2, (K / group_size) % 8 == 0, F a multiple of 256, Tsrc * K * 2 and one expert's scale bytes
 * F * (K / group_size) * 2 below 2^32 - 16, R at most 2^31 - 257, E >= 1, R >= 1.
 * Refusals, before anything is enqueued or dereferenced, in this order: flute_qgemm_grouped_glu's (dtype, the layer checks,
 * FLUTE_ERR_SHAPE for P, a negative E / R / Tsrc, Tsrc != R without rows, Tsrc == 0 with rows and R > 0 - the pointer `rows`
 * is compared with null there and not looked behind); FLUTE_ERR_SHAPE for a shape outside the list above (E == 0 or R == 0
 * are inside it); E == 0 or R == 0 returns FLUTE_OK without a launch; then FLUTE_ERR_NULL for a null pointer other than rows. */
int flute_qgemm_grouped_glu_blocks(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K, int P,
                                   int template_id, const void* Xsrc, const void* rows, const void* offsets, const void* Qgate,
                                   const void* Sgate, const void* QM2gate, const void* Qup, const void* Sup, const void* QM2up,
                                   void* H, int num_sms, void* stream);

/* Which of the two GLU launches a caller should take for R sorted rows read out of Tsrc source rows: FLUTE_GROUPED_FORM_BLOCKS
 * (flute_qgemm_grouped_glu_blocks) where the shape is in its list and the mean rows per expert, R / E, is at least
 * FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS - or FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS_PARTIAL where E * (F / 256) is below
 * num_sms (< 1: 256) -, else FLUTE_GROUPED_FORM_ROWS (flute_qgemm_grouped_glu; E == 0 and R == 0 included), or the negative
 * error either launch would refuse the layer with.  Host only: no pointers, nothing is enqueued; P is taken as
 * num_bits * F / 16.  The two constants are measured on the GLU launches (csrc/api_train.hip): each is the smallest
 * swept mean from which the block launch is not slower on any swept stack of its kind. */
#define FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS 16            /* E * (F / 256) >= num_sms: the experts' column blocks fill the chip */
#define FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS_PARTIAL 48    /* fewer workgroups than compute units */
int flute_qgemm_grouped_glu_blocks_form(int dtype, int num_bits, int group_size, int E, int R, int Tsrc, int F, int K,
                                        int template_id, int num_sms);

/* flute_qgemm_grouped with a per-row weight in the epilogue, for the down projection of a mixture-of-experts MLP:
 *   Y[r, :] = round_T( row_weight[r] * acc32 ),   acc32 = the fp32 sum of X[r, :] @ W_e^T,
 * for every row r in [offsets[e], offsets[e + 1]): the product in fp32, ONE rounding.  row_weight [T] fp32 in device memory.
 * Non-finite inputs propagate as in flute_qgemm_grouped, through the fp32 product: a row weight of 0 on a row holding an
 * Inf gives NaN (0 x inf), on a finite row zeros.  Y rounds to +-inf, not to 65504, also where only the weight takes it there.
 * The rows [clamp(offsets[E]), T) - rows no expert serves - are written as zeros by the same launch, whichever experts
 * have rows (none included); rows >= T are never touched.  Everything else - operands, arithmetic of w^, determinism, the
 * grid, clamping, the refusals and their order, E == 0 or T == 0, num_sms - is flute_qgemm_grouped's; row_weight is one
 * of the pointers FLUTE_ERR_NULL covers. */
int flute_qgemm_grouped_weighted(int dtype, int num_bits, int group_size, int E, int T, int N, int K, int P,
                                 int template_id, const void* X, const void* offsets, const void* Q, const void* S,
                                 const void* QM2, const float* row_weight, void* Y, int num_sms, void* stream);

/* The input gradient of flute_qgemm_grouped and of the fused forms built on it, in ONE launch: a grouped GEMM over the
 * packed stacks that contracts over N where the forward contracts over K.
 *   dX[r, :] = round_T( w_r * sum_n dY[r, n] * w^_e[n, :] )   for every row r in [offsets[e], offsets[e + 1]), e < E,
 * w^ = round_T(QM2-pair-lookup * scale) exactly as flute_dequantize and every MFMA kernel form it, products and sums in
 * fp32 in the matrix core, ONE rounding to T; w_r = row_weight[r] (fp32, device memory), or no multiply when row_weight
 * is null.  dY [R, N] T holds the rows sorted by expert; offsets [E + 1] int32 in DEVICE memory; Q [E, P, K] / S [E, N,
 * K / group_size] / QM2 [E, 2^b, 2^b] as flute_qgemm_grouped takes them; dX [R, K] T.
 * Pair form (dY2, Q2, S2, QM22 all non-null; a second stack of the same shape, num_bits, group_size and template_id):
 *   dX[r, :] = round_T( sum_n dY[r, n] * w^(1)_e[n, :] + sum_n dY2[r, n] * w^(2)_e[n, :] ),
 * both sums added in fp32 (one accumulator: the first stack's columns, then the second's) before the one rounding - the
 * gradient of a row that fed both the gate and the up projection of flute_qgemm_grouped_glu.  It takes no row_weight.
 * Two halves that would each overflow T alone and cancel give 0, not inf - inf: nothing is rounded before the sum is whole.
 * Non-finite inputs propagate by IEEE rules to exactly the outputs the formula connects them to: a NaN or Inf in row r of
 * dY (or dY2) reaches row r of dX only (Inf: +-inf by the sign of w^[n, :], NaN at a zero weight or a zero row weight).
 * fp16 subnormal weights and dY are multiplied as they are, and dX rounds to +-inf, not to 65504 (tests/test_grouped_edges_gpu.py).
 * The rows [clamp(offsets[E]), R) - rows no expert serves - are written as zeros by the same launch whatever the routing:
 * every element of dX is written whenever offsets is a proper table (0 first, non-decreasing, at most R).  Every row
 * index formed is clamped to [0, R]: a malformed table is memory-safe and leaves only the rows it names twice or skips
 * unspecified.  Expert and row bases are 64-bit.
 * A workgroup is (expert, 128 k); it walks the expert's rows in blocks of FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK rows and all
 * of N per block in a fixed order: no atomics, no split of the N reduction across workgroups, equal arguments give equal
 * bits.  The host never reads offsets: the grid is E x ceil(K / 128), from the shapes alone (num_sms is accepted for
 * symmetry and not used), so the launch is hipGraph-capturable and a replay serves what the table then holds.  A
 * workgroup whose expert has no rows requests no weight, scale or table word.
 * Supported layers are flute_qgemm_grouped's: 4 / 3 / 2 bits, TileP 32 / 64 (3 bits: 32), group sizes 32 / 64 / 128 / 256,
 * fp16 / bf16, K % max(64, group_size) == 0, N a multiple of the template's column block.
 * Refusals, before anything is enqueued and in this order: flute_qgemm_grouped's (dtype, the layer checks, FLUTE_ERR_SHAPE
 * for P or a negative E / R), FLUTE_ERR_SHAPE for a row_weight together with any pointer of the pair form; R == 0 returns
 * FLUTE_OK and enqueues nothing; then FLUTE_ERR_NULL for a null dX, and - with E > 0 - for a null dY / offsets / Q / S /
 * QM2 or a pair form given in part.  E == 0 with R > 0 writes dX as zeros (a memset node). */
#define FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK 128
int flute_qgemm_grouped_input_grad(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                   int template_id, const void* dY, const void* offsets, const void* Q, const void* S,
                                   const void* QM2, const float* row_weight, const void* dY2, const void* Q2,
                                   const void* S2, const void* QM22, void* dX, int num_sms, void* stream);
/* FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK of the library that is loaded */
int flute_qgemm_grouped_input_grad_row_block(void);

/* The two forms of the grouped input gradient.  Slabs (flute_grouped_input_grad_form_t 1) is the kernel described above.
 * Blocks (2) is built for experts with hundreds of rows: a workgroup is one 128-row block of one expert x 256 k - the row
 * blocks are found on the device from offsets as the forward's block form finds them, the grid is
 * floor((R + 127 E) / 128) x K / 256, from (E, R, K) alone - and stages the block's dY once for all 256 k.  Operands,
 * arithmetic, clamping, the zero rows from offsets[E] on, determinism and capture are the slab form's, and so is the order
 * in which every output sums over N: the two forms give EQUAL BITS.  (The block form's one difference is the forward block
 * form's: a malformed table that claims more 128-row blocks than a monotone one can own leaves the surplus unwritten.)
 * The block form serves 4 / 2 bits and K % 256 == 0 (R <= 2^31 - 257, a 31-bit grid); 3 bits and other K stay on slabs.
 * The automatic rule (0; flute_qgemm_grouped_input_grad is this) reads shapes only, never offsets: blocks where the shape
 * is eligible and the mean rows per expert, R / E, reach FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS - where one row
 * block per expert already fills the chip, E * (K / 256) >= num_sms - or FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS_PARTIAL
 * where it does not (num_sms < 1: 256).  Both are the lowest means of the recorded sweep from which the block form is not
 * slower on any stack of that kind.
 * flute_qgemm_grouped_input_grad_ex is flute_qgemm_grouped_input_grad with the form chosen by the caller.  One more
 * refusal, after the old entry's (the row_weight / pair refusal included) and before R == 0, E == 0 and the null pointers,
 * so before anything is enqueued or dereferenced: FLUTE_ERR_SHAPE for a form outside the enum, or for blocks where the
 * block form is not eligible (E == 0 or R == 0 included). */
typedef enum {
    FLUTE_GROUPED_INPUT_GRAD_FORM_AUTO = 0, FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS = 1, FLUTE_GROUPED_INPUT_GRAD_FORM_BLOCKS = 2
} flute_grouped_input_grad_form_t;
#define FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS 32            /* E * (K / 256) >= num_sms: the experts' k blocks fill the chip */
#define FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS_PARTIAL 128   /* fewer workgroups per row block than compute units */
int flute_qgemm_grouped_input_grad_ex(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                      int template_id, const void* dY, const void* offsets, const void* Q, const void* S,
                                      const void* QM2, const float* row_weight, const void* dY2, const void* Q2,
                                      const void* S2, const void* QM22, void* dX, int num_sms, void* stream, int form);
/* The form the automatic rule takes: FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS or _BLOCKS, or the negative error the launch
 * itself would refuse the shape with.  Host only: no pointers, nothing is enqueued.  pair != 0: the pair form (the same
 * rule); P is taken as num_bits * N / 16; num_sms < 1: 256. */
int flute_qgemm_grouped_input_grad_form(int pair, int dtype, int num_bits, int group_size, int E, int R, int N, int K,
                                        int template_id, int num_sms);

/* The gradient of the scales of a stack flute_qgemm_grouped multiplies by, in ONE launch: flute_qgemm_scale_grad for every
 * expert over the rows the device-side table gives it.  With b_e = clamp(offsets[e], 0, R), e_e = clamp(offsets[e + 1], 0, R):
 *   dS[e, n, j] = round_T( sum_{r in [b_e, e_e)} sum_{k in group j} dYw[r, n] * X[r, k] * L_e[k, n] ),
 * L_e the pair lookup of expert e's codes in expert e's QM2 (flute_qgemm_scale_grad's L), dYw = dY when row_weight is null and
 * dYw[r, n] = round_T(row_weight[r] * dY[r, n]) otherwise - the product in fp32, one round-to-nearest-even to T, formed where
 * the dY tile is staged - which is the gradient that reaches flute_qgemm_grouped_weighted's product.  Products and sums in
 * fp32 in flute_qgemm_scale_grad's order, one rounding of the result: wherever that launch does not split M (always without
 * scratch) an expert's dS has its bits.  Non-finite inputs propagate by IEEE rules to exactly the outputs the formula connects
 * them to - flute_qgemm_scale_grad's rule inside the expert that owns the row, and no other expert's dS: rows outside an
 * expert's range are not loaded, never multiplied by zero.  dYw and dS round to +-inf, not to 65504, and a subnormal dYw is kept.
 * dY [R, N] and X [R, K] row-major T, rows sorted by expert; offsets [E + 1] int32 in DEVICE memory; Q [E, P, K] int16;
 * QM2 [E, 2^b, 2^b] fp32 words; row_weight [R] fp32 in device memory or null; dS [E, N, K / group_size] T.
 * The host never reads offsets: the grid is (N / 128, ceil(K / 256), E), from the shapes alone (num_sms is accepted for
 * symmetry and not used).  One workgroup walks all rows of its expert: no split of the row reduction, no scratch, no
 * atomics, equal arguments give equal bits, and the launch is hipGraph-capturable (a replay serves what the table then
 * holds).  Every element of dS is written.  An expert with e_e <= b_e gets zeros and none of its codes or table words is
 * read (a table of inf / NaN there stays out of the result).  Rows from clamp(offsets[E]) on are never read, and every row
 * index formed lies inside [0, R): a malformed table (decreasing, past R) is memory-safe.  Expert bases into Q / QM2 / dS
 * and row bases into dY / X are 64-bit.
 * Supported layers are flute_qgemm_scale_grad's: 4 / 2 bits with TileP 32 / 64, 3 bits with TileP 32, fp16 / bf16, group
 * sizes 32 / 64 / 128 / 256, N % 128 == 0, K % max(64, group_size) == 0.
 * Refusals, before anything is enqueued and in this order: flute_qgemm_grouped's (dtype, the layer checks, FLUTE_ERR_SHAPE
 * for P or a negative E / R), FLUTE_ERR_SHAPE for E > 65535; E == 0 returns FLUTE_OK (dS is empty); then FLUTE_ERR_NULL for
 * a null dS; R == 0 writes dS as zeros (a memset node) and returns; then FLUTE_ERR_NULL for a null dY / X / offsets / Q /
 * QM2.  No pointer is dereferenced by the host. */
int flute_qgemm_grouped_scale_grad(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                   int template_id, const void* dY, const void* X, const void* offsets, const void* Q,
                                   const void* QM2, const float* row_weight, void* dS, int num_sms, void* stream);

/* The gradient of the lookup tables of a stack flute_qgemm_grouped multiplies by, with the codes fixed: flute_qgemm_table_grad
 * for every expert over the rows the device-side table gives it, in one main launch and one small reduce launch.  With
 * b_e = clamp(offsets[e], 0, R), e_e = clamp(offsets[e + 1], 0, R):
 *   dT2[e, c, h] = sum over (kappa, n) whose pair index in expert e's codes is c of G_e[2 kappa + h, n] * S[e, n, 2 kappa / group_size],
 *   G_e[k, n]    = sum_{r in [b_e, e_e)} X[r, k] * dYw[r, n],
 * dYw as flute_qgemm_grouped_scale_grad forms it (dY, or round_T(row_weight[r] * dY[r, n]), the product in fp32), the pair index
 * and the halves h as flute_qgemm_table_grad's c and e.  dT2 [E, 4^b, 2] fp32, written whole; the tables are not read.  dY [R, N]
 * and X [R, K] row-major T, rows sorted by expert; offsets [E + 1] int32 in DEVICE memory; Q [E, P, K] int16; S [E, N, K /
 * group_size] T; row_weight [R] fp32 in device memory or null.
 * With dS non-null the same launch also writes the stack's scale gradient dS [E, N, K / group_size] T, bit for bit what
 * flute_qgemm_grouped_scale_grad returns for the same arguments; QM2 [E, 2^b, 2^b] fp32 words is needed then and only then.
 * The host never reads offsets: the main grid is (N / 128, ceil(K / 256), E), from the shapes alone (num_sms is accepted for
 * symmetry and not used).  One workgroup walks all rows of its expert - no split of the row reduction - and writes one fp32
 * partial to `scratch`; the reduce launch sums an expert's partials in fp64 in flute_qgemm_table_grad's order (32 slots, each
 * every 32nd workgroup in the order k block * (N / 128) + n block, then a fixed binary tree) and rounds once to fp32.  So
 * dT2[e] has flute_qgemm_table_grad's bits on the expert's rows wherever that launch does not split M.  No atomics on global
 * memory, equal arguments give equal bits, and both launches are hipGraph-capturable (a replay serves what the table then holds).
 * An expert with e_e <= b_e gets dT2[e] (and its dS) as zeros; none of its codes, scales or table words is read, and neither is
 * its part of the scratch.  Rows from clamp(offsets[E]) on are never read - not multiplied by zero - and every row index formed
 * lies inside [b_e, e_e) inside [0, R): a malformed table (decreasing, past R, negative) is memory-safe and gives the result of
 * the clamped table.  Expert bases into Q / S / QM2 / dS / dT2 / scratch and row bases into dY / X are 64-bit.
 * Non-finite inputs propagate by IEEE rules to exactly the bins of the expert that owns the row - flute_qgemm_table_grad's rule
 * inside that expert - and reach no other expert's dT2 or dS.
 * `scratch` must hold flute_qgemm_grouped_table_grad_scratch_bytes(num_bits, group_size, E, N, K) =
 * E * (N / 128) * ceil(K / 256) * 2 * 4^b * 4 bytes: every (expert, block) has its slot whether or not the expert has rows,
 * which is the price of not reading offsets on the host.  A large stack pays for it: E 256, N 2048, K 7168 at 4 bits needs
 * 235 MB (the figure scales with 4^b: 15 MB at 2 bits).  Less is FLUTE_ERR_WORKSPACE (more changes nothing).  The query
 * takes no template_id: it is 0 for a num_bits / group_size / shape no template accepts (N % 128, K % max(64, group_size),
 * E < 1, E > 65535) and may be non-zero for arguments one template's own checks still refuse.
 * Supported layers are flute_qgemm_grouped_scale_grad's.  Refusals, before anything is enqueued and in this order:
 * flute_qgemm_grouped_scale_grad's (dtype, the layer checks, FLUTE_ERR_SHAPE for P or a negative E / R, FLUTE_ERR_SHAPE for
 * E > 65535); E == 0 returns FLUTE_OK (dT2 is empty); then FLUTE_ERR_NULL for a null dT2 or scratch, or a null QM2 with a dS;
 * FLUTE_ERR_WORKSPACE; R == 0 writes dT2 (and dS) as zeros (memset nodes) and returns; then FLUTE_ERR_NULL for a null dY / X /
 * offsets / Q / S.  No pointer is dereferenced by the host. */
int flute_qgemm_grouped_table_grad(int dtype, int num_bits, int group_size, int E, int R, int N, int K, int P,
                                   int template_id, const void* dY, const void* X, const void* offsets, const void* Q,
                                   const void* S, const void* QM2, const float* row_weight, float* dT2, void* dS,
                                   void* scratch, size_t scratch_bytes, int num_sms, void* stream);
size_t flute_qgemm_grouped_table_grad_scratch_bytes(int num_bits, int group_size, int E, int N, int K);

/* The routing of a mixture-of-experts step in ONE launch: from the router's choice to every array the grouped launches
 * and flute_moe_combine read.  ids [T, k] int32 or int64 (id_dtype: flute_index_dtype; torch.topk returns int64), weights
 * [T, k] fp16 / bf16 / fp32 (weight_dtype: flute_dtype) or null, E experts.  With P = T k and the pairs (token, slot)
 * numbered p = token k + slot, all outputs have a fixed shape:
 *   offsets    [E + 1] int32   offsets[e] = the number of pairs whose id is in [0, e): expert e's rows are
 *                              [offsets[e], offsets[e + 1]), offsets[E] = the pairs some expert serves
 *   perm       [P] int32       the pair of sorted row i; a STABLE sort by expert: pairs of one expert in ascending p
 *   rows       [P] int32       perm[i] / k, the token of sorted row i (flute_qgemm_grouped_glu's `rows`)
 *   row_weight [P] fp32        (float) weights[perm[i]], exact (flute_qgemm_grouped_weighted's `row_weight`); not written
 *                              and not looked at when weights is null
 *   pos        [T, k] int32    the inverse: pos[perm[i]] = i
 * An id outside [0, E) sorts behind every expert, from offsets[E] on, in ascending p among its like, and still gets its
 * perm / rows / row_weight / pos entries.  The comparison is made at the ids' own width: an int64 id of 2^32 + 1 is
 * outside, not expert 1.  offsets, perm are integrations/moe.py sort_by_expert's, value for value.
 * Integer counting only: a counting sort inside one workgroup of 16 waves (moe_route.hip), each wave on one contiguous
 * range of the pairs, no atomics on global memory, nothing that depends on scheduling: equal arguments give equal bits.
 * The host reads neither ids nor weights; the grid is one workgroup whatever (P, E) (hipGraph-capturable, a replay serves
 * what the arrays then hold).  Correct for every P below FLUTE_MOE_ROUTE_MAX_PAIRS, fast for decode-sized ones: the
 * multi-workgroup form for prefill-sized P is flute_moe_route_wide below.
 * Refusals in this order, before anything is enqueued: FLUTE_ERR_DTYPE (id_dtype, then weight_dtype - checked with null
 * weights too); FLUTE_ERR_SHAPE (a negative T / k / E, E > FLUTE_MOE_ROUTE_MAX_EXPERTS, T k >=
 * FLUTE_MOE_ROUTE_MAX_PAIRS); P == 0 (T == 0 or k == 0) with a null offsets returns FLUTE_OK without a launch; then
 * FLUTE_ERR_NULL (offsets; with P > 0 also ids, perm, rows, pos, and row_weight when weights is given).  P == 0 with
 * offsets given is served by the same launch, which then reads no other pointer and writes the E + 1 zeros. */
#define FLUTE_MOE_ROUTE_MAX_EXPERTS 1024
#define FLUTE_MOE_ROUTE_MAX_PAIRS (1 << 27) /* 2^31 / 16: a wave's range end, rounded up to 64, stays an int */
int flute_moe_route(int id_dtype, int weight_dtype, int T, int k, int E, const void* ids, const void* weights,
                    int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* stream);

/* The gating of a mixture-of-experts step in ONE launch: from the router's logits [T, E] fp16 / bf16 / fp32 (logit_dtype:
 * flute_dtype, FLUTE_F32 included) to the k experts each token goes to, ids [T, k] int32, and their weights [T, k] fp32 -
 * exactly what flute_moe_route accepts (FLUTE_I32, FLUTE_F32).  bias [E] fp32 or null.  Everything is computed in fp32.
 *   score      x_e = (float) logits[t, e].  FLUTE_GATE_SOFTMAX: m = max_e x_e, u_e = exp(x_e - m), s_e = u_e / sum over ALL e of u_e.
 *              FLUTE_GATE_SIGMOID: s_e = 1 / (1 + exp(-x_e)).
 *   key        without bias the key of expert e is x_e itself (both scorings increase with x, so no rounding of a probability can
 *              make or break a tie); with bias it is s_e + bias[e] in fp32 (the "correction bias" of DeepSeek-V3 / GLM: it decides
 *              the choice only and never enters a weight).  A NaN key compares as -infinity (and -0 as +0).
 *   choice     slot j holds the expert with the j-th largest key, equal keys in ascending expert index: a total order, so ids is
 *              defined value for value and never holds an expert twice.
 *   weight     w_j = s_{ids[j]}; with renormalize (any nonzero value) w_j = s_{ids[j]} / (s_{ids[0]} + ... + s_{ids[k-1]}), a
 *              compensated sum taken in slot order - for a softmax without bias as u_{ids[j]} / (the same sum of u): the sum
 *              over all E is then not formed.  Then w_j = w_j * scale (one more rounding; scale = 1 changes nothing).  A row in
 *              which every chosen score is 0 or not finite gets whatever this arithmetic gives (a division by zero, NaN); only
 *              its ids are defined.
 * Limits: 1 <= k <= min(E, FLUTE_MOE_GATE_MAX_TOPK), E <= FLUTE_MOE_ROUTE_MAX_EXPERTS, T k < FLUTE_MOE_ROUTE_MAX_PAIRS.
 * The choice here is over all E experts; DeepSeek's group-limited selection (n_group, topk_group) is flute_moe_gate_limited /
 * flute_moe_gate_route_limited below.
 * One wave per token, lane l holding experts l, l + 64, ... in registers; the max, the sum and the k rounds of "largest key,
 * lowest index" are wave reductions in a fixed order and ballots, without LDS (moe_gate.hip).  The host reads nothing, the grid follows from T
 * alone (hipGraph-capturable), no atomics, plain vector stores: equal arguments give equal bits, and a token's ids and weights
 * depend neither on T nor on the row it sits in.
 * Refusals in this order, before anything is enqueued: FLUTE_ERR_DTYPE (logit_dtype, then scoring); FLUTE_ERR_SHAPE (a negative
 * T, k < 1, k > E, k > FLUTE_MOE_GATE_MAX_TOPK, E > FLUTE_MOE_ROUTE_MAX_EXPERTS, T k >= FLUTE_MOE_ROUTE_MAX_PAIRS); T == 0 returns
 * FLUTE_OK without a launch; then FLUTE_ERR_NULL (logits, ids, weights; bias is optional). */
#define FLUTE_MOE_GATE_MAX_TOPK 64
int flute_moe_gate(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale, const void* logits,
                   const float* bias, int32_t* ids, float* weights, void* stream);

/* flute_moe_gate and flute_moe_route in ONE launch: a decode step goes from the router's logits to every routing array.  It
 * writes ids and weights exactly as flute_moe_gate does, and offsets, perm, rows, row_weight, pos exactly as
 * flute_moe_route(FLUTE_I32, FLUTE_F32, T, k, E, ids, weights, ...) then writes on them: bit for bit the two-call sequence (both
 * forms run the same per-token device function and the same counting sort).  One workgroup of 16 waves, flute_moe_route's design
 * point: its waves loop over the tokens, and after a barrier the count / scan / place phases run on what they wrote.  Correct for
 * every T the limits admit, fast for decode-sized ones.  Everything else - the arithmetic, the limits, the properties - is
 * flute_moe_gate's.
 * Refusals in the same order: FLUTE_ERR_DTYPE; FLUTE_ERR_SHAPE; T == 0 with a null offsets returns FLUTE_OK without a launch;
 * then FLUTE_ERR_NULL (offsets; with T > 0 also logits, ids, weights, perm, rows, row_weight, pos).  T == 0 with offsets given is
 * served by the same launch, which then reads no other pointer and writes the E + 1 zeros, as flute_moe_route does. */
int flute_moe_gate_route(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale,
                         const void* logits, const float* bias, int32_t* ids, float* weights, int32_t* offsets,
                         int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* stream);

/* flute_moe_gate with DeepSeek's group-limited selection: the E experts form n_group contiguous groups of gs = E / n_group
 * (group g is experts g gs .. (g + 1) gs - 1), the topk_group best groups are chosen first, and the k experts are then chosen
 * among the experts of those groups only.  Score, key and weight are flute_moe_gate's; one stage sits between key and choice:
 *   group key     group_score (flute_gate_group_score) FLUTE_GATE_GROUP_MAX (DeepSeek-V2): the largest expert key of the group - the
 *                 keys are flute_moe_gate's, the logit itself without a bias (nothing is rounded), s_e + bias[e] with one.
 *                 FLUTE_GATE_GROUP_TOP2SUM (DeepSeek-V3): the sum, ONE fp32 addition, of the two largest c_e = s_e (+ bias[e]) of
 *                 the group, a NaN c_e counting as -infinity; needs gs >= 2.  s_e is the normalised score: with
 *                 FLUTE_GATE_SOFTMAX this form always divides by the sum over all E, under renormalize and without a bias too,
 *                 where flute_moe_gate renormalises the u_e directly - the weights are then s_j / (the compensated sum of the
 *                 chosen s), equal in value and not always in bits.  A NaN group key compares as -infinity (and -0 as +0).
 *   group choice  the topk_group groups with the largest group keys, equal keys to the lower group index: a total order.
 *   choice        flute_moe_gate's k rounds over the experts of the chosen groups.  An expert of another group is never chosen,
 *                 whatever its key (the -infinity mask of vLLM's grouped_topk; the HF modelling code fills with 0.0 instead, which
 *                 lets a masked expert beat an allowed one with a negative key - that is not reproduced).  Hence k <= topk_group gs.
 * With topk_group == n_group (n_group == 1 included) every expert is allowed, whatever group_score is: the call is served by
 * flute_moe_gate's own kernel and the result is bit for bit flute_moe_gate's.
 * Limits: flute_moe_gate's, and 1 <= n_group <= FLUTE_MOE_GATE_MAX_GROUPS, E % n_group == 0, 1 <= topk_group <= n_group,
 * k <= topk_group gs.  The same wave-per-token kernel with the group stage compiled in (moe_gate.hip): a wave-uniform loop over the
 * groups (a masked wave maximum each, two for the sum), topk_group rounds of "largest group key, lowest group" on lane g's group key,
 * and the keys of the experts outside the chosen groups cleared; no LDS, no atomics, plain vector stores; every property of
 * flute_moe_gate holds (capturable, equal bits for equal arguments, a token's result independent of T and of its row).
 * Refusals in this order, before anything is enqueued: FLUTE_ERR_DTYPE (logit_dtype, then scoring, then group_score);
 * FLUTE_ERR_SHAPE (flute_moe_gate's conditions; then n_group < 1 or > FLUTE_MOE_GATE_MAX_GROUPS; E % n_group; topk_group < 1 or
 * > n_group; k > topk_group gs; FLUTE_GATE_GROUP_TOP2SUM with gs < 2); T == 0 returns FLUTE_OK without a launch; then FLUTE_ERR_NULL
 * (logits, ids, weights; bias is optional). */
#define FLUTE_MOE_GATE_MAX_GROUPS 64
int flute_moe_gate_limited(int logit_dtype, int T, int E, int k, int n_group, int topk_group, int group_score, int scoring,
                           int renormalize, float scale, const void* logits, const float* bias, int32_t* ids, float* weights,
                           void* stream);

/* flute_moe_gate_limited and flute_moe_route in ONE launch, as flute_moe_gate_route is for flute_moe_gate: ids and weights bit for bit
 * flute_moe_gate_limited's, the five routing arrays bit for bit what flute_moe_route then writes on them.  One workgroup of 16 waves.
 * With topk_group == n_group it is served by flute_moe_gate_route's kernel, bit for bit in all seven arrays.
 * Refusals: flute_moe_gate_limited's FLUTE_ERR_DTYPE and FLUTE_ERR_SHAPE; T == 0 with a null offsets returns FLUTE_OK without a
 * launch; then FLUTE_ERR_NULL (offsets; with T > 0 also logits, ids, weights, perm, rows, row_weight, pos).  T == 0 with offsets
 * given writes the E + 1 zeros. */
int flute_moe_gate_route_limited(int logit_dtype, int T, int E, int k, int n_group, int topk_group, int group_score, int scoring,
                                 int renormalize, float scale, const void* logits, const float* bias, int32_t* ids,
                                 float* weights, int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos,
                                 void* stream);

/* The routing over MANY workgroups, for prefill and training token counts: flute_moe_route's contract in three plain launches
 * (moe_route_wide.hip).  All five arrays are bit for bit what flute_moe_route writes for the same arguments - a stable sort by expert
 * has one answer, and the device code of the count and the place is the one-workgroup kernel's.
 *   chunks   chunk c owns the chunk_tokens consecutive tokens [c chunk_tokens, (c + 1) chunk_tokens) cut at T, one contiguous range
 *            of pairs; C = ceil(T / chunk_tokens) chunks (C = 1 where T k == 0), one workgroup of 16 waves each.
 *   count    grid C: each workgroup counts its chunk per bucket (E + 1 buckets, the last for ids outside [0, E)) into hist[c][.].
 *   scan     grid ceil((E + 1) / 64): each bucket's column of hist becomes its exclusive prefix over the chunks; its total to total[.].
 *   place    grid C: each workgroup scans total over the buckets (workgroup 0 stores offsets), counts its chunk per wave again and
 *            places: row = (pairs of lower buckets) + (pairs of this bucket in earlier chunks, earlier waves) + rank in the wave's step.
 * The kernel boundaries are the only ordering between workgroups: no workgroup waits on another inside a launch, there is no arrival
 * counter and no atomic on global memory, so the launches need no co-residency and cannot hang.  The price is two more launches.
 * workspace: flute_moe_route_wide_workspace(T, k, E, chunk_tokens) bytes, (C + 1) (E + 1) int32 - hist [C][E + 1], chunk-major (the
 * two grid-C launches then touch contiguous rows; the scan reads 64 neighbouring buckets per wave, contiguous too), then total
 * [E + 1].  Every word a launch reads was written by an earlier launch of the SAME call: the workspace may hold anything before, and
 * holds nothing of use after.  The query returns 0 for a shape or chunk_tokens the launch refuses; with chunk_tokens 0 it covers the
 * automatic chunk of either entry.  More bytes change nothing.
 * chunk_tokens: 0 = automatic, a function of (T, k) only: the tokens of FLUTE_MOE_ROUTE_WIDE_PAIRS pairs here,
 * FLUTE_MOE_GATE_ROUTE_WIDE_TOKENS tokens in the gated entry, either grown where C would pass FLUTE_MOE_ROUTE_MAX_CHUNKS (the
 * workspace at E = 1024 then stays below 34 MB).  Both come from the sweep of DESIGN.md 3.3s: 512 pairs is the fastest or within
 * 2 % of it at every swept shape of 8192 pairs and more (2048 pairs per chunk costs 12 - 22 % more, 4096 up to 55 %), and 16 tokens
 * is the fastest gated chunk at E = 256 and at 1024 tokens of E = 8 and E = 64 (at E = 256 32 tokens costs 28 - 44 % more: a wave
 * gates its tokens one after the other) and within 13 % of the fastest, 32, at 4096 tokens of E = 8 and E = 64.  An explicit value (>= 1, with C <= FLUTE_MOE_ROUTE_MAX_CHUNKS) is for tests and
 * sweeps, the routing's counterpart of flute_overrides.
 * C == 1 (T <= chunk_tokens; T k == 0 with offsets given, which writes the E + 1 zeros) is served by flute_moe_route's own
 * one-workgroup launch, as topk_group == n_group is served by the unlimited gating kernel; the workspace is then not touched and
 * may be null.
 * Every property of flute_moe_route holds: the host reads nothing, the grids follow from (T, k, E, chunk_tokens) alone
 * (hipGraph-capturable), equal arguments give equal bits.
 * Refusals in this order, before anything is enqueued: flute_moe_route's FLUTE_ERR_DTYPE and FLUTE_ERR_SHAPE, in its order;
 * FLUTE_ERR_SHAPE for chunk_tokens < 0 or C > FLUTE_MOE_ROUTE_MAX_CHUNKS; T k == 0 with a null offsets returns FLUTE_OK without a
 * launch; FLUTE_ERR_NULL (flute_moe_route's pointers, and workspace when C > 1); FLUTE_ERR_WORKSPACE when C > 1 and workspace_bytes
 * is below the query's figure for the same (T, k, E) and the chunk in use. */
#define FLUTE_MOE_ROUTE_MAX_CHUNKS 8192
#define FLUTE_MOE_ROUTE_WIDE_PAIRS 512
#define FLUTE_MOE_GATE_ROUTE_WIDE_TOKENS 16
size_t flute_moe_route_wide_workspace(int T, int k, int E, int chunk_tokens);
int flute_moe_route_wide(int id_dtype, int weight_dtype, int T, int k, int E, const void* ids, const void* weights,
                         int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* workspace,
                         size_t workspace_bytes, int chunk_tokens, void* stream);

/* flute_moe_gate_route and flute_moe_gate_route_limited over many workgroups, ONE entry for both gatings: topk_group == n_group
 * (n_group == 1 included) is the unlimited gating, as in flute_moe_gate_route_limited.  ids, weights and the five routing arrays
 * are bit for bit what flute_moe_gate_route[_limited] writes.  The first launch is the gated count (moe_gate.hip): workgroup c's
 * wave w gates the chunk's tokens w, w + 16, ... with the per-token device function every gating kernel runs, then the workgroup
 * counts the ids it wrote itself; scan and place are flute_moe_route_wide's launches on those ids and weights.  Workspace,
 * chunk_tokens (automatic: FLUTE_MOE_GATE_ROUTE_WIDE_TOKENS tokens, one per wave and round) and C == 1 (served by the one-workgroup
 * flute_moe_gate_route[_limited] launch) as above.
 * Refusals in this order: flute_moe_gate_route_limited's FLUTE_ERR_DTYPE and FLUTE_ERR_SHAPE; FLUTE_ERR_SHAPE for chunk_tokens;
 * T == 0 with a null offsets returns FLUTE_OK; FLUTE_ERR_NULL (its pointers, and workspace when C > 1); FLUTE_ERR_WORKSPACE. */
int flute_moe_gate_route_wide(int logit_dtype, int T, int E, int k, int n_group, int topk_group, int group_score, int scoring,
                              int renormalize, float scale, const void* logits, const float* bias, int32_t* ids, float* weights,
                              int32_t* offsets, int32_t* perm, int32_t* rows, float* row_weight, int32_t* pos, void* workspace,
                              size_t workspace_bytes, int chunk_tokens, void* stream);

/* Which routing to take for T tokens, top-k, E experts - gated: flute_moe_gate_route[_limited] against flute_moe_gate_route_wide,
 * else flute_moe_route against flute_moe_route_wide: FLUTE_MOE_ROUTE_FORM_ONE or FLUTE_MOE_ROUTE_FORM_WIDE, or (< 0) the launch's
 * FLUTE_ERR_SHAPE.  Host only, shapes alone, monotone in T at fixed (k, E): wide from T k >= FLUTE_MOE_ROUTE_WIDE_MIN_PAIRS pairs on
 * (where the automatic chunk gives more than one chunk, which it then does), gated or not.  The threshold is the measured crossover
 * (profiles/grouped_moe_route_wide.json): against the better of the one-launch flute_moe_gate_route[_limited] and the
 * two-call flute_moe_gate[_limited] + flute_moe_route the wide form loses at every measured row of 2048 pairs and below (1024 tokens
 * top-2 at E = 8: 10.5 us against 7.9; 256 tokens top-8 at E = 64 and E = 256: 11.7 against 9.9, 21.1 against 16.8) and wins at
 * every row of 8192 pairs and above (4096 tokens top-2: 14.5 us against 17.4; 1024 tokens top-8: 13.0 against 23.1, 22.6 against
 * 30.5; 16384 tokens top-8 at E = 256: 78 us against 313, and against 11.6 ms of the one-launch form); ungated the same two rows
 * (8192 pairs: 0.62 - 0.75 of flute_moe_route's time, 131072 pairs: 0.09).  Nothing between 2048 and 8192 pairs was measured: the
 * rule says "one" there.  The one-launch gated form alone - what a caller of flute_moe_gate_route has today - is passed much
 * earlier, at 64 - 256 tokens; a caller who has only that alternative may take the wide entry from there.  num_sms is accepted as
 * in the other _form entries (< 1: a whole part) and does not enter the rule: the crossover was measured on a whole part only. */
#define FLUTE_MOE_ROUTE_FORM_ONE 1
#define FLUTE_MOE_ROUTE_FORM_WIDE 2
#define FLUTE_MOE_ROUTE_WIDE_MIN_PAIRS 8192
int flute_moe_route_form(int gated, int T, int k, int E, int num_sms);

/* The end of a mixture-of-experts step: the sorted rows Y [P, N] T of the down projection (flute_qgemm_grouped_weighted's
 * output), summed per token through pos [T, k] int32 (flute_moe_route's), into out [T, N] T.  Per element:
 *   served = clamp(offsets[E], 0, P)
 *   acc = +0.0f;  for j = 0 .. k - 1, ascending:  p = pos[t, j];  if (0 <= p < served) acc += (float) Y[p, n]
 *   out[t, n] = round_T(acc)
 * fp32 additions in slot order, ONE rounding (to +-inf, not to 65504).  Non-finite inputs propagate by IEEE rules to
 * exactly the outputs the formula connects them to: a NaN in a served row reaches its token's row in that column, +inf
 * and -inf in two slots of one token give NaN there.  Every element of out is written - a token with no served slot is zeros -
 * so out needs no zero fill.  Rows of Y at or past `served` and positions outside [0, P) are never read: the result does
 * not depend on what the rows no expert served hold.  No atomics: equal arguments give equal bits for every k.  Of
 * offsets [E + 1] int32 only offsets[E] is read, on the device; the host reads neither it nor pos, and the grid follows
 * from (T, N) alone (hipGraph-capturable).  A pure stream, 16 bytes per lane (moe_combine.hip).
 * Refusals in this order, before anything is enqueued: FLUTE_ERR_DTYPE; FLUTE_ERR_SHAPE (a negative T / k / E / N,
 * N % 8, T k or T * ceil(N / 1024) above 2^31 - 1); T == 0 or N == 0 returns FLUTE_OK without a launch; then
 * FLUTE_ERR_NULL (offsets, out; Y and pos unless k == 0 - with k == 0 the launch writes out as zeros). */
int flute_moe_combine(int dtype, int T, int k, int E, int N, const void* Y, const int32_t* pos, const int32_t* offsets,
                      void* out, void* stream);

/* The SwiGLU derivative of the fused GLU launch's backward: from g, u (the recomputed gate and up products) and dh (the gradient
 * of h = silu(g) u), all [R, F] T, contiguous, F % 8 == 0, the gradients dg, du [R, F] T.  Per element, in fp32, every operation
 * rounded once, in this order (no contraction into an fma), ONE rounding to T per output (to +-inf, not to 65504):
 *   d   = 1 + expf(-g)
 *   sl  = g / d                          (silu32, csrc/silu32.h: the forward's function, the same bits from the same g)
 *   sig = 1 / d
 *   ds  = sig * (1 + g * (1 - sig))
 *   dg  = round_T((dh * u) * ds)
 *   du  = round_T(dh * sl)
 * The contract is the formula: no selects, no special cases.  Every finite g of either type gives finite ds and sl - where expf(-g)
 * overflows (g <= -89; g = -65504, g = -3.39e38) d = inf, sig = +0, sl = -0 and ds = +0 * (1 + g) = -0; where it vanishes against
 * the 1 (g >= 18; g = +65504, g = +3.39e38) d = 1, sig = 1, 1 - sig = 0, sl = g and ds = 1.  A non-finite g, u or dh gives what IEEE
 * arithmetic gives for that element and touches no other element.
 * offsets [E + 1] int32 (device memory) or NULL.  NULL: every row is served and E is ignored.  Otherwise
 * served = clamp(offsets[E], 0, R), read on the device, and the rows at or past `served` are written as +0 in both outputs while
 * their g, u and dh are never read (the plain launches leave those rows unwritten).  Every element of dg and du is written in
 * either case.  The host reads no operand; the grid follows from (R, F) alone (hipGraph-capturable).  A pure stream, one lane per
 * 8 columns of one row: 10 bytes per element (csrc/swiglu_grad.hip).  Equal arguments give equal bits.
 *
 * Error account, against the formula in exact arithmetic on the same 16-bit inputs, to first order.  eps = 2^-24 is fp32's unit
 * roundoff and u_T the unit roundoff of T (2^-11 fp16, 2^-8 bf16); expf is within 1 ulp (2 eps relative); |g| <= 88 (silu32.h's
 * range), no fp32 intermediate subnormal and the result normal in T.
 *   sl: silu32.h's count, 2 eps + eps + eps = 4 eps = 2^-22.  du adds the fp32 product (eps) and the rounding to T:
 *       |du - du_ref| <= (u_T + eps_s) |du_ref|,  eps_s = 2^-21 (silu32.h's constant, which covers 5 eps).
 *   ds: sig = 1 / d carries 4 eps relative (expf 2, the sum 1, the quotient 1).  1 - sig then carries 4 eps sig + eps (1 - sig)
 *       absolute, g (1 - sig) that times |g| plus its own eps, the sum with 1 one more eps of its value, and the product with sig
 *       sig's 4 eps and one more.  With sig <= 1, sig + (1 - sig) = 1 and |ds_ref| <= 1.1:
 *       |ds - ds_ref| <= eps (4 |g| + 6 |ds_ref|) <= 6.6 eps (1 + |g|).
 *   dg: dh * u (eps; exact for fp16) and the product with ds (eps) add 2 eps |ds_ref| <= 2.2 eps: 8.8 eps (1 + |g|) |dh u| = 4.4 * 2^-23
 *       (1 + |g|) |dh u| before the rounding to T, which adds u_T of the value.  With the constant rounded up for the second-order terms
 *       |dg - dg_ref| <= u_T |dg_ref| + c * 2^-23 * (1 + |g|) * |dh * u|,  c = 5.
 *       (ds_ref passes through zero at g = -1.278..: a bound relative to dg_ref alone does not exist.  Outside |g| <= 88 ds and ds_ref
 *       are both within 2^-120 of 0 or both of 1, so the bound holds there too.)
 * Refusals in this order, before anything is enqueued and before a required pointer is looked at: FLUTE_ERR_DTYPE; FLUTE_ERR_SHAPE
 * (a negative R or F, a negative E with offsets given, F % 8, R * ceil(F / 1024) above 2^31 - 1); R == 0 or F == 0 returns FLUTE_OK
 * without a launch; then FLUTE_ERR_NULL (g, u, dh, dg, du). */
int flute_swiglu_grad(int dtype, int R, int F, int E, const void* g, const void* u, const void* dh, const int32_t* offsets,
                      void* dg, void* du, void* stream);

/* The row gather in front of the backward's recompute, the transpose of flute_moe_combine: X [Tsrc, K] T, rows [R] int32
 * (flute_moe_route's), K % 8 == 0, out [R, K] T with
 *   out[r, :] = X[clamp(rows[r], 0, Tsrc - 1), :]   for r < served;   +0 for r >= served, whose rows[r] is never read
 * served as flute_swiglu_grad's (offsets NULL: R, and E is ignored).  A copy of 16-bit patterns: a served row is bit for bit the row
 * it names, NaN payloads included.  Every element of out is written.  The host reads neither rows nor offsets; the grid follows
 * from (R, K) alone (hipGraph-capturable).  One lane per 16 bytes (csrc/swiglu_grad.hip).
 * Refusals in this order: FLUTE_ERR_DTYPE; FLUTE_ERR_SHAPE (a negative R, Tsrc or K, a negative E with offsets given, K % 8,
 * Tsrc == 0 with R > 0 and K > 0, R * ceil(K / 1024) above 2^31 - 1); R == 0 or K == 0 returns FLUTE_OK without a launch; then
 * FLUTE_ERR_NULL (X, rows, out). */
int flute_moe_gather(int dtype, int R, int Tsrc, int K, int E, const void* X, const int32_t* rows, const int32_t* offsets,
                     void* out, void* stream);

/* The routing weight's share of the weighted launch's backward, in ONE launch.  dHp [R, K] T is the unweighted input gradient, as
 * flute_qgemm_grouped_input_grad writes it without a row weight; H [R, K] T is the weighted launch's input; row_weight [R] fp32;
 * contiguous, K % 8 == 0.  Per row r < served:
 *   d_row_weight[r] = sum over k of (float) dHp[r, k] * (float) H[r, k]          fp32
 *   dH[r, k]        = round_T(row_weight[r] * (float) dHp[r, k])                 ONE fp32 product, ONE rounding (to +-inf, not to 65504)
 * offsets [E + 1] int32 (device memory) or NULL with flute_swiglu_grad's meaning: NULL serves every row and E is ignored; otherwise
 * served = clamp(offsets[E], 0, R), read on the device, and the rows at or past `served` are written as +0 in both outputs while
 * nothing of theirs is read - not dHp, not H (which may hold NaN there), not row_weight[r].  dH may be NULL: then only d_row_weight
 * is formed; row_weight is NULL exactly when dH is.  Every element of every non-null output is written.
 * Summation order.  The product of two fp16 or two bf16 values is exact in fp32 (22 / 16 significant bits; bf16 products beyond
 * fp32's range excepted), so only the order of the additions is free, and it is fixed: one workgroup of 256 lanes takes one row;
 * lane l takes the columns 2048 i + 8 l .. + 7 of step i = 0, 1, ... and adds its products to one fp32 accumulator (from +0) in
 * ascending column order, step after step, one rounding per addition (no fma).  The 64 lanes of a wave then combine in the exchange
 * tree of csrc/moe_gate_score.h - lanes ^ 1, lanes ^ 2, the two quads of a half row, the two halves of a row of 16, the two rows of
 * a pair, the two pairs of a half wave, the two halves - every step adding the same two values in both partners; the four waves
 * combine in wave order through LDS, ((w0 + w1) + w2) + w3.  No atomics: a row's two results depend neither on R nor on the row it
 * sits in, and equal arguments give equal bits.
 * Error account for d_row_weight against the exact sum of the exact products: any order of n - 1 fp32 additions of n terms gives
 *   |d_row_weight[r] - ref| <= gamma_(K-1) * sum over k of |dHp[r, k] * H[r, k]|,   gamma_n = n 2^-24 / (1 - n 2^-24);
 * this order's depth is 8 ceil(K / 2048) + 8, so gamma of that depth holds as well.  dH carries the one rounding to T.
 * Non-finite operands propagate by IEEE rules: a NaN in a served row reaches that row's d_row_weight and the dH elements it
 * multiplies, and no other row.  The host reads no operand; the grid is R workgroups (hipGraph-capturable); 64-bit element
 * offsets; 16-byte loads and stores (csrc/router_grad.hip).
 * Refusals in this order, before anything is enqueued: FLUTE_ERR_DTYPE; FLUTE_ERR_SHAPE (a negative R or K, a negative E with
 * offsets given, K % 8); R == 0 or K == 0 returns FLUTE_OK without a launch; then FLUTE_ERR_NULL (dHp, H, d_row_weight; row_weight
 * without dH or dH without row_weight). */
int flute_moe_weight_grad(int dtype, int R, int K, int E, const void* dHp, const void* H, const float* row_weight,
                          const int32_t* offsets, float* d_row_weight, void* dH, void* stream);

/* The backward of the four gating entries (flute_moe_gate, _route, _limited, _route_limited) in ONE launch: d_logits [T, E] in the
 * logits' type from logits [T, E], the forward's ids [T, k] int32 held fixed, and the gradients that reach the weights.  The bias
 * and the groups enter the choice only, so neither is an argument.  The incoming gradient of slot (t, j) is
 *   q_j = (d_weights ? d_weights[t, j] : 0)  +  (pos && 0 <= pos[t, j] < T k ? d_row_weight[pos[t, j]] : nothing)
 * d_weights [T, k] fp32 or NULL; d_row_weight [T k] fp32 and pos [T, k] int32 (flute_moe_route's: row_weight is a permutation of the
 * weights) both given or both NULL; at least one source is given.  The scores s_e are recomputed from the logits by the forward's
 * own device function (csrc/moe_gate_score.h, gate_scores): the softmax over all E - also where the forward renormalised the u_e
 * directly - or the sigmoid.  Everything in fp32, every operation rounded once, no fma.  With s_j = s_(ids[t, j]); a slot whose id
 * is outside [0, E) is skipped in every sum, and nothing outside the token's rows is read:
 *   not renormalize:  ds_j = scale * q_j
 *   renormalize:      S = sum_j s_j;  w_j = s_j / S;  B = sum_j q_j * w_j;  ds_j = (scale * (q_j - B)) / S      plain running sums
 *                                                                                                              from +0 in slot order
 *   ds_e = sum over the slots j with ids[t, j] == e, in slot order, of ds_j      (+0 for an expert no slot names; equal ids add)
 *   FLUTE_GATE_SIGMOID:  dx_e = (ds_e * s_e) * (1 - s_e)
 *   FLUTE_GATE_SOFTMAX:  dx_e = s_e * (ds_e - D),  D = sum_e ds_e * s_e: lane l adds its experts l, l + 64, ... in ascending order
 *                        from +0, the lanes combine in the exchange tree
 *   d_logits[t, e] = round to the logits' type (dx_e)      for every e < E: every element is written
 * Error account, against the formula in exact arithmetic on the same inputs, to first order, eps = 2^-24: s_e carries the forward's
 * error (expf within 2 eps, the sum over E, one quotient: (4 + log2-depth of the sum) eps relative); S and B are running sums of
 * k terms, (k - 1) eps of their absolute sums; ds_j adds three roundings, dx_e three more.  There is no bound relative to |dx_e|
 * alone - q_j - B and ds_e - D cancel - so the tests measure the error relative to max |d_logits| against the torch fp32 backward's.
 * Limits: flute_moe_gate's.  One wave per token, lane l holding experts l, l + 64, ...; the sums over the slots are wave-uniform
 * loops on values fetched by v_readlane; no LDS, no atomics, plain vector stores.  A non-finite row gives what the arithmetic gives
 * and touches no other token.  The host reads nothing, the grid follows from T alone (hipGraph-capturable); equal arguments give
 * equal bits, and a token's result depends neither on T nor on the row it sits in.
 * Refusals in this order, before anything is enqueued: FLUTE_ERR_DTYPE (logit_dtype, then scoring); FLUTE_ERR_SHAPE (flute_moe_gate's
 * conditions); T == 0 returns FLUTE_OK without a launch; then FLUTE_ERR_NULL (logits, ids, d_logits; neither gradient source given;
 * one of d_row_weight / pos without the other). */
int flute_moe_gate_grad(int logit_dtype, int T, int E, int k, int scoring, int renormalize, float scale, const void* logits,
                        const int32_t* ids, const float* d_weights, const float* d_row_weight, const int32_t* pos, void* d_logits,
                        void* stream);

/* The router's auxiliary losses and the per-expert load, natively (csrc/moe_aux.hip): what a trained router is regularised with.
 * Inputs: logits [T, E] fp16 / bf16 / fp32; ids [T, k] int32, the forward's picks, held fixed; scoring FLUTE_GATE_SOFTMAX or
 * FLUTE_GATE_SIGMOID.  Limits, the gating's own: 1 <= k <= min(E, FLUTE_MOE_GATE_MAX_TOPK), E <= FLUTE_MOE_ROUTE_MAX_EXPERTS,
 * T k < FLUTE_MOE_ROUTE_MAX_PAIRS, and T >= 1 (the losses divide by T).
 * Per token t, in fp32 by csrc/moe_gate_score.h (gate_scores and gate_score_sums; one wave per token, fixed reduction order):
 *   m_t = max_e x_te;  u_te = exp(x_te - m_t);  S_t = sum_e u_te;  sm_te = u_te / S_t (the softmax);  lse_t = m_t + log(S_t)
 *   FLUTE_GATE_SOFTMAX:  p_te = sm_te, bit for bit gate_scores(..., normalise = true)
 *   FLUTE_GATE_SIGMOID:  s_te = 1 / (1 + exp(-x_te));  p_te = s_te / sum_j s_tj
 * lse_t is over the logits for either scoring.
 * Outputs of flute_moe_aux_loss:
 *   load [E] int32        the number of slots (t, j) with ids[t, j] == e; an id outside [0, E) counts nowhere: exactly the differences
 *                         of flute_moe_route's offsets on the same ids.  DeepSeek-V3's aux-loss-free balancing updates the gating's
 *                         `bias` from it (the rule itself is two tensor operations and is not part of this library)
 *   importance [E] fp32   sum_t p_te
 *   losses[0] = balance   E * sum_e (load_e / T) * (importance_e / T): the load-balance loss of Switch / Mixtral - Hugging Face's
 *                         load_balancing_loss_func without an attention mask.  DeepSeek's is this divided by k
 *   losses[1] = z         (1 / T) * sum_t lse_t^2: the router z-loss of ST-MoE
 * Two launches.  (1) grid C = ceil(T / chunk_tokens): workgroup c of 4 waves owns the tokens [c chunk_tokens, (c + 1) chunk_tokens)
 * cut at T; wave w takes its tokens w, w + 4, ... in ascending order and keeps the running sums of p in registers (lane l: experts
 * l, l + 64, ...) and of lse^2; the four waves combine in wave order through LDS, ((w0 + w1) + w2) + w3; the chunk's slots are
 * counted with integer atomics in LDS; the chunk writes its whole row of the workspace - E fp32 sums, E int32 counts (zeros
 * included), one fp32 sum of lse^2 - with plain stores.  (2) one workgroup: per expert the chunks' sums are added in ascending chunk
 * order in fp64 and rounded once (importance), the counts as integers (load); balance = E * (sum over e ascending of
 * (double) load_e * importance_e's fp64 sum) / T^2 and z = (sum over c ascending of the chunks' lse^2) / T in fp64, each rounded
 * once.  Every output word is written.  No float atomics, no workgroup waits on another, the host reads nothing (stream-ordered,
 * hipGraph-capturable); equal arguments give equal bits; the workspace need not be cleared.  load does not depend on chunk_tokens.
 * chunk_tokens: 0 = automatic, max(FLUTE_MOE_AUX_CHUNK_TOKENS, ceil(T / FLUTE_MOE_AUX_AUTO_CHUNKS)), from T alone; a positive value
 * is honoured where C <= FLUTE_MOE_ROUTE_MAX_CHUNKS (for tests and sweeps).  workspace: flute_moe_aux_loss_workspace(T, E,
 * chunk_tokens) = C (2 E + 1) 4 bytes - psum [C][E] fp32, pcnt [C][E] int32, pz [C] fp32; 0 for arguments the call refuses.
 * Non-finite logits: a NaN in token t makes importance, balance and z NaN and leaves load alone; a logit of -infinity is a masked
 * expert, p = +0.
 * Refusals of flute_moe_aux_loss in this order, before anything is enqueued: FLUTE_ERR_DTYPE (logit_dtype, then scoring);
 * FLUTE_ERR_SHAPE (T < 1, the gating's conditions on k and E, T k, chunk_tokens < 0, C > FLUTE_MOE_ROUTE_MAX_CHUNKS); then
 * FLUTE_ERR_NULL (logits, ids, workspace, load, importance, losses).
 *
 * flute_moe_aux_loss_grad: the backward with respect to the logits - load is a constant - in ONE launch, one wave per token:
 * d_logits [T, E] in the logits' type from logits, load [E] int32 and grads [2] fp32 ON THE DEVICE = (g_b, g_z), the incoming
 * gradients of balance and z (no host synchronise).  In fp32, every operation rounded once, no fma; sums over e: lane l adds its
 * experts in ascending order from +0, then the exchange tree:
 *   a_e = (g_b * (E / (T * T))) * load_e;   D_t = sum_e a_e * p_te;   zc_t = (g_z * (2 / T)) * lse_t
 *   FLUTE_GATE_SOFTMAX:  dx_te = p_te * (a_e - D_t) + zc_t * p_te
 *   FLUTE_GATE_SIGMOID:  dx_te = (s_te * (1 - s_te)) * ((a_e - D_t) / sum_j s_tj) + zc_t * sm_te
 *   d_logits[t, e] = round to the logits' type (dx_te + 0): every element is written, and a zero is +0
 * A token's result depends on its own logits, load, grads, T and E only; a NaN row touches no other token.  In fp16 the loss
 * gradients, of order E / T^2, fall into the subnormal range: use fp32 or bf16 logits where the losses train.
 * Refusals in this order: FLUTE_ERR_DTYPE (logit_dtype, then scoring); FLUTE_ERR_SHAPE (T < 1, E < 1, E > FLUTE_MOE_ROUTE_MAX_EXPERTS,
 * T >= FLUTE_MOE_ROUTE_MAX_PAIRS); then FLUTE_ERR_NULL (logits, load, grads, d_logits).
 * Out of scope: token masks and padding weights, sequence-wise losses per batch row, folding this backward into
 * flute_moe_gate_grad's launch, and the bias update rule. */
#define FLUTE_MOE_AUX_CHUNK_TOKENS 32
#define FLUTE_MOE_AUX_AUTO_CHUNKS 2048
size_t flute_moe_aux_loss_workspace(int T, int E, int chunk_tokens);
int flute_moe_aux_loss(int logit_dtype, int T, int E, int k, int scoring, int chunk_tokens, const void* logits, const int32_t* ids,
                       void* workspace, int32_t* load, float* importance, float* losses /* [2]: balance, z */, void* stream);
int flute_moe_aux_loss_grad(int logit_dtype, int T, int E, int scoring, const void* logits, const int32_t* load, const float* grads,
                            void* d_logits, void* stream);

/* Template table (replaces data/qgemm_kernel_raw_generated_configs.pth +
 * the generated switch, qgemm_kernel_raw_generated.cu:92-767). */
int flute_num_templates(int num_bits);
int flute_get_template_info(int num_bits, int template_id, flute_template_info* out);

/* Calibration only: stream `bytes` from `src` with the decode kernel's access shape and
 * no arithmetic (what the HBM path alone costs for a given byte count). */
int flute_debug_stream_read(const void* src, void* sink, size_t bytes, int bytes_per_wave,
                            int grid, int block, void* stream);

/* Measurement only: enqueue a one-lane kernel that writes the chip-wide 100 MHz clock (ticks of 10 ns) to the
 * 8 bytes at `dst` (device memory).  Capturable into a hipGraph: two of them bracket exactly the launches between. */
int flute_debug_timestamp(void* dst, void* stream);

const char* flute_strerror(int status);
int flute_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLUTE_AMD_H */
