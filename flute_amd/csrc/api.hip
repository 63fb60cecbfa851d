// Host side of the C ABI (include/flute_amd.h), the launch path: the dense qgemm entry points, the template and plan queries,
// flute_hadamard / _unpack / _dequantize and the debug entries.  Mirrors the role of flute/csrc/qgemm.cpp:39-83 (qgemm_raw) +
// qgemm_kernel_raw_generated.cu:15-768 (_qgemm_raw's template switch) + qgemm_kernel.hpp:824-939 (qgemm_host), re-thought for
// gfx950: a call is planned (planner.hip, planner_decode.hip: make_plan, host.h), then its kernel's arguments are packed and the
// kernel launched here.  The training entry points are api_train.hip's, the MoE ones api_moe.hip's.  Nothing on the host side is
// process-global mutable state except the per-device "large LDS granted" cache below (mutex-guarded): plan overrides travel with the call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <mutex>
#include <stdint.h>
#include <string.h>

#include "host.h"
#include "kernels.h"
#include "qgemm_persist.h"
#include "qgemm_skinny.h"
#include "qgemm_tile.h"
#include "qgemm_block.h"
#include "qgemm_splitk.h"

using namespace flute_amd;
using namespace flute_amd::host;

namespace {

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

// Calls that will fuse the rotation prefer 8-wave workgroups: the rotation is done by the workgroup's waves, 512 k each - 8 waves
// rotate a 4096-k row in one pass (4096x3584 M = 1: 5.5 us with 8 waves, 6.5 with the 4-wave shape the plain product prefers).
// (Applied inside the decode planner only: plan_decode.  Round 3 also forced the four-row decode
// kernel at M = 3, 4 to keep the rotation fused: measured again in round 4, the fused form loses there - above.)
static Ovr hadamard_ovr(Ovr o, int hadamard_size, int M, int K) {
    if (hadamard_size > 1 && hadamard_size <= 512 && M <= 4 && hadamard_worth_fusing(M, K, o.family == 0)) o.had8 = 1;
    return o;
}

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
