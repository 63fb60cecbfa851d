// The one internal header of the host side of the C ABI: what more than one of the host units (planner_decode.hip, planner.hip,
// api.hip, api_train.hip) needs, and nothing else.  Host only: no instantiation unit, kernel header or device unit includes it.
#pragma once
#include "../../include/flute_amd.h"
#include "qgemm_stream.h"

namespace flute_amd::host {

// had8: set by flute_qgemm_hadamard for M <= 4 - the DECODE planners then prefer 8-wave workgroups (the fused rotation is
// done by the workgroup's waves, 512 k each); it never reaches the MFMA planners, whose wave count is the template's
struct Ovr { int family, m_block, waves, kw, splitk, m_tiles, slabs, depth, one_shot, had8; };
inline Ovr ovr_of(const flute_overrides* o) {
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

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline int floor_pow2(int v) { int p = 1; while (p * 2 <= v) p *= 2; return p; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
// rows of a block-kernel configuration (flute_plan::m_block of family 3): 4 / 5 = 256 / 128 rows,
// 8 + RT = the skinny 3-bit blocks of RT row tiles
inline int block_rows(int cfg) { return cfg >= 8 ? (cfg - 8) * 16 : ((cfg & 1) ? 128 : 256); }

// What every entry point checks of a layer (check_layer), and one planner call: the layer, the shape, the CU count, the workspace
// and the overrides.
struct Layer { int bits, lg, J, units; flute_template_info t; };
struct Call : Layer { int dtype, M, N, K, template_id, num_sms; size_t workspace_bytes; Ovr ov; };
struct OneArgs { int lg, lkw, upw, pk, ipw, depth, pipe, nvis, nch, nwg, nsets; };

// A plan, the launch arguments the decode kernels take beside it, and its kernel (resolve_kernel): fn_had is the member that rotates
// the activations while it stages them, where that is an instantiation of its own (one-shot and persistent one-shot kernels; else null).
struct Planned { flute_plan p; OneArgs oa; StreamArgs sa; const void* fn; const void* fn_had; };

// planner.hip
bool decode_template(int bits, int id, flute_template_info* t);
int check_layer(int bits, int group, int template_id, int N, int K, int k_align, Layer* l);
int make_plan(int dtype, int bits, int group, int M, int N, int K, int template_id, int num_sms,
              size_t workspace_bytes, const Ovr& ov, Planned* out);

// planner_decode.hip, for planner.hip: the room behind the workspace's state words, each family's kernel lookup (nullptr: not
// built) and the shape planners
size_t slab_room(size_t workspace_bytes);
const void* stream_fn(const Call& c, int mb, int depth);
const void* oneshot_fn(const Call& c, int mb, int depth, int had, int pipe);
const void* persist_fn(const Call& c, int mb, int depth, int nsets, int had);
const void* fast_fn(const Call& c, int waves, int kw, int depth, int mb);
const void* fastm_fn(const Call& c, int waves, int nm, int lg, int ng);
const void* persistm_fn(const Call& c, int lg, int ng, int xr, int waves, int xres);
const void* skinny_fn(const Call& c, int depth);
const void* splitk_fn(const Call& c, int rt, int kp);
const void* block_fn(const Call& c, int cfg);
const void* tile_fn(const Call& c, int r, int mt, int sw);
int plan_oneshot(const Call& c, const Ovr& ov, flute_plan* p, OneArgs* oa);
int plan_fast(const Call& call, int rank, int want_waves, flute_plan* p, OneArgs* oa);
int plan_fastm(const Call& c, int ng_ovr, flute_plan* p, OneArgs* oa);
int plan_persistm(const Call& c, int ng_ovr, int visits_ovr, int xres_ovr, flute_plan* p, OneArgs* oa);
int plan_persist(const Call& c, const Ovr& ov, flute_plan* p, OneArgs* oa);
int plan_skinny(const Call& c, const Ovr& ov, flute_plan* p, OneArgs* ka);
int plan_splitk(int bits, int lg, int M, int N, int K, int num_sms, const Ovr& ov, size_t workspace_bytes, flute_plan* p,
                int rank = 0, double* cost_us = nullptr);
int plan_stream(int dtype, int bits, int lg, int M, int N, int K, int num_sms, const flute_template_info& t,
                const Ovr& ov, size_t workspace_bytes, flute_plan* p, StreamArgs* sa);

}  // namespace flute_amd::host
