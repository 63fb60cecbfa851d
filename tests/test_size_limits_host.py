"""Every size guard of the planner (csrc/planner.hip, csrc/planner_decode.hip), pinned at both edges.  No GPU.

The decode, prefill and MFMA decode kernels address the activations, the weights, the scales and their split-K
slabs through buffer descriptors: a 32-bit byte range and 32-bit offsets.  The planner admits a kernel only while
its largest offset stays below that range.  Past it, families 6 and 8 refuse the call (FLUTE_ERR_SHAPE); the
others, the decode kernels (family 0) included, fall back to the per-wave kernel (family 2, qgemm_tile.h), which
addresses memory through 64-bit pointers; K slices met inside the launch fall back to the reduce launch.  A guard
that moved by one row or one column would let a kernel wrap its offsets and silently corrupt the rows or columns
beyond 2 or 4 GiB, at shapes no GPU test can allocate; planning them costs nothing.

Each edge records the guard (file and function or variable), the descriptor or offset it protects, the largest shape it admits
and the smallest it refuses, and checks the guarded byte count on both sides of its limit.
tests/test_long_prefill_gpu.py runs the reachable edges on the GPU.
"""
from collections import namedtuple

import pytest

from flute_amd import TEMPLATE_CONFIGS, _lib
from tests.qgemm_cases import SUPPORTED_SHAPES

LIMIT = 0xFFFFFFF0              # the largest byte range the kernels give a descriptor
SLAB_LIMIT = 1 << 31            # in-launch split-K slabs (xwg.h: xwg_rsrc)
TILE_INLAUNCH_MAX = 4 << 20     # host.h kTileInLaunchMax
XWG_MAX_TILES = (64 << 10) // 8  # xwg.h kXwgMaxTiles
BIG_WS = 1 << 40                # a workspace that never limits a split: the size guards alone decide
WS = 64 << 20                   # what utils.make_workspace_streamk allocates
ERR_SHAPE = -4


def tid_for(bits):
    """The first TileP-32 template of a bit width (its automatic ids for 4 bits: QuantMapMode digit 0)."""
    return min(t for (b, t), c in TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)


def plan(M, N, K, bits=4, g=64, dtype=0, ws=BIG_WS, sms=256, **ovr):
    p = _lib.Plan()
    o = _lib.Overrides(**ovr) if ovr else None
    rc = _lib.get().flute_qgemm_plan_ex(dtype, bits, g, M, N, K, tid_for(bits), sms, ws, o, p)
    return rc, p


# ---------------------------------------------------------------------------
# x32_ok (planner.hip choose_block): the block kernels' activation descriptor and offsets - qgemm_block2.h:97 (x_srd),
# :111 (x_vo), qgemm_block3.h:96, :109.  A block reads up to 256 rows from its first row, so the largest byte
# offset is below (M + 256) K 2.  Largest admitted M = (LIMIT - 1) // (2 K) - 256; the next M is refused and a
# forced family 3 falls back to family 2.
# ---------------------------------------------------------------------------

X32_EDGES = {4096: 524031, 8192: 261887, 14336: 149540, 28672: 74642}


@pytest.mark.parametrize("K", sorted(X32_EDGES))
@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("dtype", [0, 1])
def test_block_activation_offsets_edge(K, bits, dtype):
    M = X32_EDGES[K]
    assert M == (LIMIT - 1) // (2 * K) - 256
    assert (M + 256) * K * 2 < LIMIT <= (M + 257) * K * 2
    N = 1024
    variants = [(dict(m_tiles=8), 4), (dict(m_tiles=4), 5)]            # 256- / 128-row blocks
    if bits == 3:
        variants.append((dict(m_block=1), 9))                        # qgemm_block3.h's 16-row blocks (some waves idle)
    for ovr, cfg in variants:
        rc, p = plan(M, N, K, bits, dtype=dtype, family=3, **ovr)
        assert rc == 0 and (p.family, p.m_block) == (3, cfg), (K, bits, ovr, p.as_dict())
        rc, p = plan(M + 1, N, K, bits, dtype=dtype, family=3, **ovr)
        assert rc == 0 and p.family == 2, (K, bits, ovr, p.as_dict())
    for ws in (WS, BIG_WS):
        rc, p = plan(M + 1, N, K, bits, dtype=dtype, ws=ws)
        assert rc == 0 and p.family != 3, (K, bits, p.as_dict())


# ---------------------------------------------------------------------------
# The other guards: one edge each.  `over` is the guarded byte count, `limit` what it must stay below.
# ---------------------------------------------------------------------------

Edge = namedtuple("Edge", "guard protects bits g dtype admitted refused ovr over limit admitted_plan refused_plan")


def _q3(M, N, K, g):
    return 3 * (N // 16) * K * 2


def _scales(M, N, K, g):
    return N * (K // g) * 2


EDGES = {
    # one descriptor over all three planes of the 3-bit weights: qgemm_block3.h:97 (w_srd), :114 (wv_p1)
    "block3_weights": Edge("planner.hip choose_block: b3_ok", "qgemm_block3.h:97,114", 3, 64, 1,
                           (4096, 1397760, 8192), (4096, 1398272, 8192), dict(family=3), _q3, LIMIT,
                           dict(family=3), dict(family=2)),
    # the 2- / 4-bit block kernels' scale descriptor: qgemm_block2.h:99 (s_srd), :119 (s_voff)
    "block2_scales_b4": Edge("planner.hip choose_block: s32_ok", "qgemm_block2.h:99,119", 4, 32, 0,
                             (4096, 1048320, 65536), (4096, 1048576, 65536), dict(family=3), _scales, LIMIT,
                             dict(family=3), dict(family=2)),
    "block2_scales_b2": Edge("planner.hip choose_block: s32_ok", "qgemm_block2.h:99,119", 2, 32, 1,
                             (4096, 1048320, 65536), (4096, 1048576, 65536), dict(family=3), _scales, LIMIT,
                             dict(family=3), dict(family=2)),
    # the decode kernels' scale descriptor (planner.hip decode_fits, taken before any decode planner; the lean kernel's own
    # clause in planner_decode.hip plan_fast is the same bound): the ring kernel qgemm_stream.h:271,302, the one-shot kernel qgemm_oneshot.h:400,411,
    # the persistent one-shot kernel qgemm_persist.h:96,114, the lean kernel qgemm_fast.h:225
    "decode_ring_scales": Edge("planner.hip decode_fits", "qgemm_stream.h:271,302", 4, 64, 0,
                               (4, 67108736, 2048), (4, 67108864, 2048), dict(family=0, one_shot=0), _scales, LIMIT,
                               dict(family=0, one_shot=0), dict(family=2)),
    "decode_ring_scales_b3": Edge("planner.hip decode_fits", "qgemm_stream.h:271,302", 3, 64, 1,
                                  (2, 33553920, 4096), (2, 33554432, 4096), dict(family=0, one_shot=0), _scales, LIMIT,
                                  dict(family=0, one_shot=0), dict(family=2)),
    "decode_oneshot_scales": Edge("planner.hip decode_fits", "qgemm_oneshot.h:400,411", 4, 64, 0,
                                  (1, 67108736, 2048), (1, 67108864, 2048), dict(family=0, one_shot=1), _scales, LIMIT,
                                  dict(family=0, one_shot=1), dict(family=2)),
    "decode_oneshot_scales_b2": Edge("planner.hip decode_fits", "qgemm_oneshot.h:400,411", 2, 64, 1,
                                     (1, 33554176, 4096), (1, 33554432, 4096), dict(family=0, one_shot=1), _scales, LIMIT,
                                     dict(family=0, one_shot=2), dict(family=2)),
    "decode_persist_scales": Edge("planner.hip decode_fits", "qgemm_persist.h:96,114", 4, 64, 0,
                                  (2, 67108736, 2048), (2, 67108864, 2048), dict(family=0, one_shot=2), _scales, LIMIT,
                                  dict(family=0, one_shot=3), dict(family=2)),
    "decode_persist_scales_auto": Edge("planner.hip decode_fits", "qgemm_persist.h:96,114", 4, 256, 1,
                                       (1, 67108736, 8192), (1, 67108864, 8192), dict(), _scales, LIMIT,
                                       dict(family=0, one_shot=3), dict(family=2)),
    "lean_decode_scales": Edge("planner.hip decode_fits", "qgemm_fast.h:225", 4, 64, 0,
                               (1, 67108736, 2048), (1, 67108864, 2048), dict(family=0, one_shot=4), _scales, LIMIT,
                               dict(family=0, one_shot=4), dict(family=2)),
    "lean_decode_scales_g256": Edge("planner.hip decode_fits", "qgemm_fast.h:225", 4, 256, 1,
                                    (2, 67108736, 8192), (2, 67108864, 8192), dict(family=0, one_shot=4), _scales, LIMIT,
                                    dict(family=0, one_shot=4), dict(family=2)),
    # the lean MFMA decode kernel's scale descriptor: qgemm_fastm.h:117 (s_srd)
    "lean_mfma_scales": Edge("planner_decode.hip plan_fastm", "qgemm_fastm.h:117", 4, 64, 0,
                             (16, 33554304, 4096), (16, 33554432, 4096), dict(family=7), _scales, LIMIT,
                             dict(family=7), dict(family=2)),
    # the persistent MFMA decode kernel's weight descriptor: qgemm_persistm.h:135 (q_srd)
    "persistent_mfma_weights_b4": Edge("planner_decode.hip plan_persistm", "qgemm_persistm.h:135", 4, 64, 0,
                                       (16, 1048448, 8192), (16, 1048576, 8192), dict(family=8),
                                       lambda M, N, K, g: N * K * 4 // 8, LIMIT, dict(family=8), None),
    "persistent_mfma_weights_b2": Edge("planner_decode.hip plan_persistm", "qgemm_persistm.h:135", 2, 128, 1,
                                       (4, 2096896, 8192), (4, 2097152, 8192), dict(family=8),
                                       lambda M, N, K, g: N * K * 2 // 8, LIMIT, dict(family=8), None),
    # the skinny MFMA kernel's weight descriptor: qgemm_skinny.h:127 (q_srd over units x K x 2 bytes)
    "skinny_weights": Edge("planner_decode.hip plan_skinny", "qgemm_skinny.h:127", 4, 64, 0,
                           (16, 2097024, 4096), (16, 2097152, 4096), dict(family=5),
                           lambda M, N, K, g: N // 4 * K * 2, LIMIT, dict(family=5), dict(family=2)),
    # the skinny kernel's in-launch K split: its slab descriptor (qgemm_skinny.h:329) is bounded through the tile count
    # (planner_decode.hip plan_skinny, units / 16 <= kXwgMaxTiles; the 2^31 clause beside it then always holds - test_dominated_clauses)
    "skinny_split_tiles": Edge("planner_decode.hip plan_skinny: kXwgMaxTiles", "qgemm_skinny.h:329", 4, 64, 0,
                               (16, 524288, 8192), (16, 524288 + 128, 8192), dict(family=5, splitk=2),
                               lambda M, N, K, g: N // 64, XWG_MAX_TILES + 1, dict(family=5, splitk=2), dict(family=2)),
    # the split-K block kernel's activation descriptor and offsets (rows of a 128-row tile): qgemm_splitk.h:213 (x_srd), :265 (lx)
    "splitk_activations": Edge("planner_decode.hip plan_splitk", "qgemm_splitk.h:213,265", 4, 64, 0,
                               (524159, 256, 4096), (524160, 256, 4096), dict(family=6, m_tiles=8, kw=2, splitk=1),
                               lambda M, N, K, g: (M + 128) * K * 2, LIMIT, dict(family=6, splitk=1), None),
    "splitk_activations_deep": Edge("planner_decode.hip plan_splitk", "qgemm_splitk.h:213,265", 2, 64, 1,
                                    (74770, 256, 28672), (74771, 256, 28672), dict(family=6, m_tiles=8, kw=2, splitk=7),
                                    lambda M, N, K, g: (M + 128) * K * 2, LIMIT, dict(family=6, splitk=7), None),
    # the split-K block kernel's in-launch slabs ([splitk][tile] 64 KB each): qgemm_splitk.h:574 (xwg_rsrc)
    "splitk_slabs": Edge("planner_decode.hip plan_splitk: legal", "qgemm_splitk.h:574", 4, 64, 0,
                         (1048448, 128, 1536), (1048449, 128, 1536), dict(family=6, m_tiles=8, kw=2, splitk=4),
                         lambda M, N, K, g: 4 * -(-M // 128) * (N // 128) * 65536, SLAB_LIMIT,
                         dict(family=6, splitk=4, splitk_mode=1), None),
    # 3-bit 128-row blocks x K slices met in the launch: the slab descriptor of xwg.h:145; beyond it the reduce launch
    "block3_inlaunch_slabs": Edge("planner.hip plan_block", "xwg.h:145", 3, 64, 1,
                                  (524160, 512, 2048), (524161, 512, 2048), dict(family=3, m_tiles=4, splitk=2),
                                  lambda M, N, K, g: 2 * -(-M // 128) * (N // 256) * 128 * 1024, SLAB_LIMIT,
                                  dict(family=3, m_block=5, splitk=2, splitk_mode=1), dict(family=3, m_block=5, splitk=2, splitk_mode=0)),
    # the per-wave kernel's in-launch slabs: qgemm_tile.h:580 (xwg_rsrc over splitk x M x N x 4 bytes), kTileInLaunchMax
    "tile_inlaunch_slabs": Edge("planner.hip plan_tile", "qgemm_tile.h:580", 4, 64, 0,
                                (512, 1024, 4096), (513, 1024, 4096), dict(family=2, splitk=2),
                                lambda M, N, K, g: 2 * M * N * 4, TILE_INLAUNCH_MAX + 1,
                                dict(family=2, splitk=2, splitk_mode=1), dict(family=2, splitk=2, splitk_mode=0)),
}

# the family (and variant) a guard keeps the automatic planner from, at its refused edge
GUARDED = {"block3_weights": (3,), "block2_scales_b4": (3,), "block2_scales_b2": (3,), "decode_ring_scales": (0,),
           "decode_ring_scales_b3": (0,), "decode_oneshot_scales": (0,), "decode_oneshot_scales_b2": (0,),
           "decode_persist_scales": (0,), "decode_persist_scales_auto": (0,), "lean_decode_scales": (0,),
           "lean_decode_scales_g256": (0,), "lean_mfma_scales": (7,), "persistent_mfma_weights_b4": (8,),
           "persistent_mfma_weights_b2": (8,), "skinny_weights": (5,), "skinny_split_tiles": (5,),
           "splitk_activations": (6,), "splitk_activations_deep": (6,), "splitk_slabs": (6,)}


def _matches(p, want):
    return all(getattr(p, k) == v for k, v in want.items())


@pytest.mark.parametrize("name", sorted(EDGES))
def test_guard_edge(name):
    e = EDGES[name]
    (Ma, Na, Ka), (Mr, Nr, Kr) = e.admitted, e.refused
    assert e.over(Ma, Na, Ka, e.g) < e.limit <= e.over(Mr, Nr, Kr, e.g), name      # the edge is where the guard says
    rc, p = plan(Ma, Na, Ka, e.bits, e.g, e.dtype, **e.ovr)
    assert rc == 0 and _matches(p, e.admitted_plan), (name, rc, p.as_dict())
    rc, p = plan(Mr, Nr, Kr, e.bits, e.g, e.dtype, **e.ovr)
    if e.refused_plan is None:                                   # families 6 and 8: refused, not replaced
        assert rc == ERR_SHAPE, (name, rc, p.as_dict())
    else:
        assert rc == 0 and _matches(p, e.refused_plan), (name, p.as_dict())
    if name in GUARDED:
        fam = GUARDED[name]
        for ws in (WS, BIG_WS):
            rc, p = plan(Mr, Nr, Kr, e.bits, e.g, e.dtype, ws=ws)
            assert rc == 0 and (p.family, p.one_shot)[:len(fam)] != fam, (name, ws, p.as_dict())


def test_dominated_clauses():
    """The guard clauses that can never be the first to refuse a legal call, and why."""
    # planner_decode.hip plan_fast, the lean decode kernel's scale clause: decode_fits (planner.hip) applies the same bound before any decode planner
    # planner_decode.hip plan_fast / plan_fastm, units K 2 >= 2^40: the scale clause beside it refuses first - N (K / g) 2 < LIMIT gives
    # units K 2 = N K / 2 < LIMIT g / 4, and g <= 256
    assert LIMIT * 256 // 4 < 1 << 40
    # planner_decode.hip plan_persistm, the scales and the activations: the weight clause refuses first.  Weights >= 8 x scale bytes (bits / 8 >=
    # 2 / 64); weights >= 2 x activation bytes (N >= 128 (4 bits) / 256 (2 bits) columns, M <= 16 rows: N bits / 8 >= 64 >= 2 M 2)
    for bits, n_min in ((4, 128), (2, 256)):
        assert bits * 8 >= 2 * 64 // 8 and n_min * bits // 8 >= 2 * 16 * 2
        rc, _ = plan(16, n_min, (1 << 27) - 128, bits, 64, family=8)   # activations 2^32 - 8 KB: the weights alone are 2^33
        assert rc == ERR_SHAPE
    # planner_decode.hip plan_skinny, (M + 16) K 2 < 0x7ffffff0: the skinny kernel's K is at most 16 slices x 4096 (K = slices x 32 x depth x waves)
    assert (16 + 16) * 65536 * 2 < 0x7FFFFFF0
    rc, p = plan(16, 1024, 131072, 4, 64, family=5, splitk=16)
    assert rc == 0 and p.family == 2
    # planner_decode.hip plan_skinny, slabs >= 2^31: at most 16 slices x kXwgMaxTiles slabs of 4 KB
    assert 16 * XWG_MAX_TILES * 4096 < SLAB_LIMIT
    # planner_decode.hip plan_splitk, the split-K block kernel's scales: at most kXwgMaxTiles column tiles of 128 and 64 groups per slice x 16 slices
    assert XWG_MAX_TILES * 128 * (64 * 16) * 2 < LIMIT


def _bounds_ok(p, M, N, K, bits, g):
    """The byte ranges the planned kernel addresses through 32-bit descriptors, all within their limits."""
    G = K // g
    f = p.family
    if f == 3:
        ok = (M + 256) * K * 2 < LIMIT and N * G * 2 < LIMIT and (bits != 3 or 3 * (N // 16) * K * 2 < LIMIT)
        return ok and (p.splitk_mode == 0 or p.workspace_needed - (64 << 10) < SLAB_LIMIT)
    if f == 5:
        return N // 4 * K * 2 < LIMIT and (M + 16) * K * 2 < 0x7FFFFFF0 and p.workspace_needed < SLAB_LIMIT
    if f == 6:
        return (M + 128) * K * 2 < LIMIT and N * G * 2 < LIMIT and p.workspace_needed < SLAB_LIMIT
    if f == 8:
        return N * K * bits // 8 < LIMIT and N * G * 2 < LIMIT and M * K * 2 < LIMIT
    if f in (0, 7):                                                # every decode kernel: one descriptor over the scales
        return N * G * 2 < LIMIT
    if f == 2 and p.splitk_mode == 1:
        return p.splitk * M * N * 4 <= TILE_INLAUNCH_MAX
    return True


SWEEP_MS = sorted({1, 2, 3, 4, 5, 8, 16, 17, 33, 64, 128, 129, 256, 512, 1024, 4096, 16384, 37449, 37450, 65536, 74642,
                   74643, 74899, 76000, 131072, 149540, 149541, 261887, 261888, 262144, 524031, 524032, 524160, 524161,
                   1 << 20})


def test_automatic_plans_within_descriptor_bounds():
    """The automatic planner over the reference's SUPPORTED_SHAPES x M up to 2^20 x 2 / 3 / 4 bits x both dtypes x two
    workspaces: no plan of the descriptor-addressed families (3, 5, 6, 7, 8, the lean decode kernel, in-launch slabs)
    breaks its bound, and the block kernels give way to the per-wave kernel past x32_ok."""
    seen = {}
    for (N, K) in SUPPORTED_SHAPES:
        for bits in (2, 3, 4):
            if N % (32 * (16 if bits == 3 else 16 // bits)):
                continue
            for g in (64, 128):
                for dtype in (0, 1):
                    for ws in (WS, BIG_WS):
                        for M in SWEEP_MS:
                            rc, p = plan(M, N, K, bits, g, dtype, ws=ws)
                            assert rc == 0, (M, N, K, bits, g, dtype, rc)
                            what = (M, N, K, bits, g, dtype, ws, p.as_dict())
                            assert _bounds_ok(p, M, N, K, bits, g), what
                            if (M + 256) * K * 2 >= LIMIT:
                                assert p.family == 2, what
                            seen[p.family] = seen.get(p.family, 0) + 1
    assert {0, 2, 3, 6, 8} <= set(seen), seen
