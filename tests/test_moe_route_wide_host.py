"""flute_moe_route_wide / flute_moe_gate_route_wide / flute_moe_route_form, their Python wrappers and
FluteExperts(wide_routing=...) without a GPU: the exports, every refusal of the C ABI in the documented order (returned
before anything is enqueued, on null or host pointers), the workspace query, the automatic rule, the signatures, and a numpy
model of the three launches (tests/moe_wide_cases.py) against the routing contract as a host loop - the kernels' index
arithmetic, checked before any GPU run."""
import inspect

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from flute_amd.integrations.moe import FluteExperts, FluteSparseMoeBlock, GroupedFluteLinear
from flute_amd.ops import MOE_ROUTE_MAX_CHUNKS, _validate_chunk_tokens
from tests.moe_wide_cases import (HEADER, ROUTE_WIDE_CASES, auto_chunk, draw_wide_ids, header_constant, host_route,
                                  model_route_wide, wave_range)

OK, ERR_SHAPE, ERR_WORKSPACE, ERR_DTYPE, ERR_NULL = 0, -4, -5, -7, -9
FAKE = 0x1000            # a host address no refusal may look behind
I32, I64 = 0, 1
F16, BF16, F32 = 0, 1, 2
MAX_CHUNKS = header_constant("FLUTE_MOE_ROUTE_MAX_CHUNKS")
# the benchmark's three gatings: (E, k)
GATINGS = [(8, 2), (64, 8), (256, 8)]


def workspace(T=64, k=2, E=8, chunk_tokens=16):
    return _lib.get().flute_moe_route_wide_workspace(T, k, E, chunk_tokens)


def route(id_dtype=I32, weight_dtype=F16, T=64, k=2, E=8, ptrs=(None,) * 7, ws=None, ws_bytes=0, chunk_tokens=16):
    """ptrs: ids, weights, offsets, perm, rows, row_weight, pos"""
    return _lib.get().flute_moe_route_wide(id_dtype, weight_dtype, T, k, E, *ptrs, ws, ws_bytes, chunk_tokens, None)


def gate_route(logit_dtype=F16, T=64, E=8, k=2, n_group=1, topk_group=1, group_score=0, scoring=0, ptrs=(None,) * 9, ws=None,
               ws_bytes=0, chunk_tokens=16):
    """ptrs: logits, bias, ids, weights, offsets, perm, rows, row_weight, pos"""
    return _lib.get().flute_moe_gate_route_wide(logit_dtype, T, E, k, n_group, topk_group, group_score, scoring, 0, 1.0, *ptrs, ws,
                                                ws_bytes, chunk_tokens, None)


def test_symbols_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_moe_route_wide_workspace", "flute_moe_route_wide", "flute_moe_gate_route_wide", "flute_moe_route_form"):
        assert name in _lib.SYMBOLS
        assert " %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert MAX_CHUNKS == MOE_ROUTE_MAX_CHUNKS
    assert flute_amd.moe_route_wide is flute_amd.ops.moe_route_wide
    assert flute_amd.moe_gate_route_wide is flute_amd.ops.moe_gate_route_wide
    assert callable(dev.moe_route_form)


def test_route_wide_refusals_in_order():
    # 1. the one-workgroup entry's, in its order
    for bad in (-1, 2, 3):
        assert route(id_dtype=bad) == ERR_DTYPE, bad
    for bad in (-1, 3):
        assert route(weight_dtype=bad) == ERR_DTYPE, bad
    assert route(id_dtype=2, T=-1) == ERR_DTYPE
    assert route(weight_dtype=3, chunk_tokens=-1) == ERR_DTYPE
    for kw in (dict(T=-1), dict(k=-1), dict(E=-1), dict(E=1025), dict(T=2 ** 26, k=2), dict(T=2 ** 30, k=8)):
        assert route(chunk_tokens=0, **kw) == ERR_SHAPE, kw
    # 2. chunk_tokens, before "nothing to do" and the nulls
    assert route(chunk_tokens=-1) == ERR_SHAPE
    assert route(T=0, chunk_tokens=-1) == ERR_SHAPE
    assert route(T=MAX_CHUNKS + 1, chunk_tokens=1) == ERR_SHAPE
    assert route(T=MAX_CHUNKS, chunk_tokens=1) == ERR_NULL
    assert route(T=2 * MAX_CHUNKS + 1, chunk_tokens=2, ptrs=[FAKE] * 7, ws=FAKE, ws_bytes=2 ** 40) == ERR_SHAPE
    assert route(T=2 ** 27 - 1, k=1, chunk_tokens=0) == ERR_NULL                # the automatic chunk respects the cap
    # 3. nothing to do
    assert route(T=0) == OK
    assert route(k=0) == OK
    assert route(T=0, ptrs=[FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE], ws=FAKE) == OK
    # 4. the nulls, the workspace among them when there is more than one chunk
    assert route() == ERR_NULL
    need = workspace()
    for i in range(7):
        if i == 1:                                               # weights are optional
            continue
        ptrs = [FAKE] * 7
        ptrs[i] = None
        assert route(ptrs=ptrs, ws=FAKE, ws_bytes=need) == ERR_NULL, i
    assert route(ptrs=[FAKE] * 7, ws=None, ws_bytes=need) == ERR_NULL
    assert route(ptrs=[FAKE] * 7, ws=None, ws_bytes=0) == ERR_NULL              # null before too small
    # 5. the workspace too small, by one byte too
    assert need == (4 + 1) * (8 + 1) * 4
    for short in (0, 4, need - 1):
        assert route(ptrs=[FAKE] * 7, ws=FAKE, ws_bytes=short) == ERR_WORKSPACE, short
    assert route(ptrs=[FAKE, None, FAKE, FAKE, FAKE, None, FAKE], ws=FAKE, ws_bytes=need - 1) == ERR_WORKSPACE


def test_gate_route_wide_refusals_in_order():
    for bad in (-1, 3):
        assert gate_route(logit_dtype=bad) == ERR_DTYPE, bad
    assert gate_route(scoring=2) == ERR_DTYPE
    assert gate_route(group_score=2) == ERR_DTYPE
    assert gate_route(scoring=2, k=0) == ERR_DTYPE
    for kw in (dict(T=-1), dict(k=0), dict(k=9), dict(E=65, k=65), dict(E=1025), dict(T=2 ** 26, k=2), dict(n_group=0),
               dict(n_group=3), dict(n_group=2, topk_group=3), dict(n_group=4, topk_group=1, k=3),
               dict(n_group=8, topk_group=2, group_score=1)):
        assert gate_route(chunk_tokens=0, **kw) == ERR_SHAPE, kw
    assert gate_route(k=0, chunk_tokens=-1) == ERR_SHAPE
    assert gate_route(chunk_tokens=-1) == ERR_SHAPE
    assert gate_route(T=MAX_CHUNKS + 1, chunk_tokens=1) == ERR_SHAPE
    assert gate_route(T=16 * MAX_CHUNKS + 1, chunk_tokens=16) == ERR_SHAPE
    assert gate_route(T=16 * MAX_CHUNKS + 1, chunk_tokens=0) == ERR_NULL        # the automatic chunk grows
    assert gate_route(T=0) == OK
    assert gate_route(T=0, ptrs=[FAKE] * 4 + [None] + [FAKE] * 4, ws=FAKE) == OK
    assert gate_route(T=0, chunk_tokens=-1) == ERR_SHAPE
    assert gate_route() == ERR_NULL
    need = workspace()
    for i in range(9):
        if i == 1:                                               # the bias is optional
            continue
        ptrs = [FAKE] * 9
        ptrs[i] = None
        assert gate_route(ptrs=ptrs, ws=FAKE, ws_bytes=need) == ERR_NULL, i
    assert gate_route(ptrs=[FAKE] * 9, ws=None, ws_bytes=need) == ERR_NULL
    for short in (0, need - 1):
        assert gate_route(ptrs=[FAKE] * 9, ws=FAKE, ws_bytes=short) == ERR_WORKSPACE, short
        assert gate_route(ptrs=[FAKE] * 9, ws=FAKE, ws_bytes=short, n_group=2, topk_group=1) == ERR_WORKSPACE, short


def test_workspace_query():
    assert workspace(64, 2, 8, 16) == (4 + 1) * 9 * 4
    assert workspace(65, 2, 8, 16) == (5 + 1) * 9 * 4
    # refused shapes and chunks
    for args in ((-1, 2, 8, 16), (4, -1, 8, 16), (4, 2, -1, 16), (4, 2, 1025, 16), (2 ** 26, 2, 8, 0), (64, 2, 8, -1),
                 (MAX_CHUNKS + 1, 2, 8, 1)):
        assert workspace(*args) == 0, args
    assert workspace(0, 2, 8, 0) > 0 and workspace(4, 0, 8, 0) > 0
    # monotone in T and in E, explicit and automatic chunk
    for ct in (0, 1, 16, 1000):
        for k in (1, 2, 8, 64):
            sizes = [workspace(T, k, 64, ct) for T in (0, 1, 15, 16, 17, 100, 1000, 4096, 8192)]
            assert sizes == sorted(sizes) and sizes[0] > 0, (ct, k, sizes)
            sizes = [workspace(4096, k, E, ct) for E in (0, 1, 8, 64, 256, 1024)]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (ct, k, sizes)
    # the automatic figure covers either entry's own chunk
    for T, k in ((4096, 2), (16384, 8), (100, 64), (5, 200)):
        for gated in (False, True):
            assert workspace(T, k, 64, 0) >= workspace(T, k, 64, auto_chunk(gated, T, k)), (T, k, gated)
    # the cap keeps the largest workspace in the tens of MB
    assert workspace(2 ** 27 - 1, 1, 1024, 0) <= (MAX_CHUNKS + 1) * 1025 * 4 < 40 * 2 ** 20


def test_route_form():
    for E, k in GATINGS:
        for gated in (True, False):
            forms = [dev.moe_route_form(T, k, E, gated=gated) for T in (0, 1, 2, 16, 17, 64, 100, 256, 1024, 4096, 16384, 10 ** 6)]
            assert forms[1] == "one" and forms[0] == "one", (E, k, gated)
            assert forms[-2] == "wide", (E, k, gated)
            assert forms == sorted(forms), ("monotone in T", E, k, gated, forms)        # "one" < "wide"
            assert dev.moe_route_form(16384, k, E, gated=gated, num_sms=256) == "wide"
    lib = _lib.get()
    assert lib.flute_moe_route_form(1, 4, 9, 8, 0) == ERR_SHAPE                 # k > E, gated
    assert lib.flute_moe_route_form(0, 4, 9, 8, 0) == 1                         # the ungated routing has no such limit
    assert lib.flute_moe_route_form(1, 4, 0, 8, 0) == ERR_SHAPE
    assert lib.flute_moe_route_form(0, -1, 2, 8, 0) == ERR_SHAPE
    assert lib.flute_moe_route_form(0, 4, 2, 1025, 0) == ERR_SHAPE
    assert lib.flute_moe_route_form(1, 2 ** 26, 2, 8, 0) == ERR_SHAPE
    with pytest.raises(RuntimeError):
        dev.moe_route_form(4, 9, 8)


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_signatures_and_validation():
    sig = inspect.signature(flute_amd.moe_route_wide).parameters
    assert list(sig) == ["topk_ids", "topk_weights", "num_experts", "chunk_tokens"] and sig["chunk_tokens"].default is None
    sig = inspect.signature(flute_amd.moe_gate_route_wide).parameters
    assert list(sig) == ["logits", "k", "num_experts", "scoring", "renormalize", "bias", "scale", "n_group", "topk_group",
                         "group_score", "chunk_tokens"]
    assert [sig[n].default for n in list(sig)[2:]] == [None, "softmax", False, None, 1.0, 1, 1, "max", None]
    sig = inspect.signature(dev.moe_route_form).parameters
    assert list(sig) == ["T", "k", "E", "gated", "num_sms"] and sig["gated"].default is True and sig["num_sms"].default == 0
    # the existing routing ops keep their lists
    assert list(inspect.signature(flute_amd.moe_route).parameters) == ["topk_ids", "topk_weights", "num_experts"]
    for fn in (FluteExperts.__init__, FluteExperts.from_linears):
        assert inspect.signature(fn).parameters["wide_routing"].default is False
    assert "wide_routing" not in inspect.signature(FluteSparseMoeBlock.__init__).parameters

    assert _validate_chunk_tokens(None, 100) == 0 and _validate_chunk_tokens(1, 100) == 1
    assert _validate_chunk_tokens(1, MAX_CHUNKS) == 1 and _validate_chunk_tokens(7, 0) == 7
    for exc, ct, T in ((ValueError, 0, 10), (ValueError, -1, 10), (ValueError, 1, MAX_CHUNKS + 1), (TypeError, 2.0, 10),
                       (TypeError, True, 10), (TypeError, "auto", 10)):
        with pytest.raises(exc):
            _validate_chunk_tokens(ct, T)
    ids, w = meta(5, 2, dtype=torch.int64), meta(5, 2)
    with pytest.raises(TypeError):
        flute_amd.moe_route_wide(meta(5, 2, dtype=torch.int16), w, 8)
    with pytest.raises(ValueError):
        flute_amd.moe_route_wide(ids, w, 8, chunk_tokens=0)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.moe_route_wide(ids, w, 8, chunk_tokens=2)
    with pytest.raises(ValueError):
        flute_amd.moe_gate_route_wide(meta(5, 8), 9)
    with pytest.raises(ValueError):
        flute_amd.moe_gate_route_wide(meta(5, 8), 2, chunk_tokens=-3)
    with pytest.raises(ValueError):
        flute_amd.moe_gate_route_wide(meta(5, 8), 2, n_group=3, topk_group=1)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.moe_gate_route_wide(meta(5, 8), 2)


def grouped(E, K, N, bits=4, g=64, tid=0):
    return GroupedFluteLinear(E, K, N, bits, g, tid, torch.device("cpu"), torch.float16)


def test_flute_experts_wide_routing_needs_native_routing():
    gate, up, down = grouped(2, 256, 512), grouped(2, 256, 512), grouped(2, 512, 256)
    assert FluteExperts(gate, up, down).wide_routing is False
    assert FluteExperts(gate, up, down, native_routing=True).wide_routing is False
    for wide in (True, "auto"):
        assert FluteExperts(gate, up, down, native_routing=True, wide_routing=wide).wide_routing == wide
        assert FluteExperts(gate, up, down, fused=True, native_routing=True, wide_routing=wide).wide_routing == wide
        with pytest.raises(ValueError, match="native_routing"):
            FluteExperts(gate, up, down, wide_routing=wide)
        with pytest.raises(ValueError, match="native_routing"):
            FluteExperts(gate, up, down, fused=True, wide_routing=wide)
    for bad in ("wide", 1, None, "Auto"):
        with pytest.raises(ValueError, match="wide_routing"):
            FluteExperts(gate, up, down, native_routing=True, wide_routing=bad)


def test_wave_ranges_tile_the_chunk():
    for lo, hi in ((0, 0), (0, 1), (5, 6), (0, 64), (3, 1027), (10, 10 + 16 * 64), (10, 11 + 16 * 64), (100, 2660)):
        spans = [wave_range(lo, hi, w) for w in range(16)]
        assert all((b - lo) % 64 == 0 and b <= e for b, e in spans)
        covered = [p for b, e in spans for p in range(b, e)]
        assert covered == list(range(lo, hi)), (lo, hi)


@pytest.mark.parametrize("T,k,E,chunk_tokens", ROUTE_WIDE_CASES)
def test_model_of_the_three_launches_is_the_contract(T, k, E, chunk_tokens):
    ct = auto_chunk(False, T, k) if chunk_tokens is None else chunk_tokens
    for seed in (1, 2):
        ids = draw_wide_ids(T, k, E, ct, 100 * seed + T + E).reshape(-1).tolist()
        if T * k > 40:
            assert any(not 0 <= v < E for v in ids)
        assert model_route_wide(ids, T, k, E, ct) == tuple(host_route(ids, k, E)), (T, k, E, ct)
    # the hostile routings of the GPU test, in the model first
    for ids in ([E - 1] * (T * k), [0] * (T * k), [-1] * (T * k)):
        assert model_route_wide(ids, T, k, E, ct) == tuple(host_route(ids, k, E)), (T, k, E, ct)
