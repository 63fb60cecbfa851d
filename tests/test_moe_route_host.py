"""flute_moe_route / flute_moe_combine, their Python wrappers and FluteExperts(native_routing=...) without a GPU: the
exports, every refusal of the C ABI in the documented order (returned before anything is enqueued, on null or host
pointers) and the wrappers' validation on meta and CPU tensors."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from flute_amd.integrations.moe import FluteExperts, GroupedFluteLinear
from flute_amd.ops import _validate_moe_combine, _validate_moe_route

OK, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
I32, I64 = 0, 1
F16, BF16, F32 = 0, 1, 2


def route(id_dtype=I32, weight_dtype=F16, T=4, k=2, E=8, ptrs=(None,) * 7):
    """ptrs: ids, weights, offsets, perm, rows, row_weight, pos"""
    return _lib.get().flute_moe_route(id_dtype, weight_dtype, T, k, E, *ptrs, None)


def combine(dtype=F16, T=4, k=2, E=8, N=64, ptrs=(None,) * 4):
    """ptrs: Y, pos, offsets, out"""
    return _lib.get().flute_moe_combine(dtype, T, k, E, N, *ptrs, None)


def test_symbols_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_moe_route", "flute_moe_combine"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert "#define FLUTE_MOE_ROUTE_MAX_EXPERTS 1024" in text
    assert flute_amd.moe_route is flute_amd.ops.moe_route
    assert flute_amd.moe_combine is flute_amd.ops.moe_combine


def test_route_refusals_in_order():
    for bad in (-1, 2, 3):
        assert route(id_dtype=bad) == ERR_DTYPE, bad
    for bad in (-1, 3):
        assert route(weight_dtype=bad) == ERR_DTYPE, bad
    for good in (F16, BF16, F32):
        assert route(weight_dtype=good) == ERR_NULL, good
    assert route(id_dtype=I64) == ERR_NULL
    # the order: dtype before shape, shape before "nothing to do" and the nulls
    assert route(id_dtype=2, T=-1) == ERR_DTYPE
    assert route(weight_dtype=3, E=2000) == ERR_DTYPE
    assert route(T=-1) == ERR_SHAPE
    assert route(k=-1) == ERR_SHAPE
    assert route(E=-1) == ERR_SHAPE
    assert route(E=1025) == ERR_SHAPE
    assert route(E=1024) == ERR_NULL
    assert route(T=0, E=1025) == ERR_SHAPE
    assert route(T=2 ** 26, k=2) == ERR_SHAPE                    # T k = 2^27
    assert route(T=2 ** 30, k=8) == ERR_SHAPE                    # T k overflows an int
    assert route(T=2 ** 31 - 1, k=2 ** 31 - 1) == ERR_SHAPE
    assert route(T=2 ** 27 - 1, k=1) == ERR_NULL
    assert route(T=2 ** 27 - 1, k=1, ptrs=[FAKE] * 2 + [None] + [FAKE] * 4) == ERR_NULL


def test_route_nothing_to_do_and_nulls():
    assert route(T=0) == OK                                      # no pair, no offsets to write: no launch
    assert route(k=0) == OK
    assert route(T=0, k=0, E=0) == OK
    assert route(T=0, ptrs=[FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE]) == OK
    assert route() == ERR_NULL
    for i in range(7):
        ptrs = [FAKE] * 7
        ptrs[i] = None
        if i == 1:                                               # weights are optional: that is a valid call, not made here
            continue
        assert route(ptrs=ptrs) == ERR_NULL, i
    # without weights row_weight is not looked at; the other nulls are still refused
    for i in (0, 2, 3, 4, 6):
        ptrs = [FAKE, None, FAKE, FAKE, FAKE, None, FAKE]
        ptrs[i] = None
        assert route(ptrs=ptrs) == ERR_NULL, i


def test_combine_refusals_in_order():
    for bad in (-1, 2, 3):
        assert combine(dtype=bad) == ERR_DTYPE, bad
    assert combine(dtype=2, N=63) == ERR_DTYPE                   # the order
    assert combine(T=-1) == ERR_SHAPE
    assert combine(k=-1) == ERR_SHAPE
    assert combine(E=-1) == ERR_SHAPE
    assert combine(N=-8) == ERR_SHAPE
    for n in (1, 4, 12, 63, 1028):
        assert combine(N=n) == ERR_SHAPE, n
    assert combine(T=0, N=12) == ERR_SHAPE                       # ... before "nothing to do"
    assert combine(T=2 ** 30, k=2) == ERR_SHAPE                  # T k overflows an int
    assert combine(T=2 ** 30, k=1, N=2048) == ERR_SHAPE          # tokens x column chunks does not fit the grid
    assert combine(T=2 ** 30, k=1, N=1024) == ERR_NULL
    assert combine(E=5000) == ERR_NULL                           # the cap on E is moe_route's; only offsets[E] is read here


def test_combine_nothing_to_do_and_nulls():
    assert combine(T=0) == OK
    assert combine(N=0) == OK
    assert combine(T=0, ptrs=[FAKE] * 4) == OK
    assert combine() == ERR_NULL
    for i in range(4):
        ptrs = [FAKE] * 4
        ptrs[i] = None
        assert combine(ptrs=ptrs) == ERR_NULL, i
    # k == 0 is a launch that writes zeros: Y and pos are not needed, offsets and out are
    assert combine(k=0) == ERR_NULL
    assert combine(k=0, ptrs=[None, None, FAKE, None]) == ERR_NULL
    assert combine(k=0, ptrs=[None, None, None, FAKE]) == ERR_NULL


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_validate_moe_route():
    ids, w = meta(5, 2, dtype=torch.int64), meta(5, 2)
    _validate_moe_route(ids, w, 8)
    _validate_moe_route(ids.int(), w.float(), 8)
    _validate_moe_route(ids, w.bfloat16(), 1024)
    _validate_moe_route(ids, None, 0)
    V, T = ValueError, TypeError
    bad = [(V, meta(10, dtype=torch.int64), None, 8), (V, meta(5, 2, 1, dtype=torch.int64), None, 8),
           (T, meta(5, 2, dtype=torch.int16), w, 8), (T, meta(5, 2), w, 8), (T, ids, w.double(), 8),
           (T, ids, meta(5, 2, dtype=torch.int32), 8), (V, ids, meta(5, 3), 8), (V, ids, meta(10), 8),
           (V, ids, w, -1), (V, ids, w, 1025), (V, meta(2 ** 26, 2, dtype=torch.int32), None, 8)]
    for exc, i, ww, E in bad:
        with pytest.raises(exc):
            _validate_moe_route(i, ww, E)
    # the public function validates before any device call, then refuses tensors that are not on a GPU
    with pytest.raises(T):
        flute_amd.moe_route(meta(5, 2, dtype=torch.int16), w, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.moe_route(ids, w, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.moe_route(torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 2), 8)


def test_validate_moe_combine():
    y, pos, off = meta(10, 64), meta(5, 2, dtype=torch.int32), meta(9, dtype=torch.int32)
    _validate_moe_combine(y, pos, off)
    _validate_moe_combine(y.bfloat16(), pos, off)
    V, T = ValueError, TypeError
    bad = [(V, meta(10, 64, 1), pos, off), (V, y, meta(10, dtype=torch.int32), off), (V, y, pos, meta(9, 1, dtype=torch.int32)),
           (T, y.float(), pos, off), (T, y, pos.long(), off), (T, y, pos, off.long()),
           (V, meta(9, 64), pos, off), (V, meta(10, 60), pos, off), (V, y, pos, meta(0, dtype=torch.int32))]
    for exc, yy, pp, oo in bad:
        with pytest.raises(exc):
            _validate_moe_combine(yy, pp, oo)
    with pytest.raises(T):
        flute_amd.moe_combine(y, pos.long(), off)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.moe_combine(y, pos, off)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.moe_combine(torch.zeros(10, 64, dtype=torch.float16), torch.zeros(5, 2, dtype=torch.int32),
                              torch.zeros(9, dtype=torch.int32))


def grouped(E, K, N, bits=4, g=64, tid=0):
    return GroupedFluteLinear(E, K, N, bits, g, tid, torch.device("cpu"), torch.float16)


def test_flute_experts_native_routing_is_off_by_default():
    gate, up, down = grouped(2, 256, 512), grouped(2, 256, 512), grouped(2, 512, 256)
    assert FluteExperts(gate, up, down).native_routing is False
    assert FluteExperts(gate, up, down, fused=True).native_routing is False
    assert FluteExperts(gate, up, down, native_routing=False).native_routing is False
    both = FluteExperts(gate, up, down, fused=True, native_routing=True)
    assert both.native_routing is True and both.fused is True
    only = FluteExperts(gate, up, down, native_routing=True)
    assert only.native_routing is True and only.fused is False


def test_from_linears_takes_native_routing():
    import inspect
    sig = inspect.signature(FluteExperts.from_linears)
    assert sig.parameters["native_routing"].default is False
    assert inspect.signature(FluteExperts.__init__).parameters["native_routing"].default is False
