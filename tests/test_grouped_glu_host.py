"""flute_qgemm_grouped_glu / flute_qgemm_grouped_weighted, their Python wrappers and FluteExperts(fused=...) without a
GPU: the exports, every refusal of the C ABI (returned before anything is enqueued, on null or host pointers) and the
wrappers' validation on meta tensors."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from flute_amd.integrations.moe import FluteExperts, GroupedFluteLinear
from flute_amd.ops import _validate_grouped_glu, _validate_grouped_weighted
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind


def glu(dtype=0, bits=4, g=64, E=4, R=8, Tsrc=8, F=1024, K=512, P=None, tid=0, ptrs=(None,) * 10, num_sms=256):
    """ptrs: Xsrc, rows, offsets, Qgate, Sgate, QM2gate, Qup, Sup, QM2up, H"""
    P = bits * F // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_glu(dtype, bits, g, E, R, Tsrc, F, K, P, tid, *ptrs, num_sms, None)


def weighted(dtype=0, bits=4, g=64, E=4, T=8, N=1024, K=512, P=None, tid=0, ptrs=(None,) * 7, num_sms=256):
    """ptrs: X, offsets, Q, S, QM2, row_weight, Y"""
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_weighted(dtype, bits, g, E, T, N, K, P, tid, *ptrs, num_sms, None)


def test_symbols_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_glu", "flute_qgemm_grouped_weighted"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert "silu32(g) = g / (1 + exp(-g))" in text and "eps_s = 2^-21" in text
    assert flute_amd.qgemm_grouped_glu is flute_amd.ops.qgemm_grouped_glu
    assert flute_amd.qgemm_grouped_weighted is flute_amd.ops.qgemm_grouped_weighted


@pytest.mark.parametrize("call", [glu, weighted])
def test_layer_refusals_with_null_pointers(call):
    assert call(dtype=2) == ERR_DTYPE
    assert call(bits=5) == ERR_NUM_BITS
    assert call(bits=1) == ERR_NUM_BITS
    for g in (0, 16, 48, 512):
        assert call(g=g) == ERR_GROUP_SIZE, g
    assert call(tid=10 ** 6) == ERR_TEMPLATE_ID
    width = "F" if call is glu else "N"
    assert call(bits=3, tid=first_template(3, 64), **{width: 512}) == ERR_TEMPLATE_ID      # 3 bits: TileP 32 only
    assert call(dtype=2, bits=5) == ERR_DTYPE                                        # the order: dtype first
    assert call(bits=5, g=48, K=480, E=-1) == ERR_NUM_BITS


@pytest.mark.parametrize("call", [glu, weighted])
def test_shape_refusals_with_null_pointers(call):
    width = "F" if call is glu else "N"
    rows = "R" if call is glu else "T"
    assert call(**{width: 1000}) == ERR_SHAPE
    assert call(tid=first_template(4, 32), **{width: 64}) == ERR_SHAPE
    assert call(tid=first_template(4, 64), **{width: 128}) == ERR_SHAPE      # TileP 64: the column block is 256
    assert call(bits=3, tid=first_template(3, 32), **{width: 256}) == ERR_SHAPE
    assert call(K=480) == ERR_SHAPE              # K % 64
    assert call(K=384, g=256) == ERR_SHAPE       # K % g
    assert call(K=0) == ERR_SHAPE
    assert call(P=255) == ERR_SHAPE
    assert call(E=-1) == ERR_SHAPE
    assert call(**{rows: -1}) == ERR_SHAPE


def test_glu_source_rows_refusals():
    assert glu(Tsrc=-1) == ERR_SHAPE
    assert glu(R=8, Tsrc=9) == ERR_SHAPE                                   # no index: Xsrc has exactly R rows
    assert glu(R=8, Tsrc=7) == ERR_SHAPE
    with_rows = [None, FAKE] + [None] * 8
    assert glu(R=8, Tsrc=0, ptrs=with_rows) == ERR_SHAPE                   # an index into no rows
    assert glu(R=8, Tsrc=3, ptrs=with_rows) == ERR_NULL                    # any Tsrc >= 1 is a shape; the nulls come next
    assert glu(R=0, Tsrc=0, ptrs=with_rows) == OK
    assert glu(R=0, Tsrc=5) == ERR_SHAPE                                   # ... refused before "nothing to do"


def test_nothing_to_do_is_ok_and_nulls_are_refused():
    assert glu(R=0, Tsrc=0) == OK                  # no launch: the null pointers are never looked at
    assert glu(E=0) == OK
    assert weighted(T=0) == OK
    assert weighted(E=0) == OK
    assert glu() == ERR_NULL
    assert weighted() == ERR_NULL
    for i in range(10):
        ptrs = [FAKE] * 10
        ptrs[i] = None
        if i == 1:                                 # rows is optional: null with every other pointer set is a valid call
            continue                               # (Tsrc == R) that would launch on these host pointers - not made here
        assert glu(ptrs=ptrs) == ERR_NULL, i
        ptrs[1] = None
        assert glu(ptrs=ptrs) == ERR_NULL, i       # ... and without the index
    for i in range(7):
        ptrs = [FAKE] * 7
        ptrs[i] = None
        assert weighted(ptrs=ptrs) == ERR_NULL, i


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def stack(E=4, K=512, N=1024, bits=4, g=64, dtype=torch.float16):
    return (meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g, dtype=dtype),
            meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))


def test_validate_grouped_glu():
    x, off = meta(8, 512), meta(5, dtype=torch.int32)
    gate, up = stack(), stack()
    rows = meta(20, dtype=torch.int32)
    _validate_grouped_glu(x, off, *gate, *up, 4, 64, None)
    _validate_grouped_glu(x, off, *gate, *up, 4, 64, rows)
    V, T = ValueError, TypeError
    bad = [
        (V, stack(N=2048), None),                              # the stacks differ: F
        (V, stack(E=3), None),                                 # E
        (V, stack(K=1024), None),                              # K
        (V, stack(g=128), None),                               # group count
        (V, stack(bits=2), None),                              # the packed rows of another bit width
        (T, stack(dtype=torch.bfloat16), None),                # dtype of the scales
        (T, (up[0].to(torch.int32), up[1], up[2]), None),
        (T, (up[0], up[1], up[2].half()), None),
        (T, up, rows.long()),                                  # rows: int32 only
        (T, up, rows.float()),
        (V, up, rows[:, None]),                                # rows: one axis
    ]
    for exc, u, r in bad:
        with pytest.raises(exc):
            _validate_grouped_glu(x, off, *gate, *u, 4, 64, r)
        if r is None:                                          # the same mismatch with the stacks swapped
            with pytest.raises(exc):
                _validate_grouped_glu(x, off, *u, *gate, 4, 64, r)
    with pytest.raises(T):
        _validate_grouped_glu(x, off.long(), *gate, *up, 4, 64, None)
    with pytest.raises(V):
        _validate_grouped_glu(x, off, *gate, *up, 5, 64, None)
    # the public function validates before any device call, then refuses tensors that are not on a GPU
    with pytest.raises(T):
        flute_amd.qgemm_grouped_glu(x, off, *gate, *up, 4, 64, 0, rows=rows.long())
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.qgemm_grouped_glu(x, off, *gate, *up, 4, 64, 0, rows=rows)


def test_validate_grouped_weighted():
    x, off = meta(8, 512), meta(5, dtype=torch.int32)
    w = stack()
    rw = meta(8, dtype=torch.float32)
    _validate_grouped_weighted(x, off, *w, rw, 4, 64)
    V, T = ValueError, TypeError
    for exc, r in ((T, rw.half()), (T, rw.double()), (T, meta(8, dtype=torch.int32)), (V, meta(7, dtype=torch.float32)),
                   (V, meta(8, 1, dtype=torch.float32))):
        with pytest.raises(exc):
            _validate_grouped_weighted(x, off, *w, r, 4, 64)
    with pytest.raises(V):
        _validate_grouped_weighted(x, off, *stack(K=1024), rw, 4, 64)
    with pytest.raises(T):
        flute_amd.qgemm_grouped_weighted(x, off, *w, rw.half(), 4, 64, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.qgemm_grouped_weighted(x, off, *w, rw, 4, 64, 0)


def grouped(E, K, N, bits=4, g=64, tid=0):
    return GroupedFluteLinear(E, K, N, bits, g, tid, torch.device("cpu"), torch.float16)


def test_flute_experts_fused_is_off_by_default():
    gate, up, down = grouped(2, 256, 512), grouped(2, 256, 512), grouped(2, 512, 256)
    assert FluteExperts(gate, up, down).fused is False
    assert FluteExperts(gate, up, down, fused=False).fused is False
    assert FluteExperts(gate, up, down, fused=True).fused is True
    with pytest.raises(ValueError):
        FluteExperts(gate, grouped(2, 256, 512, g=128), down, fused=True)      # one launch: one group size for gate and up
    FluteExperts(gate, grouped(2, 256, 512, g=128), down)                      # the unfused forward takes it, as before
