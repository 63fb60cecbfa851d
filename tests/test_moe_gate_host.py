"""flute_moe_gate / flute_moe_gate_route, their Python wrappers, FluteExperts.forward_logits and FluteSparseMoeBlock without
a GPU: the exports, every refusal of the C ABI in the documented order (returned before anything is enqueued, on null or
host pointers), the wrappers' validation on meta and CPU tensors, and the fp64 reference (tests/moe_gate_ref.py) on a
hand-worked example."""
import inspect
import math
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from flute_amd.integrations.moe import FluteExperts, FluteSparseMoeBlock, GroupedFluteLinear
from flute_amd.ops import _validate_moe_gate
from tests import moe_gate_ref as R

OK, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
F16, BF16, F32 = 0, 1, 2
SOFTMAX, SIGMOID = 0, 1


def gate(dtype=F16, T=4, E=8, k=2, scoring=SOFTMAX, renorm=0, scale=1.0, ptrs=(None,) * 4):
    """ptrs: logits, bias, ids, weights"""
    return _lib.get().flute_moe_gate(dtype, T, E, k, scoring, renorm, scale, *ptrs, None)


def gate_route(dtype=F16, T=4, E=8, k=2, scoring=SOFTMAX, renorm=0, scale=1.0, ptrs=(None,) * 9):
    """ptrs: logits, bias, ids, weights, offsets, perm, rows, row_weight, pos"""
    return _lib.get().flute_moe_gate_route(dtype, T, E, k, scoring, renorm, scale, *ptrs, None)


BOTH = [(gate, 4), (gate_route, 9)]


def test_symbols_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_moe_gate", "flute_moe_gate_route"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert "FLUTE_GATE_SOFTMAX = 0" in text and "FLUTE_GATE_SIGMOID = 1" in text
    assert "#define FLUTE_MOE_GATE_MAX_TOPK 64" in text
    assert "n_group" in text and "topk_group" in text            # group-limited selection is named as out of scope
    assert flute_amd.moe_gate is flute_amd.ops.moe_gate
    assert flute_amd.moe_gate_route is flute_amd.ops.moe_gate_route


@pytest.mark.parametrize("fn,n", BOTH)
def test_refusals_in_order(fn, n):
    every = [FAKE] * n
    for bad in (-1, 3, 4):
        assert fn(dtype=bad, ptrs=every) == ERR_DTYPE, bad
    for bad in (-1, 2):
        assert fn(scoring=bad, ptrs=every) == ERR_DTYPE, bad
    for good in (F16, BF16, F32):
        for scoring in (SOFTMAX, SIGMOID):
            assert fn(dtype=good, scoring=scoring) == ERR_NULL, (good, scoring)
    # dtype and scoring before shape
    assert fn(dtype=3, k=0) == ERR_DTYPE
    assert fn(scoring=2, E=1025) == ERR_DTYPE
    assert fn(dtype=3, scoring=2, T=-1) == ERR_DTYPE
    # shape, with every pointer given: nothing may be enqueued on them
    assert fn(k=0, ptrs=every) == ERR_SHAPE
    assert fn(k=-1, ptrs=every) == ERR_SHAPE
    assert fn(E=8, k=9, ptrs=every) == ERR_SHAPE                  # k > E
    assert fn(E=0, k=1, ptrs=every) == ERR_SHAPE
    assert fn(E=128, k=65, ptrs=every) == ERR_SHAPE               # k > 64
    assert fn(E=1025, ptrs=every) == ERR_SHAPE
    assert fn(T=-1, ptrs=every) == ERR_SHAPE
    assert fn(T=2 ** 26, k=2, ptrs=every) == ERR_SHAPE            # T k = 2^27
    assert fn(T=2 ** 30, k=8, E=64, ptrs=every) == ERR_SHAPE      # T k overflows an int
    # ... before "nothing to do"
    assert fn(T=0, k=0, ptrs=every) == ERR_SHAPE
    assert fn(T=0, E=1025, ptrs=every) == ERR_SHAPE
    assert fn(T=0, E=8, k=9) == ERR_SHAPE
    # the limits themselves pass the shape check
    assert fn(E=128, k=64) == ERR_NULL
    assert fn(E=1024, k=1) == ERR_NULL
    assert fn(E=1, k=1) == ERR_NULL
    assert fn(T=2 ** 27 - 1, k=1) == ERR_NULL
    assert fn(T=2 ** 26 - 1, k=2) == ERR_NULL


def test_gate_nothing_to_do_and_nulls():
    assert gate(T=0) == OK
    assert gate(T=0, ptrs=[FAKE] * 4) == OK
    assert gate() == ERR_NULL
    for i in (0, 2, 3):
        ptrs = [FAKE] * 4
        ptrs[i] = None
        assert gate(ptrs=ptrs) == ERR_NULL, i
        ptrs[1] = None                                           # the bias is optional; the other nulls are still refused
        assert gate(ptrs=ptrs) == ERR_NULL, i


def test_gate_route_nothing_to_do_and_nulls():
    assert gate_route(T=0) == OK                                 # no token, no offsets to write: no launch
    assert gate_route(T=0, ptrs=[FAKE] * 4 + [None] + [FAKE] * 4) == OK
    assert gate_route() == ERR_NULL
    for i in (0, 2, 3, 4, 5, 6, 7, 8):
        ptrs = [FAKE] * 9
        ptrs[i] = None
        assert gate_route(ptrs=ptrs) == ERR_NULL, i
        ptrs[1] = None
        assert gate_route(ptrs=ptrs) == ERR_NULL, i


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_validate_moe_gate():
    x, b = meta(5, 8), meta(8, dtype=torch.float32)
    _validate_moe_gate(x, 2, "softmax", None)
    _validate_moe_gate(x.bfloat16(), 8, "sigmoid", b)
    _validate_moe_gate(x.float(), 1, "softmax", b, 8)
    _validate_moe_gate(meta(3, 1024), 64, "softmax", None, 1024)
    V, T = ValueError, TypeError
    bad = [(V, meta(40), 2, "softmax", None, None), (V, meta(5, 8, 1), 2, "softmax", None, None),
           (T, x.double(), 2, "softmax", None, None), (T, meta(5, 8, dtype=torch.int32), 2, "softmax", None, None),
           (V, x, 2, "tanh", None, None), (V, x, 2, 0, None, None),
           (V, x, 2, "softmax", None, 9), (T, x, 2, "softmax", meta(8), None), (V, x, 2, "softmax", meta(9, dtype=torch.float32), None),
           (V, x, 2, "softmax", meta(1, 8, dtype=torch.float32), None),
           (V, x, 0, "softmax", None, None), (V, x, 9, "softmax", None, None), (V, meta(5, 128), 65, "softmax", None, None),
           (V, meta(5, 1025), 2, "softmax", None, None), (V, meta(2 ** 26, 8), 2, "softmax", None, None)]
    for exc, xx, k, scoring, bias, E in bad:
        with pytest.raises(exc):
            _validate_moe_gate(xx, k, scoring, bias, E)
    # the public functions validate before any device call, then refuse tensors that are not on a GPU
    for fn in (flute_amd.moe_gate, flute_amd.moe_gate_route):
        with pytest.raises(T):
            fn(x.double(), 2)
        with pytest.raises(V):
            fn(x, 9)
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x, 2)
        with pytest.raises(RuntimeError, match="GPU"):
            fn(torch.zeros(5, 8), 2, bias=torch.zeros(8))
    with pytest.raises(V):
        flute_amd.moe_gate_route(x, 2, 7)
    assert list(inspect.signature(flute_amd.moe_gate).parameters) == ["logits", "k", "scoring", "renormalize", "bias", "scale"]
    assert list(inspect.signature(flute_amd.moe_gate_route).parameters) == \
        ["logits", "k", "num_experts", "scoring", "renormalize", "bias", "scale"]
    sig = inspect.signature(flute_amd.moe_gate).parameters
    assert (sig["scoring"].default, sig["renormalize"].default, sig["bias"].default, sig["scale"].default) == \
        ("softmax", False, None, 1.0)


def test_reference_on_a_hand_worked_row():
    """logits ln 1, ln 2, ln 4, ln 2: the softmax is 1/9, 2/9, 4/9, 2/9, and experts 1 and 3 tie."""
    x = torch.tensor([[0.0, math.log(2.0), math.log(4.0), math.log(2.0)]], dtype=torch.float64)
    close = lambda got, want: torch.allclose(got, torch.tensor([want], dtype=torch.float64), rtol=1e-14, atol=0)
    ids, w = R.gate(x, 2)
    assert ids.tolist() == [[2, 1]] and close(w, [4 / 9, 2 / 9])                    # the tie goes to the lower index
    ids, w = R.gate(x, 3)
    assert ids.tolist() == [[2, 1, 3]] and close(w, [4 / 9, 2 / 9, 2 / 9])
    ids, w = R.gate(x, 2, renormalize=True, scale=3.0)
    assert ids.tolist() == [[2, 1]] and close(w, [2.0, 1.0])
    ids, w = R.gate(x, 4)
    assert ids.tolist() == [[2, 1, 3, 0]] and abs(float(w.sum()) - 1) < 1e-15
    # the bias moves the choice and never enters a weight
    bias = torch.tensor([0.5, 0.0, 0.0, 0.0])
    ids, w = R.gate(x, 2, bias=bias)
    assert ids.tolist() == [[0, 2]] and close(w, [1 / 9, 4 / 9])
    ids, w = R.gate(x, 2, bias=bias, renormalize=True)
    assert ids.tolist() == [[0, 2]] and close(w, [1 / 5, 4 / 5])
    # sigmoid of 0, ln 3, -ln 3, ln 3: 1/2, 3/4, 1/4, 3/4
    y = torch.tensor([[0.0, math.log(3.0), -math.log(3.0), math.log(3.0)]], dtype=torch.float64)
    ids, w = R.gate(y, 3, scoring="sigmoid")
    assert ids.tolist() == [[1, 3, 0]] and close(w, [0.75, 0.75, 0.5])
    ids, w = R.gate(y, 2, scoring="sigmoid", renormalize=True, scale=2.5)
    assert ids.tolist() == [[1, 3]] and close(w, [1.25, 1.25])
    # a NaN key ranks as -infinity: behind every number, in index order among its like
    z = torch.tensor([[float("nan"), -5.0, float("-inf"), float("nan")]], dtype=torch.float64)
    assert R.gate(z, 4)[0].tolist() == [[1, 0, 2, 3]]
    # all equal: 0 .. k - 1; -0 equals +0
    assert R.gate(torch.zeros(2, 6), 4)[0].tolist() == [[0, 1, 2, 3]] * 2
    assert R.gate(torch.tensor([[0.0, -0.0, 0.0]]), 2)[0].tolist() == [[0, 1]]
    assert R.separated(R.keys(x, "softmax"), 1).tolist() == [True]
    assert R.separated(R.keys(x, "softmax"), 2).tolist() == [False]


def grouped(E, K, N, bits=4, g=64, tid=0):
    return GroupedFluteLinear(E, K, N, bits, g, tid, torch.device("cpu"), torch.float16)


def test_forward_logits_and_block_signatures():
    sig = inspect.signature(FluteExperts.forward_logits).parameters
    assert list(sig) == ["self", "hidden", "router_logits", "top_k", "scoring", "renormalize", "bias", "scale"]
    assert (sig["scoring"].default, sig["renormalize"].default, sig["bias"].default, sig["scale"].default) == \
        ("softmax", False, None, 1.0)
    experts = FluteExperts(grouped(4, 256, 512), grouped(4, 256, 512), grouped(4, 512, 256), fused=True, native_routing=True)
    with pytest.raises(ValueError):
        experts.forward_logits(torch.zeros(3, 256), torch.zeros(3, 5), 2)
    router = torch.zeros(4, 256, dtype=torch.float16)
    block = FluteSparseMoeBlock(router, experts, 2, renormalize=True)
    assert block.top_k == 2 and block.scoring == "softmax" and block.renormalize is True and block.scale == 1.0
    assert block.bias is None and block.experts is experts and "router_weight" in dict(block.named_buffers())
    biased = FluteSparseMoeBlock(router, experts, 4, scoring="sigmoid", bias=torch.zeros(4), scale=2.5)
    assert "bias" in dict(biased.named_buffers()) and biased.scale == 2.5
    for bad in (dict(router_weight=torch.zeros(5, 256), top_k=2), dict(router_weight=torch.zeros(4, 128), top_k=2),
                dict(router_weight=router, top_k=0), dict(router_weight=router, top_k=5),
                dict(router_weight=router, top_k=2, scoring="tanh"),
                dict(router_weight=router, top_k=2, bias=torch.zeros(5)),
                dict(router_weight=router, top_k=2, bias=torch.zeros(4, dtype=torch.float16))):
        with pytest.raises(ValueError):
            FluteSparseMoeBlock(experts=experts, **bad)
    assert "n_group" in FluteSparseMoeBlock.__doc__ and "dense torch op" in FluteSparseMoeBlock.__doc__
