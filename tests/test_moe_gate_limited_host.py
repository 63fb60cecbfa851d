"""flute_moe_gate_limited / flute_moe_gate_route_limited, their Python wrappers, FluteExperts.forward_logits_limited and the
group arguments of FluteSparseMoeBlock without a GPU: the exports, every refusal of the C ABI in the documented order
(returned before anything is enqueued, on null or host pointers), the wrappers' validation on meta and CPU tensors, and the
fp64 reference (tests/moe_gate_limited_ref.py) on a hand-worked row."""
import inspect
import math
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from flute_amd.integrations.moe import FluteExperts, FluteSparseMoeBlock, GroupedFluteLinear
from flute_amd.ops import _validate_moe_gate_limited
from tests import moe_gate_limited_ref as L
from tests import moe_gate_ref as R

OK, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
F16, BF16, F32 = 0, 1, 2
SOFTMAX, SIGMOID = 0, 1
GMAX, TOP2SUM = 0, 1


def gate(dtype=F16, T=4, E=8, k=2, n_group=4, topk_group=2, group_score=GMAX, scoring=SOFTMAX, renorm=0, scale=1.0,
         ptrs=(None,) * 4):
    """ptrs: logits, bias, ids, weights"""
    return _lib.get().flute_moe_gate_limited(dtype, T, E, k, n_group, topk_group, group_score, scoring, renorm, scale, *ptrs,
                                             None)


def gate_route(dtype=F16, T=4, E=8, k=2, n_group=4, topk_group=2, group_score=GMAX, scoring=SOFTMAX, renorm=0, scale=1.0,
               ptrs=(None,) * 9):
    """ptrs: logits, bias, ids, weights, offsets, perm, rows, row_weight, pos"""
    return _lib.get().flute_moe_gate_route_limited(dtype, T, E, k, n_group, topk_group, group_score, scoring, renorm, scale,
                                                   *ptrs, None)


BOTH = [(gate, 4), (gate_route, 9)]


def test_symbols_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_moe_gate_limited", "flute_moe_gate_route_limited"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert "FLUTE_GATE_GROUP_MAX = 0" in text and "FLUTE_GATE_GROUP_TOP2SUM = 1" in text
    assert "#define FLUTE_MOE_GATE_MAX_GROUPS 64" in text
    assert "n_group, topk_group) is out of scope" not in text
    assert flute_amd.moe_gate_limited is flute_amd.ops.moe_gate_limited
    assert flute_amd.moe_gate_route_limited is flute_amd.ops.moe_gate_route_limited
    assert flute_amd.ops.MOE_GATE_MAX_GROUPS == 64


@pytest.mark.parametrize("fn,n", BOTH)
def test_refusals_in_order(fn, n):
    every = [FAKE] * n
    # 1. dtype: logit_dtype, then scoring, then group_score - each before every shape
    for bad in (-1, 3, 4):
        assert fn(dtype=bad, ptrs=every) == ERR_DTYPE, bad
    for bad in (-1, 2):
        assert fn(scoring=bad, ptrs=every) == ERR_DTYPE, bad
        assert fn(group_score=bad, ptrs=every) == ERR_DTYPE, bad
    assert fn(dtype=3, k=0) == ERR_DTYPE
    assert fn(scoring=2, E=1025) == ERR_DTYPE
    assert fn(group_score=2, n_group=0) == ERR_DTYPE
    assert fn(group_score=2, k=0, T=-1, n_group=65, topk_group=0) == ERR_DTYPE
    for good in (F16, BF16, F32):
        for scoring in (SOFTMAX, SIGMOID):
            for group_score in (GMAX, TOP2SUM):
                assert fn(dtype=good, scoring=scoring, group_score=group_score) == ERR_NULL, (good, scoring, group_score)
    # 2.1 flute_moe_gate's shape conditions, with every pointer given: nothing may be enqueued on them
    assert fn(k=0, ptrs=every) == ERR_SHAPE
    assert fn(k=-1, ptrs=every) == ERR_SHAPE
    assert fn(E=8, k=9, n_group=1, topk_group=1, ptrs=every) == ERR_SHAPE            # k > E
    assert fn(E=0, k=1, ptrs=every) == ERR_SHAPE
    assert fn(E=128, k=65, n_group=1, topk_group=1, ptrs=every) == ERR_SHAPE         # k > 64
    assert fn(E=1028, ptrs=every) == ERR_SHAPE                                       # E > 1024, a multiple of n_group
    assert fn(T=-1, ptrs=every) == ERR_SHAPE
    assert fn(T=2 ** 26, k=2, ptrs=every) == ERR_SHAPE                               # T k = 2^27
    assert fn(T=2 ** 30, k=8, E=64, ptrs=every) == ERR_SHAPE                         # T k overflows an int
    # 2.2 .. 2.6 the groups
    assert fn(n_group=0, ptrs=every) == ERR_SHAPE
    assert fn(n_group=-4, ptrs=every) == ERR_SHAPE
    assert fn(E=130, n_group=65, topk_group=2, ptrs=every) == ERR_SHAPE              # n_group > 64, though it divides E
    assert fn(E=8, n_group=3, ptrs=every) == ERR_SHAPE                               # E % n_group
    assert fn(E=60, n_group=8, ptrs=every) == ERR_SHAPE
    assert fn(topk_group=0, ptrs=every) == ERR_SHAPE
    assert fn(topk_group=-1, ptrs=every) == ERR_SHAPE
    assert fn(n_group=4, topk_group=5, ptrs=every) == ERR_SHAPE                      # topk_group > n_group
    assert fn(E=8, k=3, n_group=4, topk_group=1, ptrs=every) == ERR_SHAPE            # k > topk_group gs = 2
    assert fn(E=8, k=5, n_group=4, topk_group=2, ptrs=every) == ERR_SHAPE            # k > 4
    assert fn(E=8, k=1, n_group=8, topk_group=3, group_score=TOP2SUM, ptrs=every) == ERR_SHAPE       # top2sum with gs = 1
    assert fn(E=1, k=1, n_group=1, topk_group=1, group_score=TOP2SUM, ptrs=every) == ERR_SHAPE
    # ... all before "nothing to do"
    assert fn(T=0, k=0, ptrs=every) == ERR_SHAPE
    assert fn(T=0, n_group=65, E=130, ptrs=every) == ERR_SHAPE
    assert fn(T=0, E=8, n_group=3) == ERR_SHAPE
    assert fn(T=0, topk_group=5) == ERR_SHAPE
    assert fn(T=0, E=8, k=3, n_group=4, topk_group=1) == ERR_SHAPE
    assert fn(T=0, E=8, k=1, n_group=8, topk_group=3, group_score=TOP2SUM) == ERR_SHAPE
    # the limits themselves pass the shape check
    assert fn(E=8, k=4, n_group=4, topk_group=2) == ERR_NULL                          # k = topk_group gs
    assert fn(E=1024, k=64, n_group=64, topk_group=4, group_score=TOP2SUM) == ERR_NULL
    assert fn(E=64, k=1, n_group=64, topk_group=1) == ERR_NULL                        # gs = 1 with max
    assert fn(E=4, k=2, n_group=2, topk_group=1, group_score=TOP2SUM) == ERR_NULL     # gs = 2 with top2sum
    assert fn(E=1, k=1, n_group=1, topk_group=1) == ERR_NULL
    assert fn(E=256, k=8, n_group=8, topk_group=8, group_score=TOP2SUM) == ERR_NULL   # every group allowed
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
        assert gate(n_group=4, topk_group=4, ptrs=ptrs) == ERR_NULL, i      # also where the unlimited kernel would serve


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
        assert gate_route(n_group=4, topk_group=4, ptrs=ptrs) == ERR_NULL, i


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_validate_moe_gate_limited():
    x, b = meta(5, 8), meta(8, dtype=torch.float32)
    _validate_moe_gate_limited(x, 2, 4, 2, "softmax", None, "max")
    _validate_moe_gate_limited(x.bfloat16(), 4, 4, 2, "sigmoid", b, "top2sum")
    _validate_moe_gate_limited(x.float(), 1, 8, 3, "softmax", b, "max", 8)
    _validate_moe_gate_limited(meta(3, 1024), 64, 64, 4, "softmax", None, "top2sum", 1024)
    _validate_moe_gate_limited(x, 8, 1, 1, "softmax", None, "top2sum")
    V, T = ValueError, TypeError
    #      exc, logits, k, n_group, topk_group, scoring, bias, group_score, num_experts
    bad = [(V, meta(40), 2, 4, 2, "softmax", None, "max", None), (T, x.double(), 2, 4, 2, "softmax", None, "max", None),
           (V, x, 2, 4, 2, "tanh", None, "max", None), (V, x, 2, 4, 2, "softmax", None, "sum", None),
           (V, x, 2, 4, 2, "softmax", None, 0, None), (V, x, 2, 4, 2, "softmax", None, "max", 9),
           (T, x, 2, 4, 2, "softmax", meta(8), "max", None), (V, x, 2, 4, 2, "softmax", meta(9, dtype=torch.float32), "max", None),
           (V, x, 0, 4, 2, "softmax", None, "max", None), (V, x, 9, 1, 1, "softmax", None, "max", None),
           (V, meta(5, 1028), 2, 4, 2, "softmax", None, "max", None), (V, meta(2 ** 26, 8), 2, 4, 2, "softmax", None, "max", None),
           (V, x, 2, 0, 1, "softmax", None, "max", None), (V, meta(5, 130), 2, 65, 2, "softmax", None, "max", None),
           (V, x, 2, 3, 2, "softmax", None, "max", None), (V, x, 2, 4, 0, "softmax", None, "max", None),
           (V, x, 2, 4, 5, "softmax", None, "max", None), (V, x, 3, 4, 1, "softmax", None, "max", None),
           (V, x, 1, 8, 3, "softmax", None, "top2sum", None)]
    for exc, xx, k, n_group, topk_group, scoring, bias, group_score, E in bad:
        with pytest.raises(exc):
            _validate_moe_gate_limited(xx, k, n_group, topk_group, scoring, bias, group_score, E)
    # the public functions validate before any device call, then refuse tensors that are not on a GPU
    for fn in (flute_amd.moe_gate_limited, flute_amd.moe_gate_route_limited):
        with pytest.raises(T):
            fn(x.double(), 2, 4, 2)
        with pytest.raises(V):
            fn(x, 3, 4, 1)
        with pytest.raises(V):
            fn(x, 2, 4, 2, group_score="mean")
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x, 2, 4, 2)
        with pytest.raises(RuntimeError, match="GPU"):
            fn(torch.zeros(5, 8), 2, 4, 2, bias=torch.zeros(8), group_score="top2sum")
    with pytest.raises(V):
        flute_amd.moe_gate_route_limited(x, 2, 4, 2, 7)
    assert list(inspect.signature(flute_amd.moe_gate_limited).parameters) == \
        ["logits", "k", "n_group", "topk_group", "scoring", "renormalize", "bias", "scale", "group_score"]
    assert list(inspect.signature(flute_amd.moe_gate_route_limited).parameters) == \
        ["logits", "k", "n_group", "topk_group", "num_experts", "scoring", "renormalize", "bias", "scale", "group_score"]
    for fn in (flute_amd.moe_gate_limited, flute_amd.moe_gate_route_limited):
        sig = inspect.signature(fn).parameters
        assert (sig["scoring"].default, sig["renormalize"].default, sig["bias"].default, sig["scale"].default,
                sig["group_score"].default) == ("softmax", False, None, 1.0, "max")


def test_reference_on_a_hand_worked_row():
    """Sigmoid of ln 3, -ln 3, 0, 0: s = 3/4, 1/4, 1/2, 1/2, in two groups of two."""
    x = torch.tensor([[math.log(3.0), -math.log(3.0), 0.0, 0.0]], dtype=torch.float64)
    close = lambda got, want: torch.allclose(got, torch.tensor([want], dtype=torch.float64), rtol=1e-14, atol=0)
    # max: group 0 wins on 3/4, and expert 1 at 1/4 is taken over the 1/2's of the group that lost
    assert L.group_keys(x, 2, "sigmoid").tolist() == [[math.log(3.0), 0.0]]
    assert L.allowed_mask(x, 2, 1, "sigmoid").tolist() == [[True, True, False, False]]
    ids, w = L.gate_limited(x, 2, 2, 1, "sigmoid")
    assert ids.tolist() == [[0, 1]] and close(w, [0.75, 0.25])
    assert R.gate(x, 2, "sigmoid")[0].tolist() == [[0, 2]]                  # the unlimited choice differs
    # top2sum: the sums are 1 and 1, the tie goes to group 0
    assert close(L.group_keys(x, 2, "sigmoid", None, "top2sum"), [1.0, 1.0])
    ids, w = L.gate_limited(x, 2, 2, 1, "sigmoid", group_score="top2sum")
    assert ids.tolist() == [[0, 1]] and close(w, [0.75, 0.25])
    # with the bias the sums are 1 and 3/2: group 1, and the bias enters no weight
    bias = torch.tensor([0.0, 0.0, 0.25, 0.25])
    assert close(L.group_keys(x, 2, "sigmoid", bias, "top2sum"), [1.0, 1.5])
    ids, w = L.gate_limited(x, 2, 2, 1, "sigmoid", True, bias, 1.0, "top2sum")
    assert ids.tolist() == [[2, 3]] and close(w, [0.5, 0.5])
    ids, w = L.gate_limited(x, 2, 2, 1, "sigmoid", False, bias, 2.5, "top2sum")
    assert ids.tolist() == [[2, 3]] and close(w, [1.25, 1.25])
    # separation: the tie of the two sums is none, the biased row is
    assert L.separated_limited(x, 2, 2, 1, "sigmoid", None, "top2sum").tolist() == [False]
    assert L.separated_limited(x, 2, 2, 1, "sigmoid", bias, "top2sum").tolist() == [False]      # experts 2 and 3 tie
    assert L.separated_limited(x, 1, 2, 1, "sigmoid", bias, "top2sum").tolist() == [False]      # ... also as chosen / left out
    apart = torch.tensor([0.0, 0.0, 0.25, 0.5])
    assert L.separated_limited(x, 2, 2, 1, "sigmoid", apart, "top2sum").tolist() == [True]
    assert L.separated_limited(x, 2, 2, 2, "sigmoid", None, "top2sum").tolist() == [False]      # every group: the experts' 1/2's tie
    assert L.separated_limited(x, 2, 2, 1, "sigmoid", None, "top2sum", exact_too=False).tolist() == [False]   # the sums are rounded
    assert L.separated_limited(torch.zeros(1, 4), 2, 2, 1, exact_too=False).tolist() == [True]   # exact keys: ties are defined
    assert L.separated_limited(x, 2, 2, 1, "sigmoid").tolist() == [True]                         # k = topk_group gs: one gap
    # a NaN or -inf group ranks last, in index order; an expert of a group left out loses to an allowed -inf
    nan, inf = float("nan"), float("inf")
    z = torch.tensor([[nan, nan, -inf, -inf, -5.0, -6.0, 9.0, nan]], dtype=torch.float64)
    assert L.gate_limited(z, 2, 4, 3)[0].tolist() == [[6, 4]]
    assert L.gate_limited(z, 6, 4, 3)[0].tolist() == [[6, 4, 5, 0, 1, 7]]                        # groups 3, 2, 0; never 2 or 3
    assert L.gate_limited(z, 2, 4, 1, group_score="top2sum", scoring="sigmoid")[0].tolist() == [[4, 5]]   # 9 + NaN is -inf


@pytest.mark.parametrize("group_score", ["max", "top2sum"])
def test_reference_with_every_group_allowed_is_moe_gate_ref(group_score):
    gen = torch.Generator().manual_seed(3)
    for T, E, k, n_group in ((4, 8, 3, 4), (3, 60, 7, 6), (2, 256, 8, 8), (5, 6, 6, 1)):
        x = torch.randn(T, E, generator=gen, dtype=torch.float64)
        x[0, :3] = x[0, 3]                                                   # ties too
        bias = torch.randn(E, generator=gen)
        for scoring in ("softmax", "sigmoid"):
            for b in (None, bias):
                for renorm in (False, True):
                    ids, w = L.gate_limited(x, k, n_group, n_group, scoring, renorm, b, 2.5, group_score)
                    want_ids, want_w = R.gate(x, k, scoring, renorm, b, 2.5)
                    assert torch.equal(ids, want_ids) and torch.equal(w, want_w)
                    assert bool(L.allowed_mask(x, n_group, n_group, scoring, b, group_score).all())


def grouped(E, K, N, bits=4, g=64, tid=0):
    return GroupedFluteLinear(E, K, N, bits, g, tid, torch.device("cpu"), torch.float16)


def test_forward_logits_limited_and_block_arguments():
    sig = inspect.signature(FluteExperts.forward_logits_limited).parameters
    assert list(sig) == ["self", "hidden", "router_logits", "top_k", "n_group", "topk_group", "scoring", "renormalize", "bias",
                         "scale", "group_score"]
    assert (sig["scoring"].default, sig["renormalize"].default, sig["bias"].default, sig["scale"].default,
            sig["group_score"].default) == ("softmax", False, None, 1.0, "max")
    experts = FluteExperts(grouped(4, 256, 512), grouped(4, 256, 512), grouped(4, 512, 256), fused=True, native_routing=True)
    with pytest.raises(ValueError):
        experts.forward_logits_limited(torch.zeros(3, 256), torch.zeros(3, 5), 2, 2, 1)
    with pytest.raises(ValueError):
        experts.forward_logits_limited(torch.zeros(3, 256), torch.zeros(3, 4), 3, 2, 1)       # k > topk_group gs
    router = torch.zeros(4, 256, dtype=torch.float16)
    sig = inspect.signature(FluteSparseMoeBlock.__init__).parameters
    assert list(sig)[-3:] == ["n_group", "topk_group", "group_score"]
    assert (sig["n_group"].default, sig["topk_group"].default, sig["group_score"].default) == (1, 1, "max")
    plain = FluteSparseMoeBlock(router, experts, 2, renormalize=True)
    assert (plain.n_group, plain.topk_group, plain.group_score) == (1, 1, "max")
    block = FluteSparseMoeBlock(router, experts, 2, scoring="sigmoid", bias=torch.zeros(4), scale=2.5, n_group=2, topk_group=1,
                                group_score="top2sum")
    assert (block.n_group, block.topk_group, block.group_score) == (2, 1, "top2sum")
    assert "n_group=2, topk_group=1, group_score=top2sum" in block.extra_repr()
    assert "n_group=1, topk_group=1, group_score=max" in plain.extra_repr()
    for bad in (dict(n_group=0), dict(n_group=3), dict(n_group=65), dict(n_group=2, topk_group=0), dict(n_group=2, topk_group=3),
                dict(n_group=2, topk_group=1, top_k=3), dict(n_group=4, topk_group=2, group_score="top2sum"),
                dict(n_group=2, topk_group=1, group_score="sum"), dict(topk_group=2)):
        args = dict(dict(top_k=2), **bad)
        with pytest.raises(ValueError):
            FluteSparseMoeBlock(router, experts, **args)
    assert "n_group" in FluteSparseMoeBlock.__doc__ and "dense torch op" in FluteSparseMoeBlock.__doc__
    assert "not covered" not in FluteSparseMoeBlock.__doc__ and "not covered" not in flute_amd.moe_gate.__doc__
