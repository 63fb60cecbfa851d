"""flute_amd.moe_weight_grad and flute_amd.moe_gate_grad (router_grad.hip) without a GPU: the ABI, the refusal order, the
validators, the `native_router_grad` keyword's defaults and the module's requirement, and the header's gate-gradient formula
against fp64 autograd of the documented gate formula."""
import inspect
import itertools

import pytest
import torch

import flute_amd
from flute_amd import _lib, ops
from flute_amd.integrations import learnable
from flute_amd.integrations.moe import FluteExperts, FluteSparseMoeBlock
from tests import router_grad_cases as RC

DTYPE, SHAPE, NULL = -7, -4, -9                   # FLUTE_ERR_DTYPE, FLUTE_ERR_SHAPE, FLUTE_ERR_NULL
P = 1                                             # a non-null pointer: the refusals compare pointers with null and read nothing


def test_symbols_and_abi_version():
    for name in ("flute_moe_weight_grad", "flute_moe_gate_grad"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.get(), name)
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.moe_weight_grad is ops.moe_weight_grad and flute_amd.moe_gate_grad is ops.moe_gate_grad


def test_moe_weight_grad_refusal_order():
    """dtype, then shape, then the empty launch, then pointers; nothing is launched."""
    call = _lib.get().flute_moe_weight_grad
    nulls = (None,) * 7                           # dHp, H, row_weight, offsets, d_row_weight, dH, stream
    assert call(2, -1, 12, 0, *nulls) == DTYPE    # (FLUTE_F32; the bad shape behind it is not reached)
    assert call(0, -1, 8, 0, *nulls) == SHAPE
    assert call(0, 4, -8, 0, *nulls) == SHAPE
    assert call(1, 4, 12, 0, *nulls) == SHAPE     # K % 8
    assert call(0, 4, 8, -1, None, None, None, P, None, None, None) == SHAPE     # offsets given: E < 0
    assert call(0, 4, 8, -1, *nulls) == NULL      # offsets null: E is ignored
    assert call(0, 0, 8, 0, *nulls) == 0 and call(1, 4, 0, 0, *nulls) == 0 and call(0, 0, 12, 0, *nulls) == SHAPE
    assert call(0, 4, 8, 0, None, P, None, None, P, None, None) == NULL          # dHp
    assert call(0, 4, 8, 0, P, None, None, None, P, None, None) == NULL          # H
    assert call(0, 4, 8, 0, P, P, None, None, None, None, None) == NULL          # d_row_weight
    assert call(0, 4, 8, 0, P, P, P, None, P, None, None) == NULL                # row_weight without dH
    assert call(0, 4, 8, 0, P, P, None, None, P, P, None) == NULL                # dH without row_weight


def test_moe_gate_grad_refusal_order():
    call = _lib.get().flute_moe_gate_grad
    nulls = (None,) * 7                           # logits, ids, d_weights, d_row_weight, pos, d_logits, stream
    head = lambda dt=0, T=4, E=8, k=2, scoring=0: (dt, T, E, k, scoring, 0, 1.0)
    assert call(*head(dt=3, T=-1), *nulls) == DTYPE
    assert call(*head(scoring=2, T=-1), *nulls) == DTYPE
    for bad in (dict(T=-1), dict(k=0), dict(k=9), dict(E=128, k=65), dict(E=1025), dict(T=2 ** 26, k=2)):
        assert call(*head(**bad), *nulls) == SHAPE, bad
    assert call(*head(T=0), *nulls) == 0
    assert call(*head(), *nulls) == NULL
    assert call(*head(), None, P, P, None, None, P, None) == NULL                # logits
    assert call(*head(), P, None, P, None, None, P, None) == NULL                # ids
    assert call(*head(), P, P, P, None, None, None, None) == NULL                # d_logits
    assert call(*head(), P, P, None, None, None, P, None) == NULL                # no gradient source
    assert call(*head(), P, P, P, P, None, P, None) == NULL                      # d_row_weight without pos
    assert call(*head(), P, P, None, None, P, P, None) == NULL                   # pos without d_row_weight


def test_validators():
    g = torch.zeros(4, 16, dtype=torch.float16)
    rw = torch.zeros(4)
    off = torch.zeros(3, dtype=torch.int32)
    v = ops._validate_moe_weight_grad
    v(g, g, rw, None, True)
    v(g, g, rw, off, True)
    v(g, g, None, off, False)
    for bad, exc in (((g[0], g, rw, None, True), ValueError), ((g, g[:, :8], rw, None, True), ValueError),
                     ((g[:, :12], g[:, :12], rw, None, True), ValueError), ((g, g, rw[:3], None, True), ValueError),
                     ((g, g, rw[None], None, True), ValueError), ((g, g, None, None, True), ValueError),
                     ((g, g, rw, off[:0], True), ValueError), ((g, g, rw, off[None], True), ValueError),
                     ((g.float(), g.float(), rw, None, True), TypeError), ((g, g.bfloat16(), rw, None, True), TypeError),
                     ((g, g, rw.double(), None, True), TypeError), ((g, g, rw, off.long(), True), TypeError)):
        with pytest.raises(exc):
            v(*bad)
    x = torch.zeros(5, 8)
    ids = torch.zeros(5, 2, dtype=torch.int32)
    q, drw, pos = torch.zeros(5, 2), torch.zeros(10), torch.zeros(5, 2, dtype=torch.int32)
    v = ops._validate_moe_gate_grad
    v(x, ids, q, "softmax", None, None)
    v(x.half(), ids, None, "sigmoid", drw, pos)
    v(x.bfloat16(), ids, q, "sigmoid", drw, pos)
    for bad, exc in (((x[0], ids, q, "softmax", None, None), ValueError), ((x, ids[:4], q, "softmax", None, None), ValueError),
                     ((x, ids, q, "tanh", None, None), ValueError), ((x, ids, q[:, :1], "softmax", None, None), ValueError),
                     ((x[:, :1], ids, q, "softmax", None, None), ValueError),          # k > E
                     ((x, ids, None, "softmax", None, None), ValueError),              # no source
                     ((x, ids, q, "softmax", drw, None), ValueError), ((x, ids, q, "softmax", None, pos), ValueError),
                     ((x, ids, q, "softmax", drw[:9], pos), ValueError), ((x, ids, q, "softmax", drw, pos[:4]), ValueError),
                     ((x.double(), ids, q, "softmax", None, None), TypeError), ((x, ids.long(), q, "softmax", None, None), TypeError),
                     ((x, ids, q.half(), "softmax", None, None), TypeError), ((x, ids, q, "softmax", drw.half(), pos), TypeError),
                     ((x, ids, q, "softmax", drw, pos.long()), TypeError)):
        with pytest.raises(exc):
            v(*bad)
    # moe_combine's rows
    y = torch.zeros(10, 16, dtype=torch.float16)
    off9 = torch.zeros(9, dtype=torch.int32)
    rows = torch.zeros(10, dtype=torch.int32)
    ops._validate_moe_combine(y, pos, off9, rows)
    ops._validate_moe_combine(y, pos, off9)
    with pytest.raises(TypeError):
        ops._validate_moe_combine(y, pos, off9, rows.long())
    with pytest.raises(ValueError):
        ops._validate_moe_combine(y, pos, off9, rows[:9])
    with pytest.raises(ValueError):
        ops._validate_moe_combine(y, pos, off9, rows[None])
    # host tensors pass the validators and are refused by the device check, before anything is launched
    with pytest.raises(RuntimeError, match="flute_amd.moe_weight_grad: all tensors must live on the same GPU"):
        flute_amd.moe_weight_grad(g, g, rw)
    with pytest.raises(RuntimeError, match="flute_amd.moe_gate_grad: all tensors must live on the same GPU"):
        flute_amd.moe_gate_grad(x, ids, q)


def test_not_differentiable():
    g = torch.zeros(4, 16, dtype=torch.float16)
    rw = torch.zeros(4)
    for args in ((g.clone().requires_grad_(), g, rw), (g, g.clone().requires_grad_(), rw), (g, g, rw.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="flute_amd.moe_weight_grad is not differentiable"):
            flute_amd.moe_weight_grad(*args)
    x, ids, q = torch.zeros(5, 8), torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5, 2)
    drw, pos = torch.zeros(10), torch.zeros(5, 2, dtype=torch.int32)
    for args in ((x.clone().requires_grad_(), ids, q), (x, ids, q.clone().requires_grad_()),
                 (x, ids, q, "softmax", False, 1.0, drw.clone().requires_grad_(), pos)):
        with pytest.raises(RuntimeError, match="flute_amd.moe_gate_grad is not differentiable"):
            flute_amd.moe_gate_grad(*args)
    with torch.no_grad():                         # grad mode off - a backward's state: past that refusal, on to the device check
        with pytest.raises(RuntimeError, match="must live on the same GPU"):
            flute_amd.moe_gate_grad(x.clone().requires_grad_(), ids, q)


def test_native_router_grad_defaults_to_false_everywhere():
    for fn in (flute_amd.qgemm_grouped_weighted, learnable.qgemm_grouped_weighted_learnable_scales,
               learnable.qgemm_grouped_weighted_learnable, ops._moe_gate_entry, FluteExperts.__init__, FluteExperts.from_linears):
        assert inspect.signature(fn).parameters["native_router_grad"].default is False, fn
    for fn in (ops._grouped_weighted_backward, ops._GroupedWeightedFunction.forward, ops._MoeGateFunction.forward,
               ops._moe_gate_op):
        assert inspect.signature(fn).parameters["native"].default is False, fn
    assert inspect.signature(flute_amd.moe_combine).parameters["rows"].default is None
    assert inspect.signature(ops._MoeCombineFunction.forward).parameters["rows"].default is None
    assert "native_router_grad" not in inspect.signature(FluteSparseMoeBlock.__init__).parameters


class _Stack(torch.nn.Module):
    """What FluteExperts.__init__ reads of a stack."""

    def __init__(self, k, n):
        super().__init__()
        self.num_experts, self.in_features, self.out_features = 2, k, n
        self.num_bits, self.group_size, self.template_id = 4, 64, 0
        self.scales = torch.zeros(1, dtype=torch.float16)


def test_flute_experts_native_router_grad_needs_the_fused_native_path():
    stacks = (_Stack(64, 128), _Stack(64, 128), _Stack(128, 64))
    for fused, native in ((False, False), (True, False), (False, True)):
        with pytest.raises(ValueError, match="native_router_grad"):
            FluteExperts(*stacks, fused=fused, native_routing=native, native_router_grad=True)
    on = FluteExperts(*stacks, fused=True, native_routing=True, native_router_grad=True)
    off = FluteExperts(*stacks, fused=True, native_routing=True)
    assert on.native_router_grad is True and off.native_router_grad is False


@pytest.mark.parametrize("scoring,renormalize", list(itertools.product(("softmax", "sigmoid"), (False, True))))
def test_the_headers_formula_is_the_gradient_of_the_gate_formula(scoring, renormalize):
    """Section by section the header's formula, restated in fp64 (tests/router_grad_cases.py, which the GPU test shares), against
    torch.autograd.grad of the documented gate formula in fp64: agreement to a few units of fp64 roundoff."""
    gen = torch.Generator().manual_seed(5)
    for T, E, k, scale in ((1, 8, 1, 1.0), (37, 8, 2, 2.5), (37, 72, 8, 1.0), (5, 256, 8, 2.5)):
        logits = torch.randn(T, E, generator=gen, dtype=torch.float64) * 2
        ids = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)]).int()
        q = torch.randn(T, k, generator=gen, dtype=torch.float64)
        got = RC.gate_grad_formula(logits, ids, q, scoring, renormalize, scale)
        ref = RC.gate_autograd(logits, ids, q, scoring, renormalize, scale)
        assert float((got - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max())), (T, E, k)


def test_the_formula_skips_ids_outside_and_adds_equal_ids():
    gen = torch.Generator().manual_seed(6)
    logits = torch.randn(3, 8, generator=gen, dtype=torch.float64)
    q = torch.randn(3, 3, generator=gen, dtype=torch.float64)
    ids = torch.tensor([[1, 8, 4], [-1, 2, 2], [9, -3, 8]], dtype=torch.int32)
    for scoring, renorm in itertools.product(("softmax", "sigmoid"), (False, True)):
        got = RC.gate_grad_formula(logits, ids, q, scoring, renorm, 1.5)
        ref0 = RC.gate_autograd(logits[:1], torch.tensor([[1, 4]]), q[:1, [0, 2]], scoring, renorm, 1.5)
        ref1 = RC.gate_autograd(logits[1:2], torch.tensor([[2, 2]]), q[1:2, 1:], scoring, renorm, 1.5)
        assert torch.allclose(got[:1], ref0, rtol=0, atol=1e-13) and torch.allclose(got[1:2], ref1, rtol=0, atol=1e-13)
        if not renorm:                            # (renormalised with no slot left: 0 / 0, whatever the arithmetic gives)
            assert torch.all(got[2] == 0)


def test_the_weight_gradients_bound_holds_for_torchs_own_sum():
    """gamma_(K-1) sum |dHp H| bounds every order of fp32 additions of the exact products; torch's fp32 row sum is one."""
    dhp, h, _ = RC.draw_weight_operands(8, 4104, RC.F16, 9)
    ref, bound = RC.weight_grad_bound(dhp, h)
    got = (dhp.float() * h.float()).sum(dim=1)
    assert torch.all((got.double() - ref).abs() <= bound) and float(bound.min()) > 0
    a, b = RC.exact_weight_operands(4, 4104, RC.BF16, 10)
    prod = a.double() * b.double()
    assert torch.equal(prod * 64, (prod * 64).round()) and float(prod.abs().sum(dim=1).max()) < 2.0 ** 18
