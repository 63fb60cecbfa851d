"""flute_amd.swiglu_grad and flute_amd.moe_gather (swiglu_grad.hip) without a GPU: the ABI, the refusal order, the validators,
the `native_glu_grad` keyword's defaults, and the header's error account."""
import inspect

import numpy as np
import pytest
import torch

import flute_amd
from flute_amd import _lib, ops
from flute_amd.integrations import learnable
from flute_amd.integrations.moe import FluteExperts, FluteSparseMoeBlock
from tests import swiglu_grad_cases as SC

DTYPE, SHAPE, NULL = -7, -4, -9                   # FLUTE_ERR_DTYPE, FLUTE_ERR_SHAPE, FLUTE_ERR_NULL


def test_symbols_and_abi_version():
    for name in ("flute_swiglu_grad", "flute_moe_gather"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.get(), name)
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.swiglu_grad is ops.swiglu_grad and flute_amd.moe_gather is ops.moe_gather


def test_swiglu_grad_refusal_order():
    """dtype, then shape, then pointers - all with null pointers, so nothing is launched; empty launches return OK first."""
    call = _lib.get().flute_swiglu_grad
    nulls = (None,) * 7                           # g, u, dh, offsets, dg, du, stream
    assert call(2, -1, 12, 0, *nulls) == DTYPE    # (FLUTE_F32; the bad shape behind it is not reached)
    assert call(0, -1, 8, 0, *nulls) == SHAPE
    assert call(0, 4, -8, 0, *nulls) == SHAPE
    assert call(1, 4, 12, 0, *nulls) == SHAPE     # F % 8
    assert call(0, 2 ** 31 - 1, 2048, 0, *nulls) == SHAPE          # rows x column chunks past 2^31 - 1
    assert call(0, 2 ** 31 - 1, 1024, 0, *nulls) == NULL           # ... and the largest grid that fits
    assert call(0, 4, 8, 0, *nulls) == NULL
    assert call(0, 4, 8, -1, *nulls) == NULL      # offsets null: E is ignored
    assert call(0, 4, 8, -1, None, None, None, 1, None, None, None) == SHAPE    # offsets given (compared with null only): E < 0
    assert call(0, 0, 8, 0, *nulls) == 0 and call(1, 4, 0, 0, *nulls) == 0


def test_moe_gather_refusal_order():
    call = _lib.get().flute_moe_gather
    nulls = (None,) * 5                           # X, rows, offsets, out, stream
    assert call(2, -1, 1, 12, 0, *nulls) == DTYPE
    assert call(0, -1, 1, 8, 0, *nulls) == SHAPE
    assert call(0, 4, -1, 8, 0, *nulls) == SHAPE
    assert call(0, 4, 1, 12, 0, *nulls) == SHAPE
    assert call(0, 4, 0, 8, 0, *nulls) == SHAPE   # rows to gather and nothing to gather them from
    assert call(1, 2 ** 31 - 1, 1, 2048, 0, *nulls) == SHAPE
    assert call(0, 4, 1, 8, 0, *nulls) == NULL
    assert call(0, 4, 1, 8, -1, None, None, 1, None, None) == SHAPE
    assert call(0, 0, 0, 8, 0, *nulls) == 0 and call(0, 4, 1, 0, 0, *nulls) == 0


def test_validators():
    g = torch.zeros(4, 16, dtype=torch.float16)
    off = torch.zeros(3, dtype=torch.int32)
    ops._validate_swiglu_grad(g, g, g, None)
    ops._validate_swiglu_grad(g, g, g, off)
    with pytest.raises(ValueError):
        ops._validate_swiglu_grad(g[0], g, g, None)
    with pytest.raises(ValueError):
        ops._validate_swiglu_grad(g, g[:, :8], g, None)
    with pytest.raises(ValueError):
        ops._validate_swiglu_grad(g[:, :12], g[:, :12], g[:, :12], None)
    with pytest.raises(TypeError):
        ops._validate_swiglu_grad(g.float(), g.float(), g.float(), None)
    with pytest.raises(TypeError):
        ops._validate_swiglu_grad(g, g.bfloat16(), g, None)
    with pytest.raises(TypeError):
        ops._validate_swiglu_grad(g, g, g, off.long())
    with pytest.raises(ValueError):
        ops._validate_swiglu_grad(g, g, g, off[:0])
    with pytest.raises(ValueError):
        ops._validate_swiglu_grad(g, g, g, off[None])
    rows = torch.zeros(5, dtype=torch.int32)
    ops._validate_moe_gather(g, rows, None)
    ops._validate_moe_gather(g, rows, off)
    with pytest.raises(ValueError):
        ops._validate_moe_gather(g[0], rows, None)
    with pytest.raises(ValueError):
        ops._validate_moe_gather(g, rows[None], None)
    with pytest.raises(ValueError):
        ops._validate_moe_gather(g[:, :12], rows, None)
    with pytest.raises(ValueError):
        ops._validate_moe_gather(g[:0], rows, None)
    with pytest.raises(TypeError):
        ops._validate_moe_gather(g, rows.long(), None)
    with pytest.raises(TypeError):
        ops._validate_moe_gather(g.float(), rows, None)
    with pytest.raises(TypeError):
        ops._validate_moe_gather(g, rows, off.long())
    # host tensors pass the validators and are refused by the device check, before anything is launched
    with pytest.raises(RuntimeError, match="flute_amd.swiglu_grad: all tensors must live on the same GPU"):
        flute_amd.swiglu_grad(g, g, g)
    with pytest.raises(RuntimeError, match="flute_amd.moe_gather: all tensors must live on the same GPU"):
        flute_amd.moe_gather(g, rows)


def test_not_differentiable():
    g = torch.zeros(4, 16, dtype=torch.float16)
    rows = torch.zeros(5, dtype=torch.int32)
    for args in ((g.clone().requires_grad_(), g, g), (g, g.clone().requires_grad_(), g), (g, g, g.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="flute_amd.swiglu_grad is not differentiable"):
            flute_amd.swiglu_grad(*args)
    with pytest.raises(RuntimeError, match="flute_amd.moe_gather is not differentiable"):
        flute_amd.moe_gather(g.clone().requires_grad_(), rows)
    with torch.no_grad():                         # grad mode off - a backward's state: past that refusal, on to the device check
        with pytest.raises(RuntimeError, match="must live on the same GPU"):
            flute_amd.swiglu_grad(g.clone().requires_grad_(), g, g)


def test_native_glu_grad_defaults_to_false_everywhere():
    for fn in (flute_amd.qgemm_grouped_glu, flute_amd.qgemm_grouped_glu_blocks, learnable.qgemm_grouped_glu_learnable_scales,
               learnable.qgemm_grouped_glu_learnable, FluteExperts.__init__, FluteExperts.from_linears):
        p = inspect.signature(fn).parameters["native_glu_grad"]
        assert p.default is False, fn
    assert inspect.signature(ops._grouped_glu_backward).parameters["native"].default is False
    assert inspect.signature(ops._GroupedGluFunction.forward).parameters["native"].default is False


def test_sparse_moe_block_signature_is_unchanged():
    assert list(inspect.signature(FluteSparseMoeBlock.__init__).parameters) == \
        ["self", "router_weight", "experts", "top_k", "scoring", "renormalize", "bias", "scale", "n_group", "topk_group",
         "group_score"]


def test_header_states_the_formula_and_the_constant():
    text = SC.header_account()
    for line in ("d   = 1 + expf(-g)", "sig = 1 / d", "ds  = sig * (1 + g * (1 - sig))", "dg  = round_T((dh * u) * ds)",
                 "du  = round_T(dh * sl)", "eps_s = 2^-21"):
        assert line in text, line
    assert SC.header_c() == 5
    # the constant follows from the operation count the header gives: eps (4 |g| + 6 |ds|) <= 6.6 eps (1 + |g|) with |ds| <= 1.1,
    # 2 eps |ds| <= 2.2 eps for the two products - 8.8 eps (1 + |g|) = 4.4 * 2^-23 (1 + |g|) - rounded up
    assert max(4, 6 * 1.1) + 2 * 1.1 <= 2 * SC.header_c()
    g = torch.linspace(-30, 30, 60001, dtype=torch.float64)
    sig = torch.sigmoid(g)
    assert float((sig * (1 + g * (1 - sig))).abs().max()) <= 1.1


def test_the_three_exact_regimes_in_fp32():
    """What the GPU test's exact cases rely on, in numpy's fp32: g = 0; 1 + exp(-g) == 1 for g in [18, 64]; exp(-g) infinite for
    g <= -104."""
    one = np.float32(1)
    assert one + np.exp(np.float32(-0.0)) == np.float32(2)
    for g in range(18, 65):
        assert one + np.exp(np.float32(-g)) == one
    with np.errstate(over="ignore"):
        for g in (-104, -128, -1000, -65504):
            assert np.isinf(np.exp(-np.float32(g)))


@pytest.mark.parametrize("dtype", [SC.F16, SC.BF16])
def test_the_draw_keeps_the_bounds_from_being_vacuous(dtype):
    g, u, dh = SC.draw(300, 1024, dtype, 5)
    _, _, bdg, bdu, vdg, vdu = SC.bounds(g, u, dh, dtype, SC.header_c())
    assert float(vdg.double().mean()) < 0.01 and float(vdu.double().mean()) < 0.01
    # and the torch chain - the default backward's arithmetic - sits inside the same account on the CPU
    rdg, rdu = SC.formula64(g, u, dh)
    tdg, tdu = SC.torch_chain(g, u, dh)
    assert torch.all(((tdg.double() - rdg).abs() <= bdg) | vdg) and torch.all(((tdu.double() - rdu).abs() <= bdu) | vdu)
