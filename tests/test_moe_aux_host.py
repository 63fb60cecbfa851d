"""flute_amd.moe_aux_loss and flute_amd.moe_aux_loss_grad (moe_aux.hip) without a GPU: the three symbols and the header, the
workspace query against its formula, the refusal order of the two calls with null pointers (nothing is launched), the Python
validators on CPU and meta tensors, `FluteSparseMoeBlock.aux_loss`, and the support module's own statements - the header's
gradient formula against fp64 autograd of the definitions, the definitions against the torch chain a user writes, and the derived
bounds against an fp32 restatement summed in torch's order."""
import inspect
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib, ops
from flute_amd.integrations.moe import FluteSparseMoeBlock
from tests import moe_aux_cases as AC
from tests.moe_wide_cases import header_constant

DTYPE, SHAPE, NULL = -7, -4, -9                   # FLUTE_ERR_DTYPE, FLUTE_ERR_SHAPE, FLUTE_ERR_NULL
P = 1                                             # a non-null pointer: the refusals compare pointers with null and read nothing
MAX_CHUNKS = header_constant("FLUTE_MOE_ROUTE_MAX_CHUNKS")
NAMES = ("flute_moe_aux_loss_workspace", "flute_moe_aux_loss", "flute_moe_aux_loss_grad")


def test_symbols_header_and_abi_version():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")) as f:
        text = f.read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(_lib.get(), name)
        assert name + "(" in text
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text and _lib.get().flute_abi_version() == 9
    assert flute_amd.moe_aux_loss is ops.moe_aux_loss and flute_amd.moe_aux_loss_grad is ops.moe_aux_loss_grad
    for phrase in ("divided by k", "load_balancing_loss_func", "ST-MoE"):       # the header says which published loss is which
        assert phrase in text


def test_workspace_query():
    ws = _lib.get().flute_moe_aux_loss_workspace
    for T, E, ct in ((1, 8, 0), (5, 8, 2), (257, 64, 0), (257, 64, 100), (513, 256, 0), (130, 1000, 48), (16384, 256, 0),
                     (2 ** 27 - 1, 1024, 0), (MAX_CHUNKS, 8, 1), (40, 1, 7)):
        assert ws(T, E, ct) == AC.workspace_bytes(T, E, ct or None), (T, E, ct)
    assert AC.auto_chunk(16384) == 32 and AC.auto_chunk(2 ** 27 - 1) == 65536
    assert ws(2 ** 27 - 1, 1024, 0) <= 2048 * 2049 * 4
    for T, E, ct in ((0, 8, 0), (-1, 8, 0), (5, 1025, 0), (5, 0, 0), (5, 8, -1), (2 ** 27, 8, 0), (MAX_CHUNKS + 1, 8, 1)):
        assert ws(T, E, ct) == 0, (T, E, ct)


def test_aux_loss_refusal_order():
    """dtype, then scoring, then the shapes and the chunk, then pointers; nothing is launched."""
    call = _lib.get().flute_moe_aux_loss
    nulls = (None,) * 7                           # logits, ids, workspace, load, importance, losses, stream
    head = lambda dt=0, T=4, E=8, k=2, scoring=0, ct=0: (dt, T, E, k, scoring, ct)
    assert call(*head(dt=3, T=-1), *nulls) == DTYPE
    assert call(*head(scoring=2, T=-1), *nulls) == DTYPE
    for bad in (dict(T=0), dict(T=-1), dict(k=0), dict(k=9), dict(E=128, k=65), dict(E=1025), dict(T=2 ** 26, k=2), dict(ct=-1),
                dict(T=MAX_CHUNKS + 1, ct=1)):
        assert call(*head(**bad), *nulls) == SHAPE, bad
        assert call(*head(**bad), P, P, P, P, P, P, None) == SHAPE, bad
    assert call(*head(), *nulls) == NULL
    assert call(*head(T=MAX_CHUNKS, ct=1), *nulls) == NULL
    assert call(*head(dt=2, T=2 ** 26, k=1, E=1024, scoring=1), *nulls) == NULL
    for missing in range(6):
        ptrs = [P] * 6
        ptrs[missing] = None
        assert call(*head(), *ptrs, None) == NULL, missing


def test_aux_loss_grad_refusal_order():
    call = _lib.get().flute_moe_aux_loss_grad
    nulls = (None,) * 5                           # logits, load, grads, d_logits, stream
    head = lambda dt=0, T=4, E=8, scoring=0: (dt, T, E, scoring)
    assert call(*head(dt=3, T=-1), *nulls) == DTYPE
    assert call(*head(scoring=-1, E=0), *nulls) == DTYPE
    for bad in (dict(T=0), dict(T=-1), dict(E=0), dict(E=1025), dict(T=2 ** 27)):
        assert call(*head(**bad), *nulls) == SHAPE, bad
        assert call(*head(**bad), P, P, P, P, None) == SHAPE, bad
    assert call(*head(dt=1, T=2 ** 27 - 1, E=1024, scoring=1), *nulls) == NULL
    for missing in range(4):
        ptrs = [P] * 4
        ptrs[missing] = None
        assert call(*head(), *ptrs, None) == NULL, missing


def test_validators():
    """Ranks (ValueError), then types (TypeError), then values (ValueError), on CPU and meta tensors."""
    x = torch.zeros(5, 8)
    ids = torch.zeros(5, 2, dtype=torch.int32)
    v = ops._validate_moe_aux_loss
    assert v(x, ids, "softmax", None) == 0 and v(x.half(), ids, "sigmoid", 2) == 2 and v(x.bfloat16(), ids, "softmax", 5) == 5
    assert v(torch.empty(2 ** 20, 1024, device="meta"), torch.empty(2 ** 20, 64, dtype=torch.int32, device="meta"), "sigmoid", None) == 0
    for bad, exc in (((x[0], ids, "softmax", None), ValueError), ((x, ids[0], "softmax", None), ValueError),
                     ((x[0], ids.long(), "softmax", None), ValueError),                # the rank comes first
                     ((x.double(), ids, "softmax", None), TypeError), ((x, ids.long(), "softmax", None), TypeError),
                     ((x, ids, "softmax", 2.0), TypeError), ((x, ids, "softmax", True), TypeError),
                     ((x.double(), ids, "tanh", None), TypeError),                     # the type comes before the value
                     ((x, ids, "tanh", None), ValueError), ((x, ids[:4], "softmax", None), ValueError),
                     ((x[:0], ids[:0], "softmax", None), ValueError),                  # T >= 1
                     ((x[:, :1], ids, "softmax", None), ValueError),                   # k > E
                     ((x, ids[:, :0], "softmax", None), ValueError),                   # k >= 1
                     ((x, ids, "softmax", 0), ValueError), ((x, ids, "softmax", -3), ValueError),
                     ((torch.empty(MAX_CHUNKS + 1, 8, device="meta"), torch.empty(MAX_CHUNKS + 1, 2, dtype=torch.int32, device="meta"),
                       "softmax", 1), ValueError),
                     ((torch.empty(4, 1025, device="meta"), torch.empty(4, 2, dtype=torch.int32, device="meta"), "softmax", None),
                      ValueError),
                     ((torch.empty(2 ** 26, 8, device="meta"), torch.empty(2 ** 26, 2, dtype=torch.int32, device="meta"), "softmax",
                       None), ValueError)):
        with pytest.raises(exc):
            v(*bad)
    load, grads = torch.zeros(8, dtype=torch.int32), torch.zeros(2)
    v = ops._validate_moe_aux_loss_grad
    v(x, load, grads, "softmax")
    v(x.half(), load, grads, "sigmoid")
    for bad, exc in (((x[0], load, grads, "softmax"), ValueError), ((x, load[None], grads, "softmax"), ValueError),
                     ((x, load, grads[0], "softmax"), ValueError), ((x.double(), load, grads, "softmax"), TypeError),
                     ((x, load.long(), grads, "softmax"), TypeError), ((x, load, grads.half(), "softmax"), TypeError),
                     ((x, load.long(), grads, "tanh"), TypeError), ((x, load, grads, "tanh"), ValueError),
                     ((x, load[:7], grads, "softmax"), ValueError), ((x, load, torch.zeros(3), "softmax"), ValueError),
                     ((x[:0], load, grads, "softmax"), ValueError)):
        with pytest.raises(exc):
            v(*bad)
    # host tensors pass the validators and are refused by the device check, before anything is allocated or launched
    with pytest.raises(RuntimeError, match="flute_amd.moe_aux_loss: all tensors must live on the same GPU"):
        flute_amd.moe_aux_loss(x, ids)
    with pytest.raises(RuntimeError, match="flute_amd.moe_aux_loss: all tensors must live on the same GPU"):
        flute_amd.moe_aux_loss(x.clone().requires_grad_(), ids, "sigmoid", 2)
    with pytest.raises(RuntimeError, match="flute_amd.moe_aux_loss_grad: all tensors must live on the same GPU"):
        flute_amd.moe_aux_loss_grad(x, load, grads)
    with pytest.raises(ValueError):
        flute_amd.moe_aux_loss(x, ids, chunk_tokens=0)


def test_the_grad_op_is_not_differentiable():
    x, load, grads = torch.zeros(5, 8), torch.zeros(8, dtype=torch.int32), torch.zeros(2)
    for args in ((x.clone().requires_grad_(), load, grads), (x, load, grads.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="flute_amd.moe_aux_loss_grad is not differentiable"):
            flute_amd.moe_aux_loss_grad(*args)
    with torch.no_grad():                         # grad mode off - a backward's state: past that refusal, on to the device check
        with pytest.raises(RuntimeError, match="must live on the same GPU"):
            flute_amd.moe_aux_loss_grad(x.clone().requires_grad_(), load, grads)
    sig = inspect.signature(flute_amd.moe_aux_loss).parameters
    assert sig["scoring"].default == "softmax" and sig["chunk_tokens"].default is None


class _Stack(torch.nn.Module):
    """What FluteExperts.__init__ reads of a stack."""

    def __init__(self, k, n):
        super().__init__()
        self.num_experts, self.in_features, self.out_features = 2, k, n
        self.num_bits, self.group_size, self.template_id = 4, 64, 0
        self.scales = torch.zeros(1, dtype=torch.float16)


def test_sparse_moe_block_validates_aux_loss():
    """The switch is the attribute `block.aux_loss` - the constructor's parameter list is pinned by the tests of earlier options -
    and it takes a bool and nothing else."""
    from flute_amd.integrations.moe import FluteExperts, MoeAuxLosses
    experts = FluteExperts(_Stack(64, 128), _Stack(64, 128), _Stack(128, 64), fused=True, native_routing=True)
    block = FluteSparseMoeBlock(torch.zeros(2, 64, dtype=torch.float16), experts, top_k=1)
    assert block.aux_loss is False and "aux_loss" not in inspect.signature(FluteSparseMoeBlock.__init__).parameters
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(TypeError, match="aux_loss"):
            block.aux_loss = bad
        assert block.aux_loss is False
    assert "aux_loss" not in block.extra_repr() and not hasattr(block, "aux")
    block.aux_loss = True
    assert block.aux_loss is True and "aux_loss=True" in block.extra_repr()
    assert not hasattr(block, "aux")                                   # `aux` appears with the first forward that computes it
    block.aux_loss = False
    assert block.aux_loss is False and FluteSparseMoeBlock(torch.zeros(2, 64, dtype=torch.float16), experts, top_k=1).aux_loss is False
    assert MoeAuxLosses._fields == ("balance", "z", "load", "importance")


@pytest.mark.parametrize("scoring", AC.SCORINGS)
def test_the_headers_formula_is_the_gradient_of_the_definitions(scoring):
    """The header's two lines, restated in fp64, against torch.autograd.grad of the definitions in fp64."""
    for i, (T, E, k, spread, _) in enumerate(AC.SHAPES):
        logits, ids = AC.draw(T, E, k, spread, torch.float64, 300 + i)
        g_b, g_z = (float(g) for g in AC.draw_grads(310 + i))
        got = AC.aux_grad_formula(logits, AC.load_of(ids, E), g_b, g_z, scoring)
        ref = AC.aux_autograd(logits, ids, g_b, g_z, scoring)
        assert float((got - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max())), (T, E, k)


@pytest.mark.parametrize("scoring", AC.SCORINGS)
def test_the_definitions_are_the_chain_a_user_writes(scoring):
    """In fp64 on fp32 logits the definitions and the Hugging Face chain are one function, values and gradient."""
    for i, (T, E, k, spread, _) in enumerate(AC.SHAPES):
        logits, ids = AC.draw(T, E, k, spread, torch.float32, 320 + i)
        balance, z, _, _ = AC.aux_forward(logits, ids, scoring)
        x = logits.clone().requires_grad_()
        cb, cz = AC.torch_chain(x, ids, scoring)
        assert abs(float(cb.detach()) - float(balance)) <= 1e-5 * float(balance)
        assert abs(float(cz.detach()) - float(z)) <= 1e-5 * float(z) + 1e-12
        (cb + 0.5 * cz).backward()
        ref = AC.aux_grad_formula(logits, AC.load_of(ids, E), 1.0, 0.5, scoring)
        assert float((x.grad.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), (T, E, k)


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("scoring", AC.SCORINGS)
def test_the_bounds_hold_for_an_fp32_restatement_in_torchs_order(scoring, dtype):
    """The derived bounds hold for any order of fp32 additions; torch's fp32 restatement of the definitions is one.  The GPU test
    asks the kernels for no more than this asks of torch."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, (T, E, k, spread, _) in enumerate(AC.SHAPES):
        logits, ids = AC.draw(T, E, k, spread, dtype, 330 + i)
        ref, (b_bound, z_bound, imp_bound) = AC.forward_bounds(logits, ids, scoring)
        got = AC.aux_forward(logits, ids, scoring, torch.float32)
        g_b, g_z = (float(g) for g in AC.draw_grads(340 + i))
        dref, dbound = AC.backward_bound(logits, ref[2], g_b, g_z, scoring)
        dgot = AC.aux_grad_formula(logits, ref[2], g_b, g_z, scoring, torch.float32).to(dtype)
        ratios = (AC.worst_ratio(got[0], ref[0], b_bound), AC.worst_ratio(got[1], ref[1], z_bound),
                  AC.worst_ratio(got[3], ref[3], imp_bound), AC.worst_ratio(dgot, dref, dbound))
        print("fp32 restatement %s %s T=%d E=%d: balance %.3f z %.3f importance %.3f d_logits %.3f" % (scoring, dtype, T, E, *ratios))
        worst = [max(a, b) for a, b in zip(worst, ratios)]
    assert max(worst) <= 1.0, worst
