"""Learnable scales and lookup tables on packed layers: the codes stay packed and fixed, the float parameters train.

The reference learns scales on a dense copy (flute/integrations/learnable.py keeps the bf16 weight and rebuilds the
fake-quantized weight every forward).  Here only the 4-bit weight is resident: the forward is `flute.qgemm` itself,
the input gradient is the op's own native backward, and the scale gradient is `flute_amd.qgemm_scale_grad` (a HIP
kernel).  With the codes fixed this is exactly the reference's `absmax` gradient: the code index carries none.

    params = make_scales_learnable(model)     # FluteLinear -> LearnableScalesFluteLinear, in place
    opt = torch.optim.Adam(params, lr=1e-4)
    ...
    freeze_scales(model)                      # back to plain FluteLinear with the learned scales

The lookup table trains the same way (`make_learnable` / `freeze`): an fp32 master codebook - the scalar table
[2^b] or the pair codebook [2^b, 2^b, 2] the kernels read - is rounded to the layer's type every forward, and its
gradient comes from `flute_amd.qgemm_table_grad`, in one launch with the scale gradient when both train.

    params = make_learnable(model, scales=True, table="scalar")   # FluteLinear -> LearnableFluteLinear, in place
    ...
    freeze(model)                             # plain FluteLinear: learned scales, tables and tables2, in the layer's type

The experts of a mixture-of-experts layer train their scales the same way: `qgemm_grouped_learnable_scales`,
`qgemm_grouped_glu_learnable_scales` and `qgemm_grouped_weighted_learnable_scales` are the three grouped ops with a
gradient to the stacks' scales from `flute_amd.qgemm_grouped_scale_grad` (one launch per stack, the row counts stay on the
device).  Their lookup tables train too: `qgemm_grouped_learnable`, `qgemm_grouped_glu_learnable` and
`qgemm_grouped_weighted_learnable` take a stack's fp32 master `codebook` ([E, 2^b] or [E, 2^b, 2^b, 2]) in `table2`'s
place, and their backward adds one `flute_amd.qgemm_grouped_table_grad` launch per stack, which also carries the scale
gradient when both train.  The modules on them are `integrations.moe.make_experts_learnable` / `freeze_experts`.

Not registered by `install_as_flute()`: the reference's `flute.integrations.learnable` is its dense layer.
"""
from typing import List, Optional

import torch

import flute_amd
from flute_amd import ops as _ops
from .base import FluteLinear


def qgemm_learnable_scales(input: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor, table: torch.Tensor,
                           table2: torch.Tensor, workspace: torch.Tensor, num_bits: int, group_size: int,
                           template_id: int, num_sms: int, hadamard_size: int = 0) -> torch.Tensor:
    """`flute.qgemm` (or `flute.qgemm_hadamard` when hadamard_size > 0), differentiable with respect to `input` and
    `scales`.  Gradients for `table` / `table2` are not available and are refused."""
    if table.requires_grad or table2.requires_grad:
        raise RuntimeError("qgemm_learnable_scales: no gradient for table / table2 (only input and scales train)")
    return _Learnable.apply(input, scales, None, weight, table, table2, workspace, num_bits, group_size, template_id,
                            num_sms, hadamard_size)


_ATTRS = ("in_features", "out_features", "num_bits", "group_size", "template_id", "num_sms", "workspace",
          "workspace_lazy_init")


def _share(new: torch.nn.Module, layer: FluteLinear, scales: torch.Tensor) -> None:
    # `new` takes the layer's configuration and its weight / tables / bias tensors; nothing is copied
    for name in _ATTRS:
        setattr(new, name, getattr(layer, name))
    new.register_buffer("weight", layer.weight)
    if isinstance(scales, torch.nn.Parameter):
        new.scales = scales
    else:
        new.register_buffer("scales", scales)
    new.register_buffer("tables", layer.tables)
    new.register_buffer("tables2", layer.tables2)
    if layer.bias is not None:
        new.bias = layer.bias
    else:
        new.register_parameter("bias", None)
    new.train(layer.training)


class LearnableScalesFluteLinear(FluteLinear):
    """A `FluteLinear` whose `scales` is an `nn.Parameter`.  Same state-dict keys and extra state as `FluteLinear`;
    `weight`, `tables`, `tables2` and `bias` are the source layer's tensors, the scales a copy."""

    def __init__(self, layer: FluteLinear) -> None:
        if not isinstance(layer, FluteLinear):
            raise TypeError("LearnableScalesFluteLinear wraps a FluteLinear")
        torch.nn.Module.__init__(self)
        _share(self, layer, torch.nn.Parameter(layer.scales.detach().clone()))

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        num_sms, workspace = self._launch_resources(inputs.device)
        output = qgemm_learnable_scales(inputs, self.weight, self.scales, self.tables, self.tables2, workspace,
                                        self.num_bits, self.group_size, self.template_id, num_sms)
        if self.bias is not None:
            output.add_(self.bias)
        return output


def _swap(module: torch.nn.Module, convert) -> None:
    for name, child in module.named_children():
        new = convert(child)
        if new is not child:
            setattr(module, name, new)
        else:
            _swap(child, convert)


def make_scales_learnable(module: torch.nn.Module) -> List[torch.nn.Parameter]:
    """Replace every `FluteLinear` below `module` by a `LearnableScalesFluteLinear`, in place; returns the scale
    parameters of all learnable layers below `module`, in module order."""
    if type(module) is FluteLinear:
        raise ValueError("make_scales_learnable swaps the layers below a module: pass the module that holds it")
    _swap(module, lambda m: LearnableScalesFluteLinear(m) if type(m) is FluteLinear else m)
    return [m.scales for m in module.modules() if isinstance(m, LearnableScalesFluteLinear)]


def _frozen(layer: LearnableScalesFluteLinear) -> FluteLinear:
    new = FluteLinear.__new__(FluteLinear)
    torch.nn.Module.__init__(new)
    _share(new, layer, layer.scales.detach())
    return new


def freeze_scales(module: torch.nn.Module) -> None:
    """Replace every `LearnableScalesFluteLinear` below `module` by a plain `FluteLinear` holding the learned scales
    as its buffer, in place: the model runs the unchanged `flute.qgemm` path again."""
    if isinstance(module, LearnableScalesFluteLinear):
        raise ValueError("freeze_scales swaps the layers below a module: pass the module that holds it")
    _swap(module, lambda m: _frozen(m) if isinstance(m, LearnableScalesFluteLinear) else m)


def _codebook_tables(codebook: torch.Tensor, num_bits: int, dtype: torch.dtype):
    """(table [2^b] T, table2 [2^b, 2^b, 1] fp32 words of T pairs) of an fp32 master codebook, rounded to T."""
    n = 2 ** num_bits
    if codebook.dtype != torch.float32:
        raise TypeError("qgemm_learnable: the codebook is an fp32 master parameter")
    if tuple(codebook.shape) == (n,):
        table = codebook.detach().to(dtype)
        return table, flute_amd.utils.make_qmap2_from_qmap(table)
    if tuple(codebook.shape) == (n, n, 2):
        pairs = codebook.detach().to(dtype).contiguous()
        return pairs[:, 0, 0].contiguous(), pairs.view(torch.float32)      # `table` is not read by the kernels
    raise ValueError(f"qgemm_learnable: codebook of shape {tuple(codebook.shape)}, expected ({n},) or ({n}, {n}, 2)")


class _Learnable(torch.autograd.Function):
    """`flute.qgemm` / `flute.qgemm_hadamard` with gradients to `scales` and to the fp32 master `codebook`; a codebook of
    None means the caller's `table` / `table2` are used as given (and nothing but input and scales trains)."""

    @staticmethod
    def forward(ctx, input, scales, codebook, weight, table, table2, workspace, num_bits, group_size, template_id,
                num_sms, hadamard_size):
        if codebook is not None:
            table, table2 = _codebook_tables(codebook, num_bits, input.dtype)
        # the op runs on a detached leaf with detached scales, so its own Autograd kernel gives dX unchanged
        with torch.enable_grad():
            x = input.detach().requires_grad_(input.requires_grad)
            if hadamard_size:
                y = flute_amd.qgemm_hadamard(x, weight, scales.detach(), table, table2, workspace, num_bits,
                                             group_size, hadamard_size, template_id, num_sms)
            else:
                y = flute_amd.qgemm(x, weight, scales.detach(), table, table2, workspace, num_bits, group_size,
                                    template_id, num_sms)
        ctx.inner = (x, y)
        ctx.save_for_backward(input, weight, table2, *((scales,) if codebook is not None else ()))   # (scales: dT2 only)
        ctx.cfg = (num_bits, group_size, template_id, num_sms, hadamard_size, codebook is not None and codebook.ndim == 1)
        return y.detach()       # not a differentiable view: the caller may add a bias in place

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, weight, table2, *scales = ctx.saved_tensors
        num_bits, group_size, template_id, num_sms, hadamard_size, scalar = ctx.cfg
        x, y = ctx.inner
        grad_input = grad_scales = grad_codebook = None
        if ctx.needs_input_grad[0]:
            (grad_input,) = torch.autograd.grad(y, x, grad_output)
        want_s, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if want_s or want_t:
            xs = flute_amd.hadamard_transform(input, hadamard_size) if hadamard_size else input
            if want_t:
                out = flute_amd.qgemm_table_grad(grad_output, xs, weight, scales[0].detach(), num_bits, group_size,
                                                 template_id, num_sms, table2=table2, with_scale_grad=want_s)
                grad_codebook, grad_scales = out if want_s else (out, None)
                if scalar:
                    grad_codebook = flute_amd.pair_grad_to_table_grad(grad_codebook)
            else:
                grad_scales = flute_amd.qgemm_scale_grad(grad_output, xs, weight, table2, num_bits, group_size,
                                                         template_id, num_sms)
        return (grad_input, grad_scales, grad_codebook) + (None,) * 9


def qgemm_learnable(input: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor, codebook: torch.Tensor,
                    workspace: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms: int,
                    hadamard_size: int = 0) -> torch.Tensor:
    """`flute.qgemm` (or `flute.qgemm_hadamard` when hadamard_size > 0), differentiable with respect to `input`,
    `scales` and `codebook`.  `codebook` is the fp32 master of the lookup table: [2^b] for a scalar table
    (table2 = make_qmap2_from_qmap) or [2^b, 2^b, 2] for a pair codebook.  The forward rounds it to input.dtype and
    runs the unchanged op; the gradient passes straight through that rounding, as it does for the scales."""
    return _Learnable.apply(input, scales, codebook, weight, None, None, workspace, num_bits, group_size, template_id,
                            num_sms, hadamard_size)


class LearnableFluteLinear(FluteLinear):
    """A `FluteLinear` whose scales and / or lookup table train.  `scales=True` makes `scales` an `nn.Parameter` (a
    copy, in the layer's type); `table="scalar"` / `"pair"` adds the fp32 parameter `codebook` ([2^b] from `tables` /
    [2^b, 2^b, 2] from `tables2`), `None` keeps the table fixed (no `codebook`: the forward reads the layer's
    own `tables` / `tables2`).  `weight`, `tables`, `tables2` and `bias` are the source layer's tensors.  With a
    trained table the state dict carries `codebook` next to `tables` / `tables2`, and those two are stale - the values
    before training - until `freeze` writes the rounded codebook into them.  Like `FluteLinear` the layer passes no
    Hadamard size: a layer whose input is rotated first trains through `qgemm_learnable(..., hadamard_size)`."""

    def __init__(self, layer: FluteLinear, scales: bool = True, table: Optional[str] = "scalar") -> None:
        if not isinstance(layer, FluteLinear):
            raise TypeError("LearnableFluteLinear wraps a FluteLinear")
        if table not in ("scalar", "pair", None):
            raise ValueError("table is 'scalar', 'pair' or None")
        torch.nn.Module.__init__(self)
        _share(self, layer, torch.nn.Parameter(layer.scales.detach().clone()) if scales else layer.scales)
        self.table_mode = table
        if table is None:
            return                                    # the fixed table: the layer's own `tables` / `tables2`
        n = 2 ** layer.num_bits
        dtype = layer.scales.dtype
        if table == "scalar":
            if not torch.equal(flute_amd.utils.make_qmap2_from_qmap(layer.tables.to(dtype)), layer.tables2):
                raise ValueError("table='scalar': the layer's tables2 is not the pair table of its tables "
                                 "(a pair codebook trains with table='pair')")
            codebook = layer.tables.detach().float()
        else:
            codebook = layer.tables2.detach().contiguous().view(dtype).view(n, n, 2).float()
        self.codebook = torch.nn.Parameter(codebook)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        num_sms, workspace = self._launch_resources(inputs.device)
        if self.table_mode is None:
            output = qgemm_learnable_scales(inputs, self.weight, self.scales, self.tables, self.tables2, workspace,
                                            self.num_bits, self.group_size, self.template_id, num_sms)
        else:
            output = qgemm_learnable(inputs, self.weight, self.scales, self.codebook, workspace, self.num_bits,
                                     self.group_size, self.template_id, num_sms)
        if self.bias is not None:
            output.add_(self.bias)
        return output


def make_learnable(module: torch.nn.Module, scales: bool = True,
                   table: Optional[str] = "scalar") -> List[torch.nn.Parameter]:
    """Replace every `FluteLinear` below `module` by a `LearnableFluteLinear(layer, scales, table)`, in place; returns
    the parameters this makes trainable (scales, then codebook, per layer in module order)."""
    if type(module) is FluteLinear:
        raise ValueError("make_learnable swaps the layers below a module: pass the module that holds it")
    _swap(module, lambda m: LearnableFluteLinear(m, scales, table) if type(m) is FluteLinear else m)
    params = []
    for m in module.modules():
        if isinstance(m, LearnableFluteLinear):
            params += [p for p in (m.scales, getattr(m, "codebook", None)) if isinstance(p, torch.nn.Parameter)]
    return params


def _frozen_learnable(layer: LearnableFluteLinear) -> FluteLinear:
    new = FluteLinear.__new__(FluteLinear)
    torch.nn.Module.__init__(new)
    _share(new, layer, layer.scales.detach())
    if layer.table_mode is not None:
        table, table2 = _codebook_tables(layer.codebook, layer.num_bits, layer.scales.dtype)
        if layer.table_mode == "scalar":
            new.tables = table                        # a pair codebook keeps the source's `tables`: nothing reads it
        new.tables2 = table2
    return new


def freeze(module: torch.nn.Module) -> None:
    """Replace every `LearnableFluteLinear` below `module` by a plain `FluteLinear` whose `scales`, `tables` and
    `tables2` buffers carry the learned values, rounded to the layer's type as every forward rounded them, in place:
    the model runs the unchanged `flute.qgemm` path again, with `FluteLinear`'s state-dict keys."""
    if isinstance(module, LearnableFluteLinear):
        raise ValueError("freeze swaps the layers below a module: pass the module that holds it")
    _swap(module, lambda m: _frozen_learnable(m) if isinstance(m, LearnableFluteLinear) else m)


# ---- the experts' scales: the three grouped ops with a gradient to the stacks' scales - the ops' own autograd functions
# (flute_amd/ops.py), whose scale slot only these entry points open

def _refuse_table_grad(name, *tables):
    if any(t.requires_grad for t in tables):
        raise RuntimeError(f"{name}: no gradient for table2 (only input, row_weight and scales train)")


# The three bodies.  Each serves a pair of entry points, `name` the one that was called: `*_learnable_scales` hands in the
# stack's `table2`, which must not require grad; `*_learnable` (below) hands in None there and the stack's fp32 master
# `codebook`, from which `table2` is built (`_codebook_stack`) before anything is validated.  `layer` = (num_bits, group_size,
# template_id, num_sms).

def _grouped_learnable(name, input, offsets, weight, scales, table2, layer, codebook=None):
    if codebook is not None:
        table2 = _codebook_stack(name, codebook, layer[0], input.dtype, scales)
    _ops._validate_grouped(input, offsets, weight, scales, table2, layer[0], layer[1])
    if codebook is None:
        _refuse_table_grad(name, table2)
    if not _ops._records_grad(input, scales, codebook):
        return flute_amd.qgemm_grouped(input, offsets, weight, scales, table2, *layer)
    return _ops._GroupedFunction.apply(input, scales, codebook, offsets, weight, table2, layer)


def _grouped_weighted_learnable(name, input, offsets, weight, scales, table2, row_weight, layer, native_router_grad,
                                codebook=None):
    if codebook is not None:
        table2 = _codebook_stack(name, codebook, layer[0], input.dtype, scales)
    _ops._validate_grouped_weighted(input, offsets, weight, scales, table2, row_weight, layer[0], layer[1])
    if codebook is None:
        _refuse_table_grad(name, table2)
    if not _ops._records_grad(input, row_weight, scales, codebook):
        return flute_amd.qgemm_grouped_weighted(input, offsets, weight, scales, table2, row_weight, *layer)
    return _ops._GroupedWeightedFunction.apply(input, row_weight, scales, codebook, offsets, weight, table2, layer, None,
                                               bool(native_router_grad))


def _grouped_glu_learnable(name, input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2, layer,
                           rows, pos, blocks, native_glu_grad, gate_codebook=None, up_codebook=None):
    if gate_codebook is not None:
        gate_table2 = _codebook_stack(name, gate_codebook, layer[0], input.dtype, gate_scales)
        up_table2 = _codebook_stack(name, up_codebook, layer[0], input.dtype, up_scales)
    _ops._validate_grouped_glu(input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2,
                               layer[0], layer[1], rows)
    if gate_codebook is None:
        _refuse_table_grad(name, gate_table2, up_table2)
    if not _ops._records_grad(input, gate_scales, up_scales, gate_codebook, up_codebook):
        return _glu_op(blocks)(input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2, *layer,
                               rows=rows, pos=pos, native_glu_grad=native_glu_grad)
    _ops._validate_grouped_glu_pos(input, rows, pos)
    return _ops._GroupedGluFunction.apply(input, gate_scales, up_scales, gate_codebook, up_codebook, rows, pos, offsets,
                                          gate_weight, gate_table2, up_weight, up_table2, layer,
                                          _glu_form(blocks, name, input, rows, gate_weight, gate_scales, layer),
                                          bool(native_glu_grad))


def qgemm_grouped_learnable_scales(input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor,
                                   table2: torch.Tensor, num_bits: int, group_size: int, template_id: int,
                                   num_sms=None) -> torch.Tensor:
    """`flute_amd.qgemm_grouped`, differentiable with respect to `input` and `scales` [E, N, K / g].  The forward is the
    op's launch (the same bits); the backward adds dS = `qgemm_grouped_scale_grad(dY, input, ...)`.  With grad mode off, or
    nothing requiring grad, it is the plain op.  `table2` requiring grad is refused."""
    return _grouped_learnable("qgemm_grouped_learnable_scales", input, offsets, weight, scales, table2,
                              (num_bits, group_size, template_id, num_sms))


def qgemm_grouped_weighted_learnable_scales(input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor,
                                            scales: torch.Tensor, table2: torch.Tensor, row_weight: torch.Tensor,
                                            num_bits: int, group_size: int, template_id: int, num_sms=None,
                                            native_router_grad: bool = False) -> torch.Tensor:
    """`flute_amd.qgemm_grouped_weighted`, differentiable with respect to `input`, `row_weight` and `scales`.  The
    forward is the op's launch; the gradients of `input` and `row_weight` are the op's own (`native_router_grad` as the
    op's: one `moe_weight_grad` launch for the two when `row_weight` trains), and
    dS = `qgemm_grouped_scale_grad(dY, input, ..., row_weight=row_weight)`.  `table2` requiring grad is refused."""
    return _grouped_weighted_learnable("qgemm_grouped_weighted_learnable_scales", input, offsets, weight, scales, table2,
                                       row_weight, (num_bits, group_size, template_id, num_sms), native_router_grad)


def _glu_op(blocks):
    """The public fused GLU op a learnable entry falls back to when nothing records a gradient."""
    return flute_amd.qgemm_grouped_glu_blocks if blocks else flute_amd.qgemm_grouped_glu


def _glu_form(blocks, name, input, rows, gate_weight, gate_scales, layer):
    """`_GroupedGluFunction`'s form for `blocks`: the block launch after its eligibility check (raises), or the op's default."""
    if not blocks:
        return None
    _ops._require_glu_blocks(name, input, rows, gate_weight, gate_scales, layer)
    return _ops._GLU_BLOCKS


def qgemm_grouped_glu_learnable_scales(input: torch.Tensor, offsets: torch.Tensor, gate_weight: torch.Tensor,
                                       gate_scales: torch.Tensor, gate_table2: torch.Tensor, up_weight: torch.Tensor,
                                       up_scales: torch.Tensor, up_table2: torch.Tensor, num_bits: int, group_size: int,
                                       template_id: int, num_sms=None, rows=None, pos=None, blocks=False,
                                       native_glu_grad: bool = False) -> torch.Tensor:
    """`flute_amd.qgemm_grouped_glu`, differentiable with respect to `input`, `gate_scales` and `up_scales`.  The forward is
    the op's launch; the backward is the op's own (gate and up recomputed, dg and du in fp32, the pair-form input gradient)
    plus one `qgemm_grouped_scale_grad` launch per stack on the gathered rows.  The tables requiring grad are refused.
    `blocks=True`: the forward is `flute_amd.qgemm_grouped_glu_blocks`' launch (a shape it does not serve raises); the
    backward is the same.  `native_glu_grad` as the op's: the backward's gather and dg, du from `moe_gather` and `swiglu_grad`."""
    return _grouped_glu_learnable("qgemm_grouped_glu_learnable_scales", input, offsets, gate_weight, gate_scales, gate_table2,
                                  up_weight, up_scales, up_table2, (num_bits, group_size, template_id, num_sms), rows, pos,
                                  blocks, native_glu_grad)


# ---- the experts' lookup tables: the same three functions with the codebook slot open.  `codebook` is a stack's fp32
# master, [E, 2^b] (scalar tables: table2[e] = make_qmap2_from_qmap) or [E, 2^b, 2^b, 2] (pair codebooks); the entry point
# rounds it to input.dtype, builds table2 and runs the unchanged launch - the public op's bits for that table2 - and the
# gradient passes straight through the rounding, as in `_Learnable`.

def _codebook_stack(name, codebook, num_bits, dtype, scales):
    """The built table2 of a stack's codebook, validated: [E, ...] with the scales' E."""
    try:
        table2 = _ops._grouped_codebook_table2(codebook, num_bits, dtype)
    except TypeError:
        raise TypeError(f"{name}: the codebook is an fp32 master parameter") from None
    if scales.ndim != 3 or table2.shape[0] != scales.shape[0]:
        raise ValueError(f"{name}: the codebook's leading dimension is the stack's number of experts")
    return table2


def qgemm_grouped_learnable(input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor,
                            codebook: torch.Tensor, num_bits: int, group_size: int, template_id: int,
                            num_sms=None) -> torch.Tensor:
    """`flute_amd.qgemm_grouped`, differentiable with respect to `input`, `scales` and the stack's fp32 master `codebook`.
    The forward has the op's bits for the table2 built from the rounded codebook; the backward adds ONE
    `qgemm_grouped_table_grad(dY, input, ...)` launch (with the scale gradient in it when the scales train too; a stack
    that trains only scales keeps `qgemm_grouped_scale_grad`), folded per expert for the scalar form."""
    return _grouped_learnable("qgemm_grouped_learnable", input, offsets, weight, scales, None,
                              (num_bits, group_size, template_id, num_sms), codebook)


def qgemm_grouped_weighted_learnable(input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor,
                                     scales: torch.Tensor, codebook: torch.Tensor, row_weight: torch.Tensor,
                                     num_bits: int, group_size: int, template_id: int, num_sms=None,
                                     native_router_grad: bool = False) -> torch.Tensor:
    """`flute_amd.qgemm_grouped_weighted`, differentiable with respect to `input`, `row_weight`, `scales` and the stack's
    fp32 master `codebook`: `qgemm_grouped_weighted_learnable_scales` with the table gradient from
    `qgemm_grouped_table_grad(dY, input, ..., row_weight=row_weight)`.  `native_router_grad` as there."""
    return _grouped_weighted_learnable("qgemm_grouped_weighted_learnable", input, offsets, weight, scales, None, row_weight,
                                       (num_bits, group_size, template_id, num_sms), native_router_grad, codebook)


def qgemm_grouped_glu_learnable(input: torch.Tensor, offsets: torch.Tensor, gate_weight: torch.Tensor,
                                gate_scales: torch.Tensor, gate_codebook: torch.Tensor, up_weight: torch.Tensor,
                                up_scales: torch.Tensor, up_codebook: torch.Tensor, num_bits: int, group_size: int,
                                template_id: int, num_sms=None, rows=None, pos=None, blocks=False,
                                native_glu_grad: bool = False) -> torch.Tensor:
    """`flute_amd.qgemm_grouped_glu`, differentiable with respect to `input`, both stacks' scales and both stacks' fp32
    master codebooks: `qgemm_grouped_glu_learnable_scales` with the table gradients from
    `qgemm_grouped_table_grad(dg, x_sorted, ...)` for gate and `(du, x_sorted, ...)` for up, one launch per stack.
    `blocks` and `native_glu_grad` as there."""
    return _grouped_glu_learnable("qgemm_grouped_glu_learnable", input, offsets, gate_weight, gate_scales, None, up_weight,
                                  up_scales, None, (num_bits, group_size, template_id, num_sms), rows, pos, blocks,
                                  native_glu_grad, gate_codebook, up_codebook)
