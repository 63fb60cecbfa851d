"""Learnable scales on packed layers: the codes stay packed and fixed, only the scales train.

The reference learns scales on a dense copy (flute/integrations/learnable.py keeps the bf16 weight and rebuilds the
fake-quantized weight every forward).  Here only the 4-bit weight is resident: the forward is `flute.qgemm` itself,
the input gradient is the op's own native backward, and the scale gradient is `flute_amd.qgemm_scale_grad` (a HIP
kernel).  With the codes fixed this is exactly the reference's `absmax` gradient: the code index carries none.

    params = make_scales_learnable(model)     # FluteLinear -> LearnableScalesFluteLinear, in place
    opt = torch.optim.Adam(params, lr=1e-4)
    ...
    freeze_scales(model)                      # back to plain FluteLinear with the learned scales

Not registered by `install_as_flute()`: the reference's `flute.integrations.learnable` is its dense layer.
"""
from typing import List

import torch

import flute_amd
from .base import FluteLinear


class _LearnableScales(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, scales, weight, table, table2, workspace, num_bits, group_size, template_id, num_sms,
                hadamard_size):
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
        ctx.save_for_backward(input, weight, table2)
        ctx.cfg = (num_bits, group_size, template_id, num_sms, hadamard_size)
        return y.detach()       # not a differentiable view: the caller may add a bias in place

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, weight, table2 = ctx.saved_tensors
        num_bits, group_size, template_id, num_sms, hadamard_size = ctx.cfg
        x, y = ctx.inner
        grad_input = grad_scales = None
        if ctx.needs_input_grad[0]:
            (grad_input,) = torch.autograd.grad(y, x, grad_output)
        if ctx.needs_input_grad[1]:
            xs = flute_amd.hadamard_transform(input, hadamard_size) if hadamard_size else input
            grad_scales = flute_amd.qgemm_scale_grad(grad_output, xs, weight, table2, num_bits, group_size,
                                                     template_id, num_sms)
        return grad_input, grad_scales, None, None, None, None, None, None, None, None, None


def qgemm_learnable_scales(input: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor, table: torch.Tensor,
                           table2: torch.Tensor, workspace: torch.Tensor, num_bits: int, group_size: int,
                           template_id: int, num_sms: int, hadamard_size: int = 0) -> torch.Tensor:
    """`flute.qgemm` (or `flute.qgemm_hadamard` when hadamard_size > 0), differentiable with respect to `input` and
    `scales`.  Gradients for `table` / `table2` are not available and are refused."""
    if table.requires_grad or table2.requires_grad:
        raise RuntimeError("qgemm_learnable_scales: no gradient for table / table2 (only input and scales train)")
    return _LearnableScales.apply(input, scales, weight, table, table2, workspace, num_bits, group_size,
                                  template_id, num_sms, hadamard_size)


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
        if self.workspace_lazy_init:
            num_sms = flute_amd.utils.get_device_num_sms(inputs.device)
            workspace = flute_amd.utils.get_workspace_streamk(inputs.device)
        else:
            num_sms, workspace = self.num_sms, self.workspace
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
