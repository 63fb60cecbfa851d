"""flute_amd - MI355X (gfx950) implementation of the `flute.qgemm` hot path.

Same operator surface as HanGuo97/flute v0.4.2 (flute/__init__.py:12-69):
`qgemm`, `qgemm_hadamard` (handles to `torch.ops.flute.qgemm_raw_simple[_hadamard]`)
and `TEMPLATE_CONFIGS` keyed `(num_bits, template_id)`.  The device code is a
hand-written HIP library behind a C ABI (include/flute_amd.h); importing this
package fails loudly if that library has not been built.
"""
from typing import Callable, cast

import torch

from . import _lib
from . import ops

__version__ = "0.1.0"

_lib.get()   # fail at import time, not at first call, when the HIP library is missing

qgemm = cast(Callable[..., torch.Tensor], torch.ops.flute.qgemm_raw_simple.default)
qgemm_hadamard = cast(Callable[..., torch.Tensor], torch.ops.flute.qgemm_raw_simple_hadamard.default)
hadamard_transform = ops.hadamard_transform
# the gradient of a packed layer's scales [N, K / g] (a plain function over the C ABI, not a torch op)
qgemm_scale_grad = ops.qgemm_scale_grad
# the gradient of a packed layer's pair codebook [2^b, 2^b, 2] fp32 (optionally with the scale gradient, one launch),
# and its fold onto a scalar table [2^b]
qgemm_table_grad = ops.qgemm_table_grad
pair_grad_to_table_grad = ops.pair_grad_to_table_grad
# qgemm for the E stacked experts of a mixture-of-experts layer over rows sorted by expert, one launch (the row offsets
# stay on the device); modules on top of it: flute_amd.integrations.moe
qgemm_grouped = ops.qgemm_grouped
qgemm_grouped_glu = ops.qgemm_grouped_glu
qgemm_grouped_glu_blocks = ops.qgemm_grouped_glu_blocks     # the same launch on 128-row blocks, for prefill / training row counts
qgemm_grouped_weighted = ops.qgemm_grouped_weighted
# their input gradient, one launch over the packed stacks (contracts over N); the grouped and mixture-of-experts functions
# here backpropagate through it to activations, routing weights and router logits
qgemm_grouped_input_grad = ops.qgemm_grouped_input_grad
# the gradient of a stack's scales [E, N, K / g], one launch over the same device-side row table; the entry points that train
# the experts' scales through it: flute_amd.integrations.learnable.qgemm_grouped*_learnable_scales, make_experts_learnable
qgemm_grouped_scale_grad = ops.qgemm_grouped_scale_grad
qgemm_grouped_table_grad = ops.qgemm_grouped_table_grad
grouped_pair_grad_to_table_grad = ops.grouped_pair_grad_to_table_grad
# the routing around them, one launch each: the router's choice [T, k] -> offsets, rows, row_weight, pos, perm (a stable
# counting sort on the device), and the sorted rows of the down projection summed per token in fp32 with one rounding
moe_route = ops.moe_route
moe_combine = ops.moe_combine
# the two streams of the fused GLU launch's backward that are not GEMMs, one launch each (the ops' `native_glu_grad=True` runs them):
# the row gather, moe_combine's transpose, and (dg, du) from g, u and the gradient of silu(g) u
moe_gather = ops.moe_gather
swiglu_grad = ops.swiglu_grad
# the router's backward, one launch each (the ops' `native_router_grad=True` runs them): d row_weight and the weighted input gradient
# from the unweighted one, and d logits of the four gating ops from the gradients of their weights / row_weight
moe_weight_grad = ops.moe_weight_grad
moe_gate_grad = ops.moe_gate_grad
# the gating in front of them: router logits [T, E] -> (ids, weights) with a defined tie order, one launch; and the same launch
# carried on through moe_route's sort: from logits to every routing array
moe_gate = ops.moe_gate
moe_gate_route = ops.moe_gate_route
moe_gate_limited = ops.moe_gate_limited
moe_gate_route_limited = ops.moe_gate_route_limited
# the routing over many workgroups, for prefill and training token counts: the same arrays bit for bit, three launches
moe_route_wide = ops.moe_route_wide
moe_gate_route_wide = ops.moe_gate_route_wide
# the router's auxiliary losses: (balance, z, load, importance) from the logits and the gate's picks, two launches, and their
# backward with respect to the logits, one launch
moe_aux_loss = ops.moe_aux_loss
moe_aux_loss_grad = ops.moe_aux_loss_grad
# the dense dequantized weight [N, K] in scales.dtype (the nn.Linear layout), bit-identical to utils.reconstruct
dequantize = cast(Callable[..., torch.Tensor], torch.ops.flute_amd.dequantize.default)

_QUANT_MAP_MODE = {1: "kVectorized   ", 32: "kVectorized_32", 16: "kVectorized_16", 8: "kVectorized_8 "}


def _load_template_configs():
    """Built from the library's own table (single source of truth) in the
    reference's format (flute/codegen_utils.py:110-152)."""
    lib = _lib.get()
    configs = {}
    for bits in (4, 3, 2):
        for tid in range(lib.flute_num_templates(bits)):
            t = _lib.TemplateInfo()
            _lib.check(lib.flute_get_template_info(bits, tid, t))
            configs[(bits, tid)] = {
                "SMs_Multiple": t.sms_multiple,
                "Threads": t.threads,
                "TileM": t.tile_m,
                "TileK": t.tile_k,
                "TileP": t.tile_p,
                "Stages": t.stages,
                "QuantMapMode": _QUANT_MAP_MODE[t.lut_copies] if bits == 4 else "kVectorized   ",
                "AccumulationMode": "kMixed",
                "DecompositionMode": "kSplitK",
                "LutCopies": t.lut_copies,
            }
    return configs


TEMPLATE_CONFIGS = _load_template_configs()

from . import utils  # noqa: E402
from . import tune   # noqa: E402


def install_as_flute() -> None:
    """Make `import flute` resolve to this package (drop-in for integrations that
    import the reference by name, e.g. transformers' HIGGS support)."""
    import sys
    from . import integrations, nf_utils
    sys.modules.setdefault("flute", sys.modules[__name__])
    for name, mod in (("utils", utils), ("tune", tune), ("ops", ops), ("nf_utils", nf_utils),
                      ("integrations", integrations)):
        sys.modules.setdefault(f"flute.{name}", mod)
    from .integrations import base, higgs
    sys.modules.setdefault("flute.integrations.base", base)
    sys.modules.setdefault("flute.integrations.higgs", higgs)
