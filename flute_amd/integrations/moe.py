"""Mixture-of-experts layers on packed weights: all experts of a projection in one launch.

`GroupedFluteLinear` stacks E `FluteLinear`s of one shape and serves rows sorted by expert through
`flute_amd.qgemm_grouped`; the per-expert row counts never leave the device (`sort_by_expert`
uses ops of fixed output shape only), so a step with changing routing can sit in one captured graph.  The launches serve
decode, prefill and training row counts: the library picks the kernel from the shapes alone - the row form
(qgemm_grouped.h) for decode-sized counts, the block form (qgemm_grouped_blocks.h: 128-row blocks of the dense prefill
kernel) from a mean of 32 - 64 rows per expert on, for the plain and weighted launches of 4- and 2-bit stacks it is eligible
for (`flute_amd.dev.grouped_form` tells which) - so the modules here need no switch: the down projection and the
backward's recompute of gate and up take the block form by themselves.  The fused GLU launch has its block form behind an
entry of its own, `flute_amd.qgemm_grouped_glu_blocks`, and `FluteExperts(fused=True, glu_blocks=...)` opts in: `True` always
(raises where the stacks are not eligible), `"auto"` where `flute_amd.dev.grouped_glu_blocks_form` says it pays for the step's
T k rows (shapes only: no host synchronise), `False` - the default - never: the forward is then bit for bit what it was.  The
backward's two input-gradient launches have their own pair of forms - slabs and, for 4- / 2-bit stacks with K % 256 == 0 from a
mean of 32 - 128 rows per expert on, 128-row x 256-k blocks (qgemm_grouped_input_grad_blocks.h;
`flute_amd.dev.grouped_input_grad_form` tells which) - with equal bits, picked the same way.
`FluteExperts` is the gated MLP of Mixtral / Qwen-MoE / DeepSeek-style blocks on three of them; with `fused=True`
its forward is two launches (`qgemm_grouped_glu`, `qgemm_grouped_weighted`) instead of three and seven torch ops; with
`native_routing=True` the torch ops around them - `sort_by_expert` and its glue before, `zeros_like` and `index_add_`
after - become two more launches (`moe_route`, `moe_combine`): four launches and no torch arithmetic, the same bits
for equal arguments at every top-k, one rounding in the sum over a token's experts.
`FluteExperts.forward_logits` takes what a router produces - logits [T, E] - instead of (topk_ids, topk_weights): the
softmax / sigmoid, the optional correction bias, the top-k with a defined tie order, the renormalisation and the scale
are `moe_gate` (moe_gate.hip), and with `native_routing=True` gating and routing are one launch (`moe_gate_route`), four
launches from logits.  `FluteSparseMoeBlock` is the whole sparse-MoE block: the router's dense GEMM (a torch op) and
`forward_logits`.  DeepSeek's group-limited selection (n_group groups of experts, the topk_group best of them allowed:
DeepSeek-V2 / V3 / R1) is `forward_logits_limited` on `moe_gate_limited` / `moe_gate_route_limited`, the same launch
count, and the block's `n_group`, `topk_group`, `group_score` arguments.

Every path here backpropagates: when `hidden`, `topk_weights` or the router's logits require grad, the launches record
their backward (`flute_amd.ops`): the input gradients of the three projections are `qgemm_grouped_input_grad` launches
(the fused GLU recomputes gate and up with two plain grouped launches and takes both gradients in one pair-form launch),
the gradient of the gather is `moe_combine` under native routing (equal bits at every top-k) and `index_add_` otherwise,
`moe_combine`'s own gradient is a gather, and the gating ops differentiate their formula in fp32 with the chosen ids
held fixed - so layers in front of the block (LoRA on attention, a trainable router) get their gradients.  With grad mode
off, or nothing requiring grad, the forward is exactly the inference path above and stays capturable.  With a trainable router,
`FluteExperts(fused=True, native_routing=True, native_router_grad=True)` runs the torch parts of that backward - d row_weight and the
weighted input gradient, the gate's derivative, `moe_combine`'s gather - as one HIP launch each (router_grad.hip, `moe_gather`).

The experts' scales train: `make_experts_learnable(model)` swaps every `GroupedFluteLinear` for a
`LearnableGroupedFluteLinear` (its `scales` an `nn.Parameter`, the packed codes and tables shared) and `FluteExperts` then
runs its three projections through `integrations.learnable.qgemm_grouped*_learnable_scales`, whose backward adds one
`flute_amd.qgemm_grouped_scale_grad` launch per stack - the row counts stay on the device there too; `freeze_experts(model)`
swaps back to plain stacks holding the learned scales.  Their lookup tables train too:
`make_experts_learnable(model, scales=True, table="scalar" | "pair")` gives every stack an fp32 master `codebook`
([E, 2^b] / [E, 2^b, 2^b, 2]) and the projections run through `qgemm_grouped*_learnable`, whose backward is one
`flute_amd.qgemm_grouped_table_grad` launch per stack - scale gradient included - and `freeze_experts` writes the rounded
codebooks into the plain stacks' `tables` / `tables2`.  The public `flute_amd.qgemm_grouped*` ops still raise on scales or
tables that require grad.

    experts = FluteExperts.from_linears(gates, ups, downs)          # lists of E FluteLinear each
    out = experts(hidden, topk_ids, topk_weights)                   # [T, K], [T, k], [T, k] -> [T, K]
    fast = FluteExperts.from_linears(gates, ups, downs, fused=True) # the same MLP through the fused launches
    four = FluteExperts.from_linears(gates, ups, downs, fused=True, native_routing=True)   # moe_route -> glu -> weighted -> moe_combine
    params = make_experts_learnable(four); ...; freeze_experts(four)                        # train the experts' scales
    params = make_experts_learnable(four, scales=True, table="scalar")                      # ... and their lookup tables
    out = four.forward_logits(hidden, router_logits, top_k=2, renormalize=True)            # moe_gate_route -> glu -> weighted -> moe_combine
    block = FluteSparseMoeBlock(router_weight, four, top_k=2, renormalize=True)             # [E, K] router, out = block(hidden)
    v3 = FluteSparseMoeBlock(router_weight, four, top_k=8, scoring="sigmoid", renormalize=True, bias=correction_bias,
                             scale=2.5, n_group=8, topk_group=4, group_score="top2sum")    # DeepSeek-V3's gating, 256 experts

Not registered by `install_as_flute()`: the reference has no grouped form.
"""
import collections
import functools
from typing import List, Optional, Sequence, Tuple, Union

import torch

import flute_amd
import flute_amd.dev
import flute_amd.utils
from .base import FluteLinear
from .learnable import (_swap, qgemm_grouped_glu_learnable, qgemm_grouped_glu_learnable_scales, qgemm_grouped_learnable,
                        qgemm_grouped_learnable_scales, qgemm_grouped_weighted_learnable,
                        qgemm_grouped_weighted_learnable_scales)


def _stack_num_sms(stack, device):
    """The CU count a stack's launches are planned for: the one it recorded when it was built on a GPU, else `device`'s."""
    return stack.num_sms if stack.num_sms is not None else flute_amd.utils.get_device_num_sms(device)


def sort_by_expert(topk_ids: torch.Tensor, num_experts: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The grouping `qgemm_grouped` takes, from the router's choice topk_ids [T, k]: `perm` [T k] lists the flattened
    (token, slot) pairs by expert, pairs of one expert in their original order (a stable sort), and `offsets`
    [E + 1] int32 are the experts' row ranges in that order.  Token of sorted row i: perm[i] // k.  Ids outside
    [0, E) sort behind every expert, past offsets[E]: no expert serves those rows.
    Ops of fixed output shape on the ids' device only (the counts are a comparison against arange(E) summed over the
    pairs, not `bincount`, whose output length depends on the data and is read back to the host): no host
    synchronise, capturable in a graph."""
    flat = topk_ids.reshape(-1)
    experts = torch.arange(num_experts, device=flat.device, dtype=flat.dtype)
    hit = flat[:, None] == experts                              # [T k, E]
    perm = torch.argsort(torch.where(hit.any(dim=1), flat, num_experts), stable=True)
    offsets = torch.zeros(num_experts + 1, dtype=torch.int32, device=flat.device)
    offsets[1:] = torch.cumsum(hit.sum(dim=0), 0)
    return perm, offsets


class GroupedFluteLinear(torch.nn.Module):
    """E packed layers [N, K] of one num_bits / group_size / template_id / dtype, stacked along a leading expert axis."""

    def __init__(self, num_experts: int, in_features: int, out_features: int, num_bits: int, group_size: int,
                 template_id: int, device: torch.device, dtype: torch.dtype) -> None:
        if dtype not in [torch.float16, torch.bfloat16]:
            raise NotImplementedError
        super().__init__()
        E, K, N = num_experts, in_features, out_features
        n = 2 ** num_bits
        self.num_experts, self.in_features, self.out_features = E, K, N
        self.num_bits, self.group_size, self.template_id = num_bits, group_size, template_id
        self.num_sms = flute_amd.utils.get_device_num_sms(device) if device.type == "cuda" else None
        tables = torch.arange(n, dtype=dtype, device=device)
        self.register_buffer("weight", torch.empty((E, N // 16 * num_bits, K), dtype=torch.int16, device=device))
        self.register_buffer("scales", torch.ones((E, N, K // group_size), dtype=dtype, device=device))
        self.register_buffer("tables", tables.repeat(E, 1))
        self.register_buffer("tables2", flute_amd.utils.make_qmap2_from_qmap(tables).repeat(E, 1, 1, 1))

    @classmethod
    def from_linears(cls, layers: Sequence[FluteLinear]) -> "GroupedFluteLinear":
        if len(layers) == 0:
            raise ValueError("GroupedFluteLinear.from_linears: no layers")
        first = layers[0]
        key = lambda m: (m.in_features, m.out_features, m.num_bits, m.group_size, m.template_id, m.scales.dtype,
                         m.scales.device)
        for i, m in enumerate(layers):
            if not isinstance(m, FluteLinear):
                raise TypeError(f"expert {i}: not a FluteLinear")
            if m.bias is not None:
                raise ValueError(f"expert {i}: a bias is not supported")
            if key(m) != key(first):
                raise ValueError(f"expert {i}: {key(m)} differs from expert 0's {key(first)}")
        new = cls(len(layers), first.in_features, first.out_features, first.num_bits, first.group_size,
                  first.template_id, device=first.scales.device, dtype=first.scales.dtype)
        new.weight.copy_(torch.stack([m.weight for m in layers]))
        new.scales.copy_(torch.stack([m.scales for m in layers]))
        new.tables.copy_(torch.stack([m.tables for m in layers]))
        new.tables2.copy_(torch.stack([m.tables2 for m in layers]))
        return new

    def forward(self, x_sorted: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        num_sms = _stack_num_sms(self, x_sorted.device)
        return flute_amd.qgemm_grouped(x_sorted, offsets, self.weight, self.scales, self.tables2, self.num_bits,
                                       self.group_size, self.template_id, num_sms)

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, in_features={self.in_features}, out_features={self.out_features}, "
                f"num_bits={self.num_bits}, group_size={self.group_size}")


_GROUPED_ATTRS = ("num_experts", "in_features", "out_features", "num_bits", "group_size", "template_id", "num_sms")


def _share_grouped(new: torch.nn.Module, stack: GroupedFluteLinear, scales: torch.Tensor) -> None:
    # `new` takes the stack's configuration and its weight / tables / tables2 tensors; nothing is copied
    for name in _GROUPED_ATTRS:
        setattr(new, name, getattr(stack, name))
    new.register_buffer("weight", stack.weight)
    if isinstance(scales, torch.nn.Parameter):
        new.scales = scales
    else:
        new.register_buffer("scales", scales)
    new.register_buffer("tables", stack.tables)
    new.register_buffer("tables2", stack.tables2)
    new.train(stack.training)


class LearnableGroupedFluteLinear(GroupedFluteLinear):
    """A `GroupedFluteLinear` whose scales and / or lookup tables train.  `scales=True` makes `scales` [E, N, K / g] an
    `nn.Parameter` (a copy); `table="scalar"` / `"pair"` adds the fp32 parameter `codebook` ([E, 2^b] from `tables` /
    [E, 2^b, 2^b, 2] from `tables2`), `None` keeps the tables fixed (no `codebook`).  `weight`, `tables` and `tables2` are
    the source stack's tensors; without a codebook the state-dict keys are `GroupedFluteLinear`'s, with one `codebook`
    comes next to `tables` / `tables2`, which are stale until `freeze_experts` writes the rounded codebook into new ones.
    The forward is `qgemm_grouped_learnable_scales` / `qgemm_grouped_learnable`: the same launch, with the parameter
    gradients from `qgemm_grouped_scale_grad` / `qgemm_grouped_table_grad`."""

    def __init__(self, stack: GroupedFluteLinear, scales: bool = True, table: Optional[str] = None) -> None:
        if not isinstance(stack, GroupedFluteLinear):
            raise TypeError("LearnableGroupedFluteLinear wraps a GroupedFluteLinear")
        if table not in ("scalar", "pair", None):
            raise ValueError("table is 'scalar', 'pair' or None")
        torch.nn.Module.__init__(self)
        _share_grouped(self, stack, torch.nn.Parameter(stack.scales.detach().clone()) if scales else stack.scales)
        self.table_mode = table
        if table is None:
            return                                    # the fixed tables: the stack's own `tables2`
        n = 2 ** stack.num_bits
        dtype = stack.scales.dtype
        if table == "scalar":
            if not torch.equal(flute_amd.ops._grouped_codebook_table2(stack.tables.float(), stack.num_bits, dtype),
                               stack.tables2):
                raise ValueError("table='scalar': an expert's tables2 is not the pair table of its tables "
                                 "(pair codebooks train with table='pair')")
            codebook = stack.tables.detach().float()
        else:
            codebook = stack.tables2.detach().contiguous().view(dtype).view(stack.num_experts, n, n, 2).float()
        self.codebook = torch.nn.Parameter(codebook)

    def forward(self, x_sorted: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        num_sms = _stack_num_sms(self, x_sorted.device)
        if self.table_mode is None:
            return qgemm_grouped_learnable_scales(x_sorted, offsets, self.weight, self.scales, self.tables2,
                                                  self.num_bits, self.group_size, self.template_id, num_sms)
        return qgemm_grouped_learnable(x_sorted, offsets, self.weight, self.scales, self.codebook, self.num_bits,
                                       self.group_size, self.template_id, num_sms)


def make_experts_learnable(module: torch.nn.Module, scales: bool = True,
                           table: Optional[str] = None) -> List[torch.nn.Parameter]:
    """Replace every `GroupedFluteLinear` below `module` by a `LearnableGroupedFluteLinear(stack, scales, table)`, in
    place; returns the parameters of all learnable stacks below `module` (scales, then codebook, per stack in module
    order - with the defaults the scale parameters).  A stack that is learnable already is kept as it is when it was
    made so with these `scales` and `table`, and refused otherwise (`freeze_experts` first): nothing is changed then."""
    if type(module) is GroupedFluteLinear:
        raise ValueError("make_experts_learnable swaps the stacks below a module: pass the module that holds it")
    if table not in ("scalar", "pair", None):
        raise ValueError("table is 'scalar', 'pair' or None")
    for m in module.modules():
        if isinstance(m, LearnableGroupedFluteLinear) and \
                (isinstance(m.scales, torch.nn.Parameter), m.table_mode) != (bool(scales), table):
            raise ValueError("make_experts_learnable: a stack below the module is learnable already with scales=%s, table=%r; "
                             "freeze_experts(module) first" % (isinstance(m.scales, torch.nn.Parameter), m.table_mode))
    _swap(module, lambda m: LearnableGroupedFluteLinear(m, scales, table) if type(m) is GroupedFluteLinear else m)
    params = []
    for m in module.modules():
        if isinstance(m, LearnableGroupedFluteLinear):
            params += [p for p in (m.scales, getattr(m, "codebook", None)) if isinstance(p, torch.nn.Parameter)]
    return params


def _frozen_grouped(stack: LearnableGroupedFluteLinear) -> GroupedFluteLinear:
    new = GroupedFluteLinear.__new__(GroupedFluteLinear)
    torch.nn.Module.__init__(new)
    _share_grouped(new, stack, stack.scales.detach())
    if stack.table_mode is not None:                  # new tensors: the source stack's buffers are not written
        if stack.table_mode == "scalar":
            new.tables = stack.codebook.detach().to(stack.scales.dtype)   # (pair codebooks keep `tables`: nothing reads it)
        new.tables2 = flute_amd.ops._grouped_codebook_table2(stack.codebook, stack.num_bits, stack.scales.dtype)
    return new


def freeze_experts(module: torch.nn.Module) -> None:
    """Replace every `LearnableGroupedFluteLinear` below `module` by a plain `GroupedFluteLinear` holding the learned
    scales - and, where the tables trained, the codebook rounded to the stack's type as every forward rounded it, in
    `tables` / `tables2` - as its buffers, in place: the experts run the unchanged inference launches again."""
    if isinstance(module, LearnableGroupedFluteLinear):
        raise ValueError("freeze_experts swaps the stacks below a module: pass the module that holds it")
    _swap(module, lambda m: _frozen_grouped(m) if isinstance(m, LearnableGroupedFluteLinear) else m)


def _has_codebook(stack) -> bool:
    return getattr(stack, "table_mode", None) is not None


def _table_of(stack):
    """What a fused entry point takes in the table's place: the stack's codebook where it has one, else `tables2`."""
    return stack.codebook if _has_codebook(stack) else stack.tables2


def _check_tristate(name, value) -> None:
    if not (value is False or value is True or (isinstance(value, str) and value == "auto")):
        raise ValueError("FluteExperts: %s is False, True or 'auto', not %r" % (name, value))


class FluteExperts(torch.nn.Module):
    """down(silu(gate(x)) * up(x)) over the experts each token was routed to, weighted and summed per token.
    `glu_blocks` (with `fused=True`): which kernel runs the fused GLU launch - False: `qgemm_grouped_glu`'s row form at every
    row count (the default, today's forward bit for bit); True: `qgemm_grouped_glu_blocks` (raises where the stacks are not
    eligible); "auto": the block launch where `flute_amd.dev.grouped_glu_blocks_form` takes it for the step's T k rows.
    `native_glu_grad` (with `fused=True`): the ops' keyword of that name - the backward of the fused GLU launch gathers its rows
    with `moe_gather` and forms dg, du with `swiglu_grad` (two HIP launches) where the default runs torch ops; the forward's bits
    are the same either way, the backward's differ within `flute_swiglu_grad`'s error account.
    `native_router_grad` (with `fused=True` and `native_routing=True`): the ops' keyword of that name - when the router trains,
    the weighted launch's backward forms d row_weight and d h in one `moe_weight_grad` launch, the gate-route launch's
    backward is one `moe_gate_grad` launch, and `moe_combine` gets `rows`, so its backward is one `moe_gather` launch; the
    default runs torch ops in all three places.  The forward's bits are the same either way.
    `wide_routing` (with `native_routing=True`): which routing launch runs - False: the one-workgroup `moe_route` /
    `moe_gate_route[_limited]` at every token count (the default, today's forward line for line); True: the multi-workgroup
    `moe_route_wide` / `moe_gate_route_wide`, three launches meant for prefill and training token counts; "auto": the wide form
    where `flute_amd.dev.moe_route_form` takes it for the step's shapes.  Outputs and every gradient are bit for bit the same."""

    def __init__(self, gate: GroupedFluteLinear, up: GroupedFluteLinear, down: GroupedFluteLinear,
                 fused: bool = False, native_routing: bool = False, glu_blocks: Union[bool, str] = False,
                 native_glu_grad: bool = False, native_router_grad: bool = False,
                 wide_routing: Union[bool, str] = False) -> None:
        super().__init__()
        _check_tristate("glu_blocks", glu_blocks)
        if glu_blocks is not False and not fused:
            raise ValueError("FluteExperts: glu_blocks selects the kernel of the fused GLU launch and needs fused=True")
        _check_tristate("wide_routing", wide_routing)
        if wide_routing is not False and not native_routing:
            raise ValueError("FluteExperts: wide_routing selects the kernels of the routing launch and needs native_routing=True")
        if native_router_grad and not (fused and native_routing):
            raise ValueError("FluteExperts: native_router_grad selects the backward of the weighted, gate-route and combine "
                             "launches and needs fused=True and native_routing=True")
        if native_glu_grad and not fused:
            raise ValueError("FluteExperts: native_glu_grad selects the backward of the fused GLU launch and needs fused=True")
        if not (gate.num_experts == up.num_experts == down.num_experts):
            raise ValueError("FluteExperts: gate, up and down differ in their number of experts")
        if (gate.in_features, gate.out_features) != (up.in_features, up.out_features) or \
                (down.in_features, down.out_features) != (gate.out_features, gate.in_features):
            raise ValueError("FluteExperts: gate / up must be [K -> F] and down [F -> K]")
        if fused and (gate.num_bits, gate.group_size, gate.template_id, gate.scales.dtype) != \
                (up.num_bits, up.group_size, up.template_id, up.scales.dtype):
            raise ValueError("FluteExperts: the fused forward needs gate and up of one num_bits / group_size / template_id / dtype")
        self.gate, self.up, self.down = gate, up, down
        self.num_experts = gate.num_experts
        self.fused = bool(fused)
        self.native_routing = bool(native_routing)
        self.glu_blocks = glu_blocks
        self.native_glu_grad = bool(native_glu_grad)
        self.native_router_grad = bool(native_router_grad)
        self.wide_routing = wide_routing

    @classmethod
    def from_linears(cls, gates: Sequence[FluteLinear], ups: Sequence[FluteLinear],
                     downs: Sequence[FluteLinear], fused: bool = False, native_routing: bool = False,
                     glu_blocks: Union[bool, str] = False, native_glu_grad: bool = False,
                     native_router_grad: bool = False, wide_routing: Union[bool, str] = False) -> "FluteExperts":
        return cls(GroupedFluteLinear.from_linears(gates), GroupedFluteLinear.from_linears(ups),
                   GroupedFluteLinear.from_linears(downs), fused=fused, native_routing=native_routing, glu_blocks=glu_blocks,
                   native_glu_grad=native_glu_grad, native_router_grad=native_router_grad, wide_routing=wide_routing)

    def forward(self, hidden: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor) -> torch.Tensor:
        if self.native_routing:
            return self._forward_native(hidden, topk_ids, topk_weights)
        k = topk_ids.shape[1]
        perm, offsets = sort_by_expert(topk_ids, self.num_experts)
        token = perm // k
        if self.fused:
            return self._forward_fused(hidden, topk_weights, perm, offsets, token)
        x = hidden[token]
        h = torch.nn.functional.silu(self.gate(x, offsets)) * self.up(x, offsets)
        y = self.down(h, offsets) * topk_weights.reshape(-1)[perm].to(hidden.dtype)[:, None]
        # rows past offsets[E] (ids outside [0, E)) were written by no expert: they contribute nothing
        served = torch.arange(y.shape[0], device=y.device) < offsets[-1]
        y = torch.where(served[:, None], y, torch.zeros_like(y))
        return torch.zeros_like(hidden).index_add_(0, token, y)

    def forward_logits(self, hidden: torch.Tensor, router_logits: torch.Tensor, top_k: int, scoring: str = "softmax",
                       renormalize: bool = False, bias=None, scale: float = 1.0) -> torch.Tensor:
        """The forward from the router's logits [T, E] (fp16 / bf16 / fp32); the gating is `flute_amd.moe_gate`'s contract
        (scoring "softmax" / "sigmoid", the optional selection `bias` [E] fp32, ties to the lower expert, `renormalize`,
        `scale`).  With `native_routing` gating and routing are one launch, `moe_gate_route`, and the forward is
        moe_gate_route -> glu -> weighted -> moe_combine (fused): four launches from logits.  Without it `moe_gate` feeds
        the existing forward.  Either way the result is bit for bit `forward(hidden, *moe_gate(...))`.  The choice is over
        all experts; group-limited selection (n_group, topk_group) is `forward_logits_limited`."""
        return self._forward_gated("forward_logits", hidden, router_logits, top_k, scoring, renormalize, bias, scale)

    def forward_logits_limited(self, hidden: torch.Tensor, router_logits: torch.Tensor, top_k: int, n_group: int,
                               topk_group: int, scoring: str = "softmax", renormalize: bool = False, bias=None,
                               scale: float = 1.0, group_score: str = "max") -> torch.Tensor:
        """`forward_logits` with DeepSeek's group-limited selection: the gating is `flute_amd.moe_gate_limited`'s contract
        (the `topk_group` best of `n_group` contiguous groups of experts by `group_score` "max" / "top2sum", then the top-k
        among their experts only).  With `native_routing` the forward is moe_gate_route_limited -> glu -> weighted ->
        moe_combine (fused): still four launches from logits.  Without it `moe_gate_limited` feeds the existing forward.
        Either way the result is bit for bit `forward(hidden, *moe_gate_limited(...))`."""
        return self._forward_gated("forward_logits_limited", hidden, router_logits, top_k, scoring, renormalize, bias, scale,
                                   (n_group, topk_group, group_score))

    def _gate_route(self, router_logits, top_k, scoring, renormalize, bias, scale, groups=None):
        """The gate-route launch, `groups` = (n_group, topk_group, group_score) or None: `moe_gate_route` /
        `moe_gate_route_limited`, or with `wide_routing` taken for these shapes `moe_gate_route_wide`, the one op of both gatings
        - looked up in `flute_amd` when it runs.  With the module's `native_router_grad` the same launch through the ops' shared
        entry, which carries the keyword to its backward."""
        wide = self._takes_wide_routing(router_logits.shape[0], top_k, gated=True)
        if wide and groups is None:
            groups = (1, 1, "max")                              # topk_group == n_group: the unlimited gating
        if self.native_router_grad:
            return flute_amd.ops._moe_gate_entry(router_logits, top_k, scoring, renormalize, bias, scale, routed=True,
                                                 num_experts=self.num_experts, groups=groups, native_router_grad=True,
                                                 wide=0 if wide else None)
        if wide:
            return flute_amd.moe_gate_route_wide(router_logits, top_k, self.num_experts, scoring, renormalize, bias, scale,
                                                 *groups)
        if groups is None:
            return flute_amd.moe_gate_route(router_logits, top_k, self.num_experts, scoring, renormalize, bias, scale)
        return flute_amd.moe_gate_route_limited(router_logits, top_k, groups[0], groups[1], self.num_experts, scoring,
                                                renormalize, bias, scale, groups[2])

    def _forward_gated(self, name, hidden, router_logits, top_k, scoring, renormalize, bias, scale, groups=None, want_ids=False):
        """The body of `forward_logits` (`groups` None) and `forward_logits_limited` (`groups` = (n_group, topk_group,
        group_score)): `moe_gate[_limited]` feeds the existing forward, with `native_routing` `_gate_route`'s routing arrays feed
        the launches behind them.  `want_ids` (`FluteSparseMoeBlock.aux_loss`): (the result, the gating's ids [T, k] int32)."""
        if router_logits.shape[1] != self.num_experts:
            raise ValueError("FluteExperts.%s: router_logits must be [T, num_experts]" % name)
        if self.native_routing:
            ids, _, offsets, rows, row_weight, pos, _ = self._gate_route(router_logits, top_k, scoring, renormalize, bias, scale,
                                                                         groups)
            out = self._forward_routed(hidden, offsets, rows, row_weight, pos)
        else:
            if groups is None:
                ids, weights = flute_amd.moe_gate(router_logits, top_k, scoring, renormalize, bias, scale)
            else:
                ids, weights = flute_amd.moe_gate_limited(router_logits, top_k, groups[0], groups[1], scoring, renormalize, bias,
                                                          scale, groups[2])
            out = self.forward(hidden, ids, weights)
        return (out, ids) if want_ids else out

    def _forward_fused(self, hidden, topk_weights, perm, offsets, token):
        """`_fused_mlp` on torch's routing: no silu, no where, no gathered copy of `hidden`."""
        y = self._fused_mlp(hidden, offsets, token.to(torch.int32), topk_weights.reshape(-1)[perm].float())
        return torch.zeros_like(hidden).index_add_(0, token, y)

    def _fused_mlp(self, hidden, offsets, rows, row_weight, pos=None):
        """Two launches (qgemm_grouped.h, GLU and weighted modes): silu(gate(x)) * up(x) with the rows of `hidden` read through the
        routing index `rows`, then the down projection with the routing weight (fp32) in its epilogue, which also writes
        the rows past offsets[E] (ids outside [0, E)) as zeros.  `pos` is read by the GLU launch's backward only."""
        gate, up, down = self.gate, self.up, self.down
        num_sms = _stack_num_sms(gate, hidden.device)
        glu, weighted = self._fused_ops(self._takes_glu_blocks(hidden, rows.shape[0], num_sms))
        h = glu(hidden, offsets, gate.weight, gate.scales, _table_of(gate), up.weight, up.scales, _table_of(up),
                gate.num_bits, gate.group_size, gate.template_id, num_sms, rows=rows, pos=pos)
        return weighted(h, offsets, down.weight, down.scales, _table_of(down), row_weight, down.num_bits, down.group_size,
                        down.template_id, num_sms)

    def _takes_wide_routing(self, tokens: int, top_k: int, gated: bool) -> bool:
        """Whether this step's routing is the multi-workgroup one: `wide_routing`, "auto" resolved from the shapes alone."""
        if self.wide_routing != "auto":
            return self.wide_routing
        return flute_amd.dev.moe_route_form(tokens, top_k, self.num_experts, gated=gated) == "wide"

    def _takes_glu_blocks(self, hidden, rows: int, num_sms: int) -> bool:
        """Whether this step's fused GLU launch is the block one: `glu_blocks`, "auto" resolved from the shapes alone."""
        if self.glu_blocks != "auto":
            return self.glu_blocks
        gate = self.gate
        return flute_amd.dev.grouped_glu_blocks_form(self.num_experts, rows, hidden.shape[0], gate.out_features,
                                                     gate.in_features, gate.num_bits, gate.group_size, gate.template_id,
                                                     num_sms, hidden.dtype) == "blocks"

    def _fused_ops(self, glu_blocks: bool = False):
        """The two fused launches: the public ops, or - when a stack is learnable - the entry points that also give the
        scales their gradient, or - when it has a codebook - those that take `_table_of(stack)`, the codebook, in
        `tables2`'s place and give it its gradient too (with grad mode off all of them are the public ops).
        `glu_blocks`: the GLU launch on its block form (`qgemm_grouped_glu_blocks`, the learnable entries' `blocks=True`).
        The module's `native_glu_grad` rides on whichever GLU entry that is, its `native_router_grad` on the weighted one."""
        gate, up, down = self.gate, self.up, self.down
        has = [_has_codebook(m) for m in (gate, up, down)]
        if has[0] != has[1]:
            raise ValueError("FluteExperts: the fused forward needs gate and up both with or both without a codebook")
        learnable = any(isinstance(m, LearnableGroupedFluteLinear) for m in (gate, up, down))
        glu = qgemm_grouped_glu_learnable if has[0] else \
            qgemm_grouped_glu_learnable_scales if learnable else flute_amd.qgemm_grouped_glu
        if glu_blocks:
            glu = flute_amd.qgemm_grouped_glu_blocks if glu is flute_amd.qgemm_grouped_glu else functools.partial(glu, blocks=True)
        if self.native_glu_grad:
            glu = functools.partial(glu, native_glu_grad=True)
        weighted = qgemm_grouped_weighted_learnable if has[2] else \
            qgemm_grouped_weighted_learnable_scales if learnable else flute_amd.qgemm_grouped_weighted
        if self.native_router_grad:
            weighted = functools.partial(weighted, native_router_grad=True)
        return glu, weighted

    def _forward_native(self, hidden, topk_ids, topk_weights):
        """`moe_route` (moe_route.hip) in place of sort_by_expert and its glue, `moe_combine` (moe_combine.hip) in place
        of zeros_like + index_add_: the sum over a token's experts is taken in fp32 in slot order and rounded once, and
        rows no expert served are never read.  Fused: four launches, nothing else."""
        route = flute_amd.moe_route_wide if self._takes_wide_routing(*topk_ids.shape, gated=False) else flute_amd.moe_route
        offsets, rows, row_weight, pos, _ = route(topk_ids, topk_weights, self.num_experts)
        return self._forward_routed(hidden, offsets, rows, row_weight, pos)

    def _forward_routed(self, hidden, offsets, rows, row_weight, pos):
        """The launches behind the routing arrays, whichever kernel wrote them (`moe_route`, `moe_gate_route[_limited]`, their `_wide` forms)."""
        if self.fused:
            y = self._fused_mlp(hidden, offsets, rows, row_weight, pos)
        else:
            x = hidden[rows]
            h = torch.nn.functional.silu(self.gate(x, offsets)) * self.up(x, offsets)
            y = self.down(h, offsets) * row_weight.to(hidden.dtype)[:, None]
        return flute_amd.moe_combine(y, pos, offsets, rows if self.native_router_grad else None)


MoeAuxLosses = collections.namedtuple("MoeAuxLosses", ("balance", "z", "load", "importance"))     # FluteSparseMoeBlock.aux


class FluteSparseMoeBlock(torch.nn.Module):
    """A whole sparse-MoE block: router, gating, experts.  forward(hidden [T, K]) is
    `experts.forward_logits(F.linear(hidden, router_weight), top_k, ...)`, bit for bit.  `router_weight` [E, K] is the
    router's dense matrix; its GEMM stays a dense torch op (E is 8 .. 256 columns: nothing to quantise or fuse), and
    everything behind it is the module's own kernels - with `FluteExperts(fused=True, native_routing=True)` four
    launches; the experts' `glu_blocks` is honoured as they were built (the block calls their `forward_logits[_limited]`).
    `scoring`, `renormalize`, `bias` (the selection bias [E] fp32, kept as a buffer) and `scale` are
    `flute_amd.moe_gate`'s.  With `n_group` > 1 the selection is DeepSeek's group-limited one (`flute_amd.moe_gate_limited`:
    the `topk_group` best of `n_group` groups of experts by `group_score` "max" / "top2sum") and forward is
    `experts.forward_logits_limited(...)`, the same number of launches; with n_group == 1 it is exactly the path above.
    `block.aux_loss = True` (a validated attribute, False by default; the constructor's parameters are as they were): forward
    also calls `flute_amd.moe_aux_loss` on the logits it computed, with the ids its gating launch
    picked and the block's own scoring, and leaves `block.aux = MoeAuxLosses(balance, z, load, importance)`: balance (the
    load-balance loss; DeepSeek's is balance / top_k) and z (the router z-loss) are attached to the graph, so
    `(loss + a * block.aux.balance + b * block.aux.z).backward()` reaches `router_weight` and `hidden` through torch's own
    `F.linear`; load [E] int32 is what an aux-loss-free bias update reads (the rule itself is not part of this module).  The
    block's output is bit for bit the one with `aux_loss` off.  Keep the router in fp32 or bf16 where the losses train: in fp16
    their gradients, of order E / T^2, fall into the subnormal range.  Token masks and per-sequence losses are out of scope.
    `block.aux` holds the autograd graph of the forward that wrote it, as a kept loss tensor does, until the next forward
    replaces it: use it in that step's loss (or `del block.aux`) before a later step runs on another stream, a graph capture
    for one.  With the default the forward is unchanged and the block has no `aux` attribute."""

    def __init__(self, router_weight: torch.Tensor, experts: FluteExperts, top_k: int, scoring: str = "softmax",
                 renormalize: bool = False, bias=None, scale: float = 1.0, n_group: int = 1, topk_group: int = 1,
                 group_score: str = "max") -> None:
        super().__init__()
        if router_weight.ndim != 2 or router_weight.shape[0] != experts.num_experts or \
                router_weight.shape[1] != experts.gate.in_features:
            raise ValueError("FluteSparseMoeBlock: router_weight must be [num_experts, in_features]")
        if scoring not in ("softmax", "sigmoid"):
            raise ValueError("FluteSparseMoeBlock: scoring is 'softmax' or 'sigmoid'")
        if not 1 <= top_k <= min(experts.num_experts, flute_amd.ops.MOE_GATE_MAX_TOPK):
            raise ValueError("FluteSparseMoeBlock: 1 <= top_k <= min(num_experts, 64)")
        if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (experts.num_experts,)):
            raise ValueError("FluteSparseMoeBlock: bias must be [num_experts] fp32")
        if group_score not in ("max", "top2sum"):
            raise ValueError("FluteSparseMoeBlock: group_score is 'max' or 'top2sum'")
        if not 1 <= n_group <= flute_amd.ops.MOE_GATE_MAX_GROUPS or experts.num_experts % n_group != 0:
            raise ValueError("FluteSparseMoeBlock: 1 <= n_group <= 64 must divide num_experts")
        if not 1 <= topk_group <= n_group:
            raise ValueError("FluteSparseMoeBlock: 1 <= topk_group <= n_group")
        group_size = experts.num_experts // n_group
        if top_k > topk_group * group_size:
            raise ValueError("FluteSparseMoeBlock: top_k <= topk_group * (num_experts / n_group)")
        if n_group > 1 and group_score == "top2sum" and group_size < 2:
            raise ValueError("FluteSparseMoeBlock: group_score 'top2sum' needs groups of two experts or more")
        self.experts = experts
        self.register_buffer("router_weight", router_weight)
        self.register_buffer("bias", bias)
        self.top_k, self.scoring, self.renormalize, self.scale = int(top_k), scoring, bool(renormalize), float(scale)
        self.n_group, self.topk_group, self.group_score = int(n_group), int(topk_group), group_score

    _aux_loss = False

    @property
    def aux_loss(self) -> bool:
        """Whether forward also computes the router's auxiliary losses into `self.aux` (the class docstring); False unless set."""
        return self._aux_loss

    @aux_loss.setter
    def aux_loss(self, value: bool) -> None:
        if not isinstance(value, bool):
            raise TypeError("FluteSparseMoeBlock: aux_loss is a bool")
        self._aux_loss = value

    def forward(self, hidden: torch.Tensor) -> torch.Tensor:
        logits = torch.nn.functional.linear(hidden, self.router_weight)
        if self.aux_loss:
            return self._forward_aux(hidden, logits)
        if self.n_group > 1:
            return self.experts.forward_logits_limited(hidden, logits, self.top_k, self.n_group, self.topk_group,
                                                       self.scoring, self.renormalize, self.bias, self.scale,
                                                       self.group_score)
        return self.experts.forward_logits(hidden, logits, self.top_k, self.scoring, self.renormalize, self.bias,
                                           self.scale)

    def _forward_aux(self, hidden, logits):
        """The forward with `aux_loss`: the same launches, the gating's ids kept, and `moe_aux_loss` on them into `self.aux`."""
        limited = self.n_group > 1
        out, ids = self.experts._forward_gated(
            "forward_logits_limited" if limited else "forward_logits", hidden, logits, self.top_k, self.scoring, self.renormalize,
            self.bias, self.scale, (self.n_group, self.topk_group, self.group_score) if limited else None, want_ids=True)
        self.aux = MoeAuxLosses(*flute_amd.moe_aux_loss(logits, ids, self.scoring))
        return out

    def extra_repr(self) -> str:
        return (f"top_k={self.top_k}, scoring={self.scoring}, renormalize={self.renormalize}, scale={self.scale}, "
                f"bias={self.bias is not None}, n_group={self.n_group}, topk_group={self.topk_group}, "
                f"group_score={self.group_score}" + (", aux_loss=True" if self.aux_loss else ""))
