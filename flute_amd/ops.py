"""torch operator surface: `flute::qgemm_raw_simple[_hadamard]` and `flute_amd::dequantize`,
plus plain functions over the C ABI: `hadamard_transform`, `qgemm_scale_grad`, `qgemm_table_grad`, `qgemm_grouped`, `qgemm_grouped_glu`,
`qgemm_grouped_weighted`, `qgemm_grouped_input_grad`, `qgemm_grouped_scale_grad`, `qgemm_grouped_table_grad`, `moe_route`, `moe_combine`, `moe_gather`, `swiglu_grad`, `moe_weight_grad`, `moe_gate_grad`, `moe_gate`, `moe_gate_route`, `moe_gate_limited`,
`moe_gate_route_limited`, `moe_aux_loss` and `moe_aux_loss_grad`.  The grouped and mixture-of-experts functions are differentiable with respect to their activations,
routing weights and router logits: when grad mode is on and such an input requires grad they run through a
`torch.autograd.Function` whose forward is the same launch and whose backward is `qgemm_grouped_input_grad`, `moe_combine`
and a few torch ops; otherwise they take exactly the path they always took.  Each of the three grouped ops has ONE such
function, which also carries the gradients of the stacks' scales (`qgemm_grouped_scale_grad`) and of their fp32 master
codebooks (`qgemm_grouped_table_grad`): the ops themselves refuse packed stacks that require grad, `integrations.learnable`
opens those slots.  Every validator of a packed layer or stack is
three calls into one set of checks (`_check_ranks`, `_check_dtypes`, `_check_packed`); the validators of the routing,
row-stream and router-gradient ops open with the first two and keep by hand only the checks whose order of exception classes
those three phases cannot express.  Every grouped launch - forward, input gradient, scale gradient - ends in `_launch_grouped`,
and every other call into the C ABI - the Hadamard transform, the dense and grouped parameter gradients, routing, gating,
combine, gather and the router's gradients - ends in `_abi_call`: the same-GPU check (`_same_gpu`, the one place that words
it), `_abi_tensor` on the inputs only, the device guard, the stream, the return code.  The five routing arrays and the wide
launches' workspace are allocated in `_routing_arrays`, for `moe_route[_wide]` and the gating ops alike.

Schemas are the reference's, verbatim (flute/csrc/qgemm.cpp:251-254); the
implementation is registered for the `CUDA` dispatch key (HIP tensors use it on
PyTorch-ROCm, as qgemm.cpp:257-260 does for CUDA) by a compiled C++ binding and
forwards to the C ABI.  The fake (meta) implementations restate flute/ops.py:4-83
so that torch.compile / opcheck see the same validation.  No CPU kernel is registered.

The binding also registers Autograd kernels for both `flute::` ops (input gradient
only: dX = dY @ dequantize(...), computed in bounded K chunks) and this project's
own `flute_amd::dequantize` (the dense [N, K] weight, a native HIP kernel).
"""
import os

import torch

from . import _lib

# The operators are DEFINED and IMPLEMENTED (dispatch key CUDA) by the compiled binding
# flute_amd/csrc/torch_binding.cpp (TORCH_LIBRARY(flute) - the role of flute/csrc/qgemm.cpp:246-260):
# validation, flatten, at::empty, device guard, current stream and ONE call into the C ABI, all in C++.
# This module loads it, fails loudly when it has not been built, and adds the fake (meta) implementations.
TORCH_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libflute_amd_torch.so")
_lib.get()                      # libflute_amd.so first: the binding links against it
if not os.path.exists(TORCH_LIB_PATH):
    raise ImportError(
        f"flute_amd: torch binding not built: {TORCH_LIB_PATH} is missing. Run "
        f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C {os.path.dirname(TORCH_LIB_PATH)} -j`. "
        f"There is no Python fallback for the operators.")
torch.ops.load_library(TORCH_LIB_PATH)

_DTYPE_ID = {torch.float16: 0, torch.bfloat16: 1}


def _validate(input, weight, scales, table, table2, workspace, num_bits, group_size):
    # flute/ops.py:17-49 (the reference validates only in the fake impl; the
    # real one trusts raw pointers, qgemm.cpp:71-77 - we check in both)
    if not all([input.ndim >= 2, weight.ndim == 2, scales.ndim == 2, table.ndim == 1,
                table2.ndim == 3, workspace.ndim == 1]):
        raise ValueError
    dtype = input.dtype
    if dtype not in _DTYPE_ID:
        raise TypeError
    if not all([weight.dtype == torch.int16, scales.dtype == dtype, table.dtype == dtype,
                table2.dtype == torch.float32, workspace.dtype == torch.uint8]):
        raise TypeError
    if not all([
        weight.shape[1] == input.shape[-1],
        weight.shape[1] == scales.shape[1] * group_size,
        weight.shape[0] == int(num_bits * (scales.shape[0] / 16)),
        table.shape[0] == 2 ** num_bits,
        table2.shape[0] == 2 ** num_bits,
        table2.shape[1] == 2 ** num_bits,
        table2.shape[2] == 1,
    ]):
        raise ValueError


def _stream_ptr(device):
    """The current stream of `device` (a `torch.device` or its index) as the C ABI takes it."""
    return torch.cuda.current_stream(device).cuda_stream


def _abi_tensor(t):
    """`t` as the C ABI takes it (include/flute_amd.h: contiguous, 16-B aligned): `t` itself when it already is - no
    allocation, no torch op - otherwise a fresh contiguous copy, which the allocator aligns.  A contiguous view such as
    buf[1:1 + n] is not aligned, and the kernels address their operands with 16-B loads and buffer descriptors."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _num_sms(num_sms, device):
    """`num_sms` as the C ABI takes it: the caller's, or with None the device's CU count."""
    return torch.cuda.get_device_properties(device).multi_processor_count if num_sms is None else num_sms


def _same_gpu(name, tensors):
    """The one GPU that `tensors` (None: absent) live on - the first one's - or RuntimeError in op `name`'s name."""
    dev = tensors[0].device
    for t in tensors:
        if t is not None and not (t.is_cuda and t.device == dev):
            raise RuntimeError(f"flute_amd.{name}: all tensors must live on the same GPU")
    return dev


def _abi_call(name, fn, head, inputs, outputs, tail=(), dev=None):
    """The tail of every validated op that is not a grouped launch: fn(*head, *pointers of `inputs`, *pointers of `outputs`,
    *tail, stream) on the inputs' GPU, the return code checked.  `inputs` (None: a null pointer) are checked to share one GPU
    (`_same_gpu`, in op `name`'s name; `dev`: the caller has asked already, before it allocated or because it may return
    before it launches) and go through `_abi_tensor`, the copies alive across the call.  `outputs` - results and scratch the
    caller allocated, None: a null pointer - are handed on as they are: a copy of one would lose the result, so nothing here
    ever copies them.  One pass, one argument list; the guard and the stream are asked by device index, which spares torch
    resolving a `torch.device` twice per call."""
    if dev is None:
        dev = _same_gpu(name, inputs)
    args, kept = [*head], []
    for t in inputs:
        if t is not None:
            t = _abi_tensor(t)
            kept.append(t)
            t = t.data_ptr()
        args.append(t)
    for t in outputs:
        args.append(t if t is None else t.data_ptr())
    index = dev.index
    with torch.cuda.device(index):
        _lib.check(fn(*args, *tail, _stream_ptr(index)))


def hadamard_transform(input: torch.Tensor, hadamard_size: int) -> torch.Tensor:
    """apply_hadamard (qgemm.cpp:201-211): out-of-place FWHT over
    input.reshape(-1, hadamard_size), orthonormal."""
    if input.dtype not in _DTYPE_ID:
        raise TypeError("Only fp16 and bf16 supported currently")
    if not input.is_cuda:
        raise RuntimeError("flute_amd.hadamard_transform: tensor must live on the GPU")
    if input.shape[-1] % hadamard_size and input.numel() % hadamard_size:
        raise RuntimeError(f"shape {tuple(input.shape)} is invalid for hadamard_size {hadamard_size}")
    out = torch.empty(input.shape, dtype=input.dtype, device=input.device)
    _abi_call("hadamard_transform", _lib.get().flute_hadamard, (_DTYPE_ID[input.dtype],), (input,), (out,),
              (input.numel(), hadamard_size))
    return out


@torch.library.register_fake("flute::qgemm_raw_simple")
def _qgemm_raw_simple_abstract(input, weight, scales, table, table2, workspace, num_bits,
                               group_size, template_id, num_sms):
    _validate(input, weight, scales, table, table2, workspace, num_bits, group_size)
    N = scales.shape[0]
    return torch.empty(input.shape[:-1] + (N,), dtype=input.dtype, device=input.device)


@torch.library.register_fake("flute::qgemm_raw_simple_hadamard")
def _qgemm_raw_simple_hadamard_abstract(input, weight, scales, table, table2, workspace,
                                        num_bits, group_size, hadamard_size, template_id,
                                        num_sms):
    return _qgemm_raw_simple_abstract(input, weight, scales, table, table2, workspace,
                                      num_bits, group_size, template_id, num_sms)


# ---- what every validator of a packed layer or stack checks, in three phases that each raise one class: ranks
# (ValueError), then dtypes (TypeError), then values and shapes (ValueError)

def _check_ranks(*tensor_ndim):
    """(tensor, ndim) pairs; "at least 2" is (t, max(t.ndim, 2))."""
    for t, ndim in tensor_ndim:
        if t.ndim != ndim:
            raise ValueError


def _check_dtypes(dtype, like=(), int16=(), fp32=(), int32=(), allowed=_DTYPE_ID):
    """`dtype` - the activations' - is fp16 or bf16 (one of `allowed`), the `like` tensors have it and the others their fixed
    type."""
    if dtype not in allowed:
        raise TypeError
    for ts, want in ((like, dtype), (int16, torch.int16), (fp32, torch.float32), (int32, torch.int32)):
        for t in ts:
            if t.dtype != want:
                raise TypeError


def _pair_table_shape(num_bits, lead=()):
    return lead + (2 ** num_bits, 2 ** num_bits, 1)


def _check_packed(weight, num_bits, group_size, N, K, lead=(), table2=None, offsets=None, n_multiple=16):
    """The values of a packed layer - or with lead = (E,) a stack of E - of N outputs and K inputs: num_bits and
    group_size legal, K % max(64, g) == 0, N % n_multiple == 0, `weight` lead + [num_bits N / 16, K], and where given
    `table2` lead + [2^b, 2^b, 1] and `offsets` of E + 1."""
    if num_bits not in (2, 3, 4) or group_size not in (32, 64, 128, 256):
        raise ValueError
    if not all([
        K > 0 and K % max(64, group_size) == 0,
        N > 0 and N % n_multiple == 0,
        tuple(weight.shape) == lead + (num_bits * (N // 16), K),
        table2 is None or tuple(table2.shape) == _pair_table_shape(num_bits, lead),
        offsets is None or offsets.shape[0] == lead[0] + 1,
    ]):
        raise ValueError


def _check_row_weight(row_weight, R):
    """`row_weight` [R] fp32."""
    if row_weight.dtype != torch.float32:
        raise TypeError
    if row_weight.ndim != 1 or row_weight.shape[0] != R:
        raise ValueError


def _validate_dequantize(weight, scales, table2, num_bits, group_size):
    _check_ranks((weight, 2), (scales, 2), (table2, 3))
    _check_dtypes(scales.dtype, int16=(weight,), fp32=(table2,))
    # (the reference's relations, flute/ops.py:40-49: which num_bits and group_size are legal is the C ABI's to say)
    if not all([
        weight.shape[1] == scales.shape[1] * group_size,
        weight.shape[0] == int(num_bits * (scales.shape[0] / 16)),
        tuple(table2.shape) == _pair_table_shape(num_bits),
    ]):
        raise ValueError


@torch.library.register_fake("flute_amd::dequantize")
def _dequantize_abstract(weight, scales, table2, num_bits, group_size, template_id):
    _validate_dequantize(weight, scales, table2, num_bits, group_size)
    return torch.empty((scales.shape[0], weight.shape[1]), dtype=scales.dtype, device=scales.device)


def _validate_scale_grad(grad_output, input, weight, table2, num_bits, group_size):
    _check_ranks((input, max(input.ndim, 2)), (grad_output, input.ndim), (weight, 2), (table2, 3))
    _check_dtypes(input.dtype, like=(grad_output,), int16=(weight,), fp32=(table2,))
    _check_packed(weight, num_bits, group_size, grad_output.shape[-1], input.shape[-1], table2=table2)
    if grad_output.shape[:-1] != input.shape[:-1]:
        raise ValueError


def _scale_grad_scratch_bytes(N, K, group_size, num_sms):
    # the most the launch can split M into (param_grad.hip: 256 x 128 blocks of (k, n), two workgroups per CU)
    blocks = (N // 128) * -(-K // 256)
    target = 2 * (num_sms if num_sms >= 1 else 256)
    if blocks == 0 or blocks >= target:
        return 0
    return -(-target // blocks) * N * (K // group_size) * 4


def qgemm_scale_grad(grad_output: torch.Tensor, input: torch.Tensor, weight: torch.Tensor,
                     table2: torch.Tensor, num_bits: int, group_size: int, template_id: int,
                     num_sms=None) -> torch.Tensor:
    """Gradient of the scales of `Y = qgemm(input, weight, scales, ...)` for the upstream gradient `grad_output`:
    dS[n, j] = round_T(sum_m sum_{k in group j} dY[m, n] * X[m, k] * L[k, n]), L the table2 pair lookup of the
    packed codes (what the forward multiplies by the scale).  Leading dimensions are flattened; returns [N, K / g]
    in input.dtype.  For a Hadamard layer pass the rotated input, `hadamard_transform(input, hadamard_size)`.
    A native HIP kernel on the current stream (param_grad.hip); the same arguments give the same bits."""
    _validate_scale_grad(grad_output, input, weight, table2, num_bits, group_size)
    dev = _same_gpu("qgemm_scale_grad", (input, grad_output, weight, table2))
    K, N = input.shape[-1], grad_output.shape[-1]
    x, dy = input.reshape(-1, K), grad_output.reshape(-1, N)
    M = x.shape[0]
    if M >= 2 ** 31:
        raise ValueError
    out = torch.empty((N, K // group_size), dtype=input.dtype, device=dev)
    if M == 0:
        return out.zero_()
    num_sms = _num_sms(num_sms, dev)
    nbytes = _scale_grad_scratch_bytes(N, K, group_size, num_sms)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _abi_call("qgemm_scale_grad", _lib.get().flute_qgemm_scale_grad,
              (_DTYPE_ID[x.dtype], num_bits, group_size, M, N, K, weight.shape[0], template_id),
              (dy, x, weight, table2), (out, scratch if nbytes else None), (nbytes, num_sms), dev)
    return out


def _validate_table_grad(grad_output, input, weight, scales, table2, num_bits, group_size, with_scale_grad):
    _check_ranks((input, max(input.ndim, 2)), (grad_output, input.ndim), (weight, 2), (scales, 2))
    _check_dtypes(input.dtype, like=(grad_output, scales), int16=(weight,))
    K, N = input.shape[-1], grad_output.shape[-1]
    _check_packed(weight, num_bits, group_size, N, K)
    if grad_output.shape[:-1] != input.shape[:-1] or tuple(scales.shape) != (N, K // group_size):
        raise ValueError
    if with_scale_grad and table2 is None:
        raise ValueError("qgemm_table_grad: with_scale_grad needs table2 (the scale gradient reads the table)")
    if table2 is not None:
        if table2.ndim != 3:
            raise ValueError
        if table2.dtype != torch.float32:
            raise TypeError
        if tuple(table2.shape) != _pair_table_shape(num_bits):
            raise ValueError


def qgemm_table_grad(grad_output: torch.Tensor, input: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor,
                     num_bits: int, group_size: int, template_id: int, num_sms=None, *, table2=None,
                     with_scale_grad: bool = False):
    """Gradient of the pair codebook of `Y = qgemm(input, weight, scales, ...)` with the codes fixed, for the upstream
    gradient `grad_output`: dT2[i, j, e] = sum over the pairs (kappa, n) with codes (i, j) at rows (2 kappa,
    2 kappa + 1) of sum_m dY[m, n] * X[m, 2 kappa + e] * S[n, 2 kappa / g], as [2^b, 2^b, 2] fp32 (element e of
    entry (i, j) of `table2` seen as pairs of T).  `pair_grad_to_table_grad` folds it for a scalar table.  The table
    itself is not read.  With `with_scale_grad` (needs `table2`) the same launch also computes the scale gradient
    and (dT2, dS) is returned, dS bit for bit `qgemm_scale_grad`'s.  Leading dimensions are flattened; for a
    Hadamard layer pass the rotated input.  Native HIP kernels on the current stream (param_grad.hip); the same
    arguments give the same bits."""
    _validate_table_grad(grad_output, input, weight, scales, table2, num_bits, group_size, with_scale_grad)
    dev = _same_gpu("qgemm_table_grad", (input, grad_output, weight, scales, table2))
    K, N = input.shape[-1], grad_output.shape[-1]
    x, dy = input.reshape(-1, K), grad_output.reshape(-1, N)
    M = x.shape[0]
    if M >= 2 ** 31:
        raise ValueError
    n = 2 ** num_bits
    dT2 = torch.empty((n, n, 2), dtype=torch.float32, device=dev)
    dS = torch.empty((N, K // group_size), dtype=input.dtype, device=dev) if with_scale_grad else None
    if M == 0:
        dT2.zero_()
        return (dT2, dS.zero_()) if with_scale_grad else dT2
    num_sms = _num_sms(num_sms, dev)
    lib = _lib.get()
    nbytes = lib.flute_qgemm_table_grad_scratch_bytes(num_bits, group_size, M, N, K, int(with_scale_grad), num_sms)
    if nbytes == 0:
        raise ValueError(f"flute_amd.qgemm_table_grad: no kernel for N = {N}, K = {K}, group size {group_size}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _abi_call("qgemm_table_grad", lib.flute_qgemm_table_grad,
              (_DTYPE_ID[x.dtype], num_bits, group_size, M, N, K, weight.shape[0], template_id),
              (dy, x, weight, scales, table2 if with_scale_grad else None), (dT2, dS, scratch), (nbytes, num_sms), dev)
    return (dT2, dS) if with_scale_grad else dT2


def pair_grad_to_table_grad(dT2: torch.Tensor) -> torch.Tensor:
    """The adjoint of `utils.make_qmap2_from_qmap` (table2[i, j] = (table[i], table[j])): the gradient [2^b] of a
    scalar table from the pair-codebook gradient [2^b, 2^b, 2], dtable[i] = sum_j dT2[i, j, 0] + sum_j dT2[j, i, 1]."""
    if dT2.ndim != 3 or dT2.shape[0] != dT2.shape[1] or dT2.shape[2] != 2:
        raise ValueError
    return dT2[:, :, 0].sum(dim=1) + dT2[:, :, 1].sum(dim=0)


def grouped_pair_grad_to_table_grad(dT2: torch.Tensor) -> torch.Tensor:
    """`pair_grad_to_table_grad` per expert: the gradients [E, 2^b] of E scalar tables from `qgemm_grouped_table_grad`'s
    [E, 2^b, 2^b, 2], dtable[e, i] = sum_j dT2[e, i, j, 0] + sum_j dT2[e, j, i, 1]."""
    if dT2.ndim != 4 or dT2.shape[1] != dT2.shape[2] or dT2.shape[3] != 2:
        raise ValueError
    return dT2[..., 0].sum(-1) + dT2[..., 1].sum(-2)


def _grouped_codebook_table2(codebook, num_bits, dtype):
    """`table2` [E, 2^b, 2^b, 1] fp32 words of T pairs from a stack's fp32 master codebook rounded to T, in a number of
    torch ops that does not depend on E: [E, 2^b] scalar tables give torch.stack([make_qmap2_from_qmap(t_e)]) bit for bit,
    [E, 2^b, 2^b, 2] pair codebooks the rounded pairs viewed as words."""
    n = 2 ** num_bits
    if codebook.dtype != torch.float32:
        raise TypeError("the codebook is an fp32 master parameter")
    if codebook.ndim == 2 and codebook.shape[1] == n:
        table = codebook.detach().to(dtype)
        E = table.shape[0]
        pairs = torch.stack([table[:, :, None].expand(E, n, n), table[:, None, :].expand(E, n, n)], dim=-1)
    elif codebook.ndim == 4 and tuple(codebook.shape[1:]) == (n, n, 2):
        pairs = codebook.detach().to(dtype)
    else:
        raise ValueError(f"codebook of shape {tuple(codebook.shape)}, expected (E, {n}) or (E, {n}, {n}, 2)")
    return pairs.contiguous().view(torch.float32)


def _grouped_table_grads(grad_output, input, offsets, weight, scales, table2, layer, want_scales, want_codebook, scalar,
                         row_weight=None):
    """(d scales, d codebook) of one stack in a grouped backward: one `qgemm_grouped_table_grad` launch when the codebook
    trains - with the scale gradient in it when the scales train too - else today's `qgemm_grouped_scale_grad`; the scalar
    form folds per expert.  The gradient passes straight through the codebook's rounding."""
    if not want_codebook:
        d_scales = qgemm_grouped_scale_grad(grad_output, input, offsets, weight, table2, *layer, row_weight=row_weight) \
            if want_scales else None
        return d_scales, None
    out = qgemm_grouped_table_grad(grad_output, input, offsets, weight, scales.detach(), *layer, table2=table2,
                                   with_scale_grad=want_scales, row_weight=row_weight)
    d_codebook, d_scales = out if want_scales else (out, None)
    return d_scales, grouped_pair_grad_to_table_grad(d_codebook) if scalar else d_codebook


def _records_grad(*tensors):
    """Whether a call on these inputs must record a graph: grad mode is on and a floating-point one requires grad."""
    return torch.is_grad_enabled() and any(t is not None and t.is_floating_point() and t.requires_grad for t in tensors)


def _refuse_stack_grads(name, *tensors):
    if any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(
            f"flute_amd.{name}: gradients with respect to scales, table or table2 are not supported "
            "(only the input gradient is); detach them or set requires_grad=False")


def _zero_unserved_(out, offsets):
    """Rows from offsets[E] on - rows no expert serves, which the launch left unwritten - as zeros, on the device: under
    autograd an unwritten row must not hold a NaN that a zero gradient could meet."""
    R = out.shape[0]
    unserved = torch.arange(R, device=out.device) >= offsets[-1].clamp(0, R)
    return out.masked_fill_(unserved[:, None], 0)


def _validate_grouped(input, offsets, weight, scales, table2, num_bits, group_size):
    _check_ranks((input, 2), (offsets, 1), (weight, 3), (scales, 3), (table2, 4))
    _check_dtypes(input.dtype, like=(scales,), int16=(weight,), fp32=(table2,), int32=(offsets,))
    E, N, K = scales.shape[0], scales.shape[1], input.shape[1]
    _check_packed(weight, num_bits, group_size, N, K, lead=(E,), table2=table2, offsets=offsets)
    if scales.shape[2] * group_size != K:
        raise ValueError


# the `form` of the three grouped forward ops -> flute_grouped_form_t
_GROUPED_FORMS = {None: 0, "rows": 1, "blocks": 2}
# the `form` of `qgemm_grouped_input_grad` -> flute_grouped_input_grad_form_t
_GROUPED_INPUT_GRAD_FORMS = {None: 0, "slabs": 1, "blocks": 2}


def _grouped_form_id(form):
    if form not in _GROUPED_FORMS:
        raise ValueError(f"form must be None, 'rows' or 'blocks', not {form!r}")
    return _GROUPED_FORMS[form]


def _grouped_input_grad_form_id(form):
    if form not in _GROUPED_INPUT_GRAD_FORMS:
        raise ValueError(f"form must be None, 'slabs' or 'blocks', not {form!r}")
    return _GROUPED_INPUT_GRAD_FORMS[form]


def _launch_grouped(name, tensors, weight, rows, N, out_shape, layer, row_limit=2 ** 31, form=(), form_id=_grouped_form_id):
    """The tail of every validated grouped op: flute_<name>(dtype, num_bits, group_size, E, *rows, N, K, P, template_id,
    *pointers, out, num_sms, stream) with `tensors` as the pointers in the ABI's order (None: a null pointer; the first
    gives the result's type and device), `rows` the ABI's row counts, each below `row_limit`, `weight` [E, P, K] one of
    the stacks and `layer` = (num_bits, group_size, template_id, num_sms).  `form` (the three forward ops, whose `name` is
    the `_ex` entry's): (None | "rows" | "blocks",), the ABI's trailing argument, mapped by `form_id` (the input gradient's
    `_ex` entry: its own names).  Returns the result, `out_shape`."""
    form = tuple(form_id(f) for f in form)
    num_bits, group_size, template_id, num_sms = layer
    first = tensors[0]
    dev = _same_gpu(name, tensors)
    if max(rows) >= row_limit:
        raise ValueError
    ptrs = [None if t is None else _abi_tensor(t) for t in tensors]
    out = torch.empty(out_shape, dtype=first.dtype, device=dev)
    num_sms = _num_sms(num_sms, dev)
    E, P, K = weight.shape
    index = dev.index                                           # (as `_abi_call`: torch resolves a `torch.device` slowly)
    with torch.cuda.device(index):
        _lib.check(getattr(_lib.get(), "flute_" + name)(
            _DTYPE_ID[first.dtype], num_bits, group_size, E, *rows, N, K, P, template_id,
            *[None if t is None else t.data_ptr() for t in ptrs], out.data_ptr(), num_sms, _stream_ptr(index), *form))
    return out


def _launch_plain(input, offsets, weight, scales, table2, layer, form=None):
    return _launch_grouped("qgemm_grouped_ex", (input, offsets, weight, scales, table2), weight, (input.shape[0],),
                           scales.shape[1], (input.shape[0], scales.shape[1]), layer, form=(form,))


# `_launch_glu`'s form for the block launch behind its own entry (flute_qgemm_grouped_glu_blocks): not one of `_GROUPED_FORMS`,
# which keep their meaning on `qgemm_grouped_glu` ("blocks" raises there)
_GLU_BLOCKS = "glu_blocks"
_FLUTE_ERR_SHAPE, _FLUTE_ERR_NULL = -4, -9       # include/flute_amd.h


def _launch_glu(input, rows, offsets, gw, gs, gt, uw, us, ut, layer, form=None):
    Tsrc = input.shape[0]
    R = Tsrc if rows is None else rows.shape[0]
    name, form = ("qgemm_grouped_glu_blocks", ()) if form == _GLU_BLOCKS else ("qgemm_grouped_glu_ex", (form,))
    return _launch_grouped(name, (input, rows, offsets, gw, gs, gt, uw, us, ut), gw, (R, Tsrc),
                           gs.shape[1], (R, gs.shape[1]), layer, form=form)


def _require_glu_blocks(name, input, rows, gate_weight, gate_scales, layer):
    """Raise ValueError where flute_qgemm_grouped_glu_blocks does not serve the shape.  Host only, before anything is launched:
    the entry refuses a shape before it looks at a pointer, so it is asked with null pointers (FLUTE_ERR_SHAPE: not served)."""
    num_bits, group_size, template_id, _ = layer
    Tsrc = input.shape[0]
    R = Tsrc if rows is None else rows.shape[0]
    E, P, K = gate_weight.shape
    if max(R, Tsrc) >= 2 ** 31:
        raise ValueError
    rc = _lib.get().flute_qgemm_grouped_glu_blocks(
        _DTYPE_ID[input.dtype], num_bits, group_size, E, R, Tsrc, gate_scales.shape[1], K, P, template_id,
        None, None if rows is None else 1, *(None,) * 8, 0, None)          # (`rows` is compared with null only)
    if rc == _FLUTE_ERR_SHAPE:
        raise ValueError(f"flute_amd.{name}: the block form of the fused GLU launch is not eligible for this shape "
                         "(include/flute_amd.h, flute_qgemm_grouped_glu_blocks: 4 / 2 bits, (K / group_size) % 8 == 0, "
                         "F % 256 == 0, Tsrc * K * 2 below 2^32 - 16)")
    if rc not in (0, _FLUTE_ERR_NULL):
        _lib.check(rc)


def _launch_weighted(input, offsets, weight, scales, table2, row_weight, layer, form=None):
    return _launch_grouped("qgemm_grouped_weighted_ex", (input, offsets, weight, scales, table2, row_weight), weight,
                           (input.shape[0],), scales.shape[1], (input.shape[0], scales.shape[1]), layer, form=(form,))


def qgemm_grouped(input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor,
                  table2: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms=None,
                  form=None) -> torch.Tensor:
    """`qgemm` for the E experts of a mixture-of-experts layer in one launch: out[r] = input[r] @ W_e^T for the rows
    r in [offsets[e], offsets[e + 1]).  `input` [T, K] holds the rows sorted by expert, `offsets` is an int32 CUDA tensor
    of E + 1 elements (0, non-decreasing, T last), `weight` [E, P, K], `scales` [E, N, K / g] and `table2`
    [E, 2^b, 2^b, 1] are E layers packed as `FluteLinear`'s buffers with one num_bits, group_size and template_id.
    Returns [T, N] in input.dtype; rows no expert covers are left unwritten, and a table that decreases or whose
    ranges overlap is memory-safe (every index is clamped to T) but leaves the contents of the rows it names twice unspecified.  The host never reads `offsets` (no
    synchronise: the call can be captured in a graph and replayed on other row counts of the same T).  A native HIP
    kernel on the current stream; the same arguments give the same bits.
    `form`: None - the library chooses from the shapes alone (`flute_amd.dev.grouped_form`): the row form (qgemm_grouped.h) for
    decode-sized row counts, the block form (qgemm_grouped_blocks.h: 128-row blocks of the dense prefill kernel) from a mean of
    32 rows per expert on (64 where the experts' column blocks do not fill the chip) where the layer is eligible for it;
    "rows" / "blocks" force one (forcing blocks on a layer that is not eligible raises).  In the block form a malformed table may also leave rows it does name unwritten."""
    _validate_grouped(input, offsets, weight, scales, table2, num_bits, group_size)
    _grouped_form_id(form)
    layer = (num_bits, group_size, template_id, num_sms)
    if _records_grad(input, scales, table2):
        _refuse_stack_grads("qgemm_grouped", scales, table2)
        return _GroupedFunction.apply(input, scales, None, offsets, weight, table2, layer, form)
    return _launch_plain(input, offsets, weight, scales, table2, layer, form)


class _GroupedFunction(torch.autograd.Function):
    """`qgemm_grouped` under autograd: the same launch (rows no expert serves then zeroed), dX = qgemm_grouped_input_grad(dY)
    and - for `integrations.learnable`; the op itself refuses scales that require grad -
    dS = qgemm_grouped_scale_grad(dY, x), the only reader of the saved `input`.  With `codebook` - a stack's fp32 master,
    which `integrations.learnable` passes next to the `table2` it built from it (`_grouped_codebook_table2`) - the
    backward's parameter gradients are `_grouped_table_grads`: one qgemm_grouped_table_grad launch for both."""

    @staticmethod
    def forward(ctx, input, scales, codebook, offsets, weight, table2, layer, form=None):
        out = _launch_plain(input, offsets, weight, scales, table2, layer, form)
        ctx.save_for_backward(offsets, weight, scales, table2, *((input,) if any(ctx.needs_input_grad[1:3]) else ()))
        ctx.layer = layer
        ctx.scalar = codebook is not None and codebook.ndim == 2
        return _zero_unserved_(out, offsets)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        offsets, weight, scales, table2, *saved_input = ctx.saved_tensors
        d_input = d_scales = d_codebook = None
        if ctx.needs_input_grad[0]:
            d_input = qgemm_grouped_input_grad(grad_output, offsets, weight, scales, table2, *ctx.layer)
        if any(ctx.needs_input_grad[1:3]):
            d_scales, d_codebook = _grouped_table_grads(grad_output, saved_input[0], offsets, weight, scales, table2,
                                                        ctx.layer, *ctx.needs_input_grad[1:3], ctx.scalar)
        return (d_input, d_scales, d_codebook) + (None,) * 5


def _validate_grouped_glu(input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2,
                          num_bits, group_size, rows):
    _validate_grouped(input, offsets, gate_weight, gate_scales, gate_table2, num_bits, group_size)
    _validate_grouped(input, offsets, up_weight, up_scales, up_table2, num_bits, group_size)
    if tuple(up_scales.shape) != tuple(gate_scales.shape):          # (weight and table2 follow from the scales' shape)
        raise ValueError
    if rows is not None:
        if rows.dtype != torch.int32:
            raise TypeError
        if rows.ndim != 1:
            raise ValueError


def _validate_grouped_glu_pos(input, rows, pos):
    """`pos` [Tsrc, k] int32, the inverse of `rows` [Tsrc k] (which it needs); None passes."""
    if pos is None:
        return
    if rows is None or pos.dtype != torch.int32:
        raise TypeError
    if pos.ndim != 2 or pos.shape[0] != input.shape[0] or pos.shape[0] * pos.shape[1] != rows.shape[0]:
        raise ValueError


def qgemm_grouped_glu(input: torch.Tensor, offsets: torch.Tensor, gate_weight: torch.Tensor, gate_scales: torch.Tensor,
                      gate_table2: torch.Tensor, up_weight: torch.Tensor, up_scales: torch.Tensor,
                      up_table2: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms=None,
                      rows=None, pos=None, form=None, native_glu_grad: bool = False) -> torch.Tensor:
    """The gated half of a mixture-of-experts MLP in one launch: out[r] = silu(x_r @ Wgate_e^T) * (x_r @ Wup_e^T) for
    the rows r in [offsets[e], offsets[e + 1]), x_r = input[rows[r]] (`rows`: an int32 CUDA tensor of R entries, each
    clamped to input's rows by the kernel; None: x_r = input[r]).  Gate and up are two stacks as `qgemm_grouped` takes
    one, of one shape, num_bits, group_size and template_id.  Both products stay in fp32 until the one rounding of the
    result (include/flute_amd.h, flute_qgemm_grouped_glu); nothing intermediate is written.  Returns [R, F] in
    input.dtype, rows no expert covers left unwritten.  The host reads neither `offsets` nor `rows` (no synchronise,
    capturable); a native HIP kernel on the current stream (qgemm_grouped.h); equal arguments give equal bits.
    `pos` (`moe_route`'s [Tsrc, k] int32, the inverse of `rows`) is read by the backward only: with it the gradient of the
    gather is `moe_combine(dx_sorted, pos, offsets)` - fp32, one rounding, equal bits at every k - without it `index_add_`.
    `form` as `qgemm_grouped`'s; on this op None and "rows" are the row form at every row count and "blocks" raises: the block
    form of the launch is an op of its own, `qgemm_grouped_glu_blocks`.  (The backward's recompute of gate and up is two plain grouped launches, which do choose automatically.)
    `native_glu_grad` is read by the backward only: False (the default) forms the gather and dg, du with torch ops, bit for bit
    as before; True runs `moe_gather` and `swiglu_grad` in their place (two launches, g and u never widened to fp32 tensors),
    whose bits differ from the torch chain's within `flute_swiglu_grad`'s error account.  The forward's bits do not depend on it."""
    _validate_grouped_glu(input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2,
                          num_bits, group_size, rows)
    _validate_grouped_glu_pos(input, rows, pos)
    _grouped_form_id(form)
    layer = (num_bits, group_size, template_id, num_sms)
    if _records_grad(input, gate_scales, gate_table2, up_scales, up_table2):
        _refuse_stack_grads("qgemm_grouped_glu", gate_scales, gate_table2, up_scales, up_table2)
        return _GroupedGluFunction.apply(input, gate_scales, up_scales, None, None, rows, pos, offsets, gate_weight,
                                         gate_table2, up_weight, up_table2, layer, form, bool(native_glu_grad))
    return _launch_glu(input, rows, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2, layer,
                       form)


def qgemm_grouped_glu_blocks(input: torch.Tensor, offsets: torch.Tensor, gate_weight: torch.Tensor, gate_scales: torch.Tensor,
                             gate_table2: torch.Tensor, up_weight: torch.Tensor, up_scales: torch.Tensor,
                             up_table2: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms=None,
                             rows=None, pos=None, native_glu_grad: bool = False) -> torch.Tensor:
    """`qgemm_grouped_glu` on the block form, for prefill and training row counts: the same operands, formula and rounding
    (include/flute_amd.h, flute_qgemm_grouped_glu_blocks) on 128-row x 256-column blocks of the dense prefill kernel - all of K
    for gate, then all of K for up, in two fp32 accumulators of the matrix core, a weight dequantised once per 128 rows
    (qgemm_block2.h, GM = 3).  Same validation, same autograd (the backward recomputes gate and up and never depends on which
    kernel ran the forward).  Equal arguments give equal bits; the bits equal `qgemm_grouped_glu`'s on exactly representable
    inputs and may differ elsewhere (another summation order).  A shape the form does not serve raises ValueError before
    anything is launched; `flute_amd.dev.grouped_glu_blocks_form` tells where the form pays.  `native_glu_grad` as there."""
    _validate_grouped_glu(input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2,
                          num_bits, group_size, rows)
    _validate_grouped_glu_pos(input, rows, pos)
    layer = (num_bits, group_size, template_id, num_sms)
    _require_glu_blocks("qgemm_grouped_glu_blocks", input, rows, gate_weight, gate_scales, layer)
    if _records_grad(input, gate_scales, gate_table2, up_scales, up_table2):
        _refuse_stack_grads("qgemm_grouped_glu_blocks", gate_scales, gate_table2, up_scales, up_table2)
        return _GroupedGluFunction.apply(input, gate_scales, up_scales, None, None, rows, pos, offsets, gate_weight,
                                         gate_table2, up_weight, up_table2, layer, _GLU_BLOCKS, bool(native_glu_grad))
    return _launch_glu(input, rows, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2, layer,
                       _GLU_BLOCKS)


class _GroupedGluFunction(torch.autograd.Function):
    """`qgemm_grouped_glu` (and, with form `_GLU_BLOCKS`, `qgemm_grouped_glu_blocks`) under autograd.  The fused forward keeps nothing intermediate, so the backward recomputes
    g and u with two plain grouped launches on the gathered rows, forms dg = dh u sigma(g) (1 + g (1 - sigma(g))) and
    du = dh silu(g) in fp32, and gets dx_sorted from ONE pair-form launch of the input-gradient kernel.  For
    `integrations.learnable` (the op itself refuses scales that require grad) dS_gate = qgemm_grouped_scale_grad(dg,
    x_sorted) and dS_up = (du, x_sorted), one launch per stack on the tensors the backward has formed.  With `gc` / `uc` -
    the stacks' fp32 master codebooks, which `gt` / `ut` were built from - each stack's parameter gradients are
    `_grouped_table_grads` on the same operands."""

    @staticmethod
    def forward(ctx, input, gs, us, gc, uc, rows, pos, offsets, gw, gt, uw, ut, layer, form=None, native=False):
        ctx.scalar = (gc is not None and gc.ndim == 2, uc is not None and uc.ndim == 2)
        ctx.native = native
        out = _launch_glu(input, rows, offsets, gw, gs, gt, uw, us, ut, layer, form)
        ctx.save_for_backward(input, offsets, gw, gs, gt, uw, us, ut, *[t for t in (rows, pos) if t is not None])
        ctx.has = (rows is not None, pos is not None)
        ctx.layer = layer
        return _zero_unserved_(out, offsets)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, offsets, gw, gs, gt, uw, us, ut, *index = ctx.saved_tensors
        rows = index[0] if ctx.has[0] else None
        pos = index[1] if ctx.has[1] else None
        dx, x, dg, du = _grouped_glu_backward(grad_output, input, rows, pos, offsets, gw, gs, gt, uw, us, ut, ctx.layer,
                                              want_input_grad=ctx.needs_input_grad[0], native=ctx.native)
        want = ctx.needs_input_grad
        d_gs, d_gc = _grouped_table_grads(dg, x, offsets, gw, gs, gt, ctx.layer, want[1], want[3], ctx.scalar[0])
        d_us, d_uc = _grouped_table_grads(du, x, offsets, uw, us, ut, ctx.layer, want[2], want[4], ctx.scalar[1])
        return (dx, d_gs, d_us, d_gc, d_uc) + (None,) * 10


def _grouped_glu_backward(grad_output, input, rows, pos, offsets, gw, gs, gt, uw, us, ut, layer, want_input_grad,
                          native=False):
    """The backward of the fused GLU launch: (d input, x_sorted, dg, du) - the gathered rows and the two gradients in T
    that the pair-form launch reads, which the scale gradients read too.  `want_input_grad` false skips the pair-form
    launch and the sum over a token's slots (d input: None).  `native` (the ops' `native_glu_grad`): the gather is
    `moe_gather` and dg, du are `swiglu_grad` on g and u as the plain launches wrote them, in T - two launches in place of
    the torch chains, whose bits (torch's sigmoid) they do not promise; rows no expert serves are zeros in x, dg and du."""
    Tsrc = input.shape[0]
    if native:
        x = input if rows is None else moe_gather(input, rows, offsets)
        g = _launch_plain(x, offsets, gw, gs, gt, layer)
        u = _launch_plain(x, offsets, uw, us, ut, layer)
        dg, du = swiglu_grad(g, u, grad_output, offsets)
    else:
        x = input if rows is None else input.index_select(0, rows.clamp(0, Tsrc - 1).long())
        g = _launch_plain(x, offsets, gw, gs, gt, layer).float()
        u = _launch_plain(x, offsets, uw, us, ut, layer).float()
        dh = grad_output.float()
        sig = torch.sigmoid(g)
        dg = (dh * u * sig * (1 + g * (1 - sig))).to(input.dtype)
        du = (dh * (g * sig)).to(input.dtype)
    if not want_input_grad:
        return None, x, dg, du
    dx = qgemm_grouped_input_grad(dg, offsets, gw, gs, gt, *layer, grad_output2=du, weight2=uw, scales2=us, table22=ut)
    if rows is not None:
        if pos is not None:
            dx = moe_combine(dx, pos, offsets)
        else:
            dx = torch.zeros_like(input).index_add_(0, rows.clamp(0, Tsrc - 1).long(), dx)
    return dx, x, dg, du


def _validate_grouped_weighted(input, offsets, weight, scales, table2, row_weight, num_bits, group_size):
    _validate_grouped(input, offsets, weight, scales, table2, num_bits, group_size)
    _check_row_weight(row_weight, input.shape[0])


def qgemm_grouped_weighted(input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor,
                           table2: torch.Tensor, row_weight: torch.Tensor, num_bits: int, group_size: int,
                           template_id: int, num_sms=None, form=None, native_router_grad: bool = False) -> torch.Tensor:
    """`qgemm_grouped` with the routing weight in its epilogue: out[r] = row_weight[r] * (input[r] @ W_e^T), the
    product in fp32 before the one rounding (`row_weight`: an fp32 CUDA tensor of T entries), and the rows from
    offsets[E] on - rows no expert serves - returned as zeros whatever the routing.  No host synchronise; a native
    HIP kernel on the current stream; equal arguments give equal bits.  `form` as `qgemm_grouped`'s.

    `native_router_grad` is read by the backward only, and only when `row_weight` requires grad: False (the default) forms
    d row_weight and d input from the unweighted input gradient with torch ops, bit for bit as before; True runs one
    `moe_weight_grad` launch in their place - d input has the same bits, d row_weight is summed in `flute_moe_weight_grad`'s
    fixed order, not torch's.  The forward's bits do not depend on it."""
    _validate_grouped_weighted(input, offsets, weight, scales, table2, row_weight, num_bits, group_size)
    _grouped_form_id(form)
    layer = (num_bits, group_size, template_id, num_sms)
    if _records_grad(input, row_weight, scales, table2):
        _refuse_stack_grads("qgemm_grouped_weighted", scales, table2)
        return _GroupedWeightedFunction.apply(input, row_weight, scales, None, offsets, weight, table2, layer, form,
                                              bool(native_router_grad))
    return _launch_weighted(input, offsets, weight, scales, table2, row_weight, layer, form)


class _GroupedWeightedFunction(torch.autograd.Function):
    """`qgemm_grouped_weighted` under autograd.  A row weight that needs no gradient rides in the input-gradient kernel's
    epilogue (one launch); one that does takes dH' = input_grad(dY), d row_weight[r] = sum_k dH'[r, k] h[r, k] in fp32
    (zero from offsets[E] on) and dH = round_T(row_weight dH').  For `integrations.learnable` (the op itself refuses
    scales that require grad) dS = qgemm_grouped_scale_grad(dY, h, row_weight=row_weight): the routing weight multiplies
    dY where the kernel stages it.  With `codebook` - the stack's fp32 master, which `table2` was built from - the
    parameter gradients are `_grouped_table_grads` with the same row weight.  `native` (the ops' `native_router_grad`):
    the two results of a row weight that needs a gradient come from one `moe_weight_grad` launch."""

    @staticmethod
    def forward(ctx, input, row_weight, scales, codebook, offsets, weight, table2, layer, form=None, native=False):
        ctx.save_for_backward(input, row_weight, offsets, weight, scales, table2)
        ctx.layer = layer
        ctx.native = native
        ctx.scalar = codebook is not None and codebook.ndim == 2
        return _launch_weighted(input, offsets, weight, scales, table2, row_weight, layer, form)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        input, row_weight, offsets, weight, scales, table2 = ctx.saved_tensors
        want_input, want_weight, want_scales, want_codebook = ctx.needs_input_grad[:4]
        d_input = d_weight = None
        if want_input or want_weight:
            d_input, d_weight = _grouped_weighted_backward(grad_output, *ctx.saved_tensors, ctx.layer, want_input,
                                                           want_weight, native=ctx.native)
        d_scales, d_codebook = _grouped_table_grads(grad_output, input, offsets, weight, scales, table2, ctx.layer,
                                                    want_scales, want_codebook, ctx.scalar, row_weight=row_weight)
        return (d_input, d_weight, d_scales, d_codebook) + (None,) * 6


def _grouped_weighted_backward(grad_output, input, row_weight, offsets, weight, scales, table2, layer, want_input,
                               want_weight, native=False):
    """(d input, d row_weight) of the weighted launch.  `native` (the ops' `native_router_grad`): with `want_weight` the
    unweighted input-gradient launch is followed by one `moe_weight_grad` launch in place of the torch lines below."""
    stack = (offsets, weight, scales, table2)
    if not want_weight:
        return qgemm_grouped_input_grad(grad_output, *stack, *layer, row_weight=row_weight), None
    if native:
        d_weight, d_input = moe_weight_grad(qgemm_grouped_input_grad(grad_output, *stack, *layer), input, row_weight, offsets,
                                            want_input_grad=want_input)
        return d_input, d_weight
    R = input.shape[0]
    dh = qgemm_grouped_input_grad(grad_output, *stack, *layer).float()
    served = torch.arange(R, device=input.device) < offsets[-1].clamp(0, R)
    # (a row no expert serves may hold anything in `input`: its dH' is zero, and the where keeps 0 x NaN out)
    d_weight = torch.where(served, (dh * input.float()).sum(dim=1), torch.zeros((), device=input.device))
    d_input = (row_weight[:, None] * dh).to(input.dtype) if want_input else None
    return d_input, d_weight


def _validate_grouped_input_grad(grad_output, offsets, weight, scales, table2, num_bits, group_size, row_weight,
                                 grad_output2, weight2, scales2, table22):
    _check_ranks((grad_output, 2), (offsets, 1), (weight, 3), (scales, 3), (table2, 4))
    _check_dtypes(grad_output.dtype, like=(scales,), int16=(weight,), fp32=(table2,), int32=(offsets,))
    E, N, K = scales.shape[0], scales.shape[1], weight.shape[2]
    _check_packed(weight, num_bits, group_size, N, K, lead=(E,), table2=table2, offsets=offsets)
    if grad_output.shape[1] != N or scales.shape[2] * group_size != K:
        raise ValueError
    second = (grad_output2, weight2, scales2, table22)
    if any(t is not None for t in second):
        if any(t is None for t in second):
            raise ValueError("qgemm_grouped_input_grad: the pair form needs grad_output2, weight2, scales2 and table22")
        if row_weight is not None:
            raise ValueError("qgemm_grouped_input_grad: the pair form takes no row_weight")
        if grad_output2.dtype != grad_output.dtype or scales2.dtype != scales.dtype or weight2.dtype != torch.int16 or \
                table22.dtype != torch.float32:
            raise TypeError
        if not all(tuple(t2.shape) == tuple(t.shape) for t2, t in zip(second, (grad_output, weight, scales, table2))):
            raise ValueError
    if row_weight is not None:
        _check_row_weight(row_weight, grad_output.shape[0])


def _grouped_input_grad_row_block():
    return _lib.get().flute_qgemm_grouped_input_grad_row_block()


GROUPED_INPUT_GRAD_ROW_BLOCK = _grouped_input_grad_row_block()      # include/flute_amd.h FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK


def qgemm_grouped_input_grad(grad_output: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor, scales: torch.Tensor,
                             table2: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms=None,
                             row_weight=None, grad_output2=None, weight2=None, scales2=None, table22=None,
                             form=None) -> torch.Tensor:
    """The input gradient of `qgemm_grouped` in one launch: dX[r] = row_weight[r] * (grad_output[r] @ W_e) for the rows r in
    [offsets[e], offsets[e + 1]), W_e [N, K] the dequantized weight of expert e (`flute_amd.dequantize`'s), the sum over
    N in fp32 in the matrix core and one rounding to grad_output.dtype.  `grad_output` [R, N] holds the rows sorted by
    expert; `offsets`, `weight` [E, P, K], `scales` [E, N, K / g], `table2` as `qgemm_grouped` takes them; `row_weight`
    [R] fp32 or None (no multiply).  With `grad_output2`, `weight2`, `scales2`, `table22` - a second stack of the same
    shape - the pair form: dX[r] = grad_output[r] @ W_e + grad_output2[r] @ W2_e, both sums added in fp32 before the one
    rounding (the gradient of a row that fed `qgemm_grouped_glu`'s gate and up); it takes no `row_weight`.  Returns
    [R, K]; the rows from offsets[E] on - rows no expert serves - are zeros, so every element is written.  A workgroup
    walks an expert's rows in blocks of GROUPED_INPUT_GRAD_ROW_BLOCK.  The host never reads `offsets` (no synchronise,
    capturable); a native HIP kernel on the current stream (qgemm_grouped_input_grad.h); equal arguments give equal
    bits.  Not differentiable itself: it raises when grad mode is on and an argument requires grad.

    `form`: None - the library chooses from the shapes alone (`flute_amd.dev.grouped_input_grad_form`): the slab form
    (a workgroup per expert and 128 k) for tens of rows per expert, the block form (qgemm_grouped_input_grad_blocks.h: a
    workgroup per 128-row block of an expert and 256 k, for 4- / 2-bit layers with K % 256 == 0) from a mean row count per
    expert on; "slabs" / "blocks" force one (forcing blocks on a layer that is not eligible raises).  Both forms give the
    same bits; in the block form a malformed table may also leave rows it does name unwritten."""
    _grouped_input_grad_form_id(form)
    _validate_grouped_input_grad(grad_output, offsets, weight, scales, table2, num_bits, group_size, row_weight,
                                 grad_output2, weight2, scales2, table22)
    tensors = (grad_output, offsets, weight, scales, table2, row_weight, grad_output2, weight2, scales2, table22)
    if _records_grad(*tensors):
        raise RuntimeError("flute_amd.qgemm_grouped_input_grad: the backward is once-differentiable (no double backward)")
    R, N = grad_output.shape
    return _launch_grouped("qgemm_grouped_input_grad_ex", tensors, weight, (R,), N, (R, weight.shape[2]),
                           (num_bits, group_size, template_id, num_sms), form=(form,), form_id=_grouped_input_grad_form_id)


def _validate_grouped_scale_grad(grad_output, input, offsets, weight, table2, num_bits, group_size, row_weight):
    _check_ranks((grad_output, 2), (input, 2), (offsets, 1), (weight, 3), (table2, 4))
    _check_dtypes(input.dtype, like=(grad_output,), int16=(weight,), fp32=(table2,), int32=(offsets,))
    _check_packed(weight, num_bits, group_size, grad_output.shape[1], input.shape[1], lead=(weight.shape[0],),
                  table2=table2, offsets=offsets, n_multiple=128)
    if grad_output.shape[0] != input.shape[0]:
        raise ValueError
    if row_weight is not None:
        _check_row_weight(row_weight, input.shape[0])


def qgemm_grouped_scale_grad(grad_output: torch.Tensor, input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor,
                             table2: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms=None,
                             row_weight=None) -> torch.Tensor:
    """The gradient of the scales of `qgemm_grouped`'s stack in one launch: `qgemm_scale_grad` for every expert over the
    rows the device-side table gives it, dS[e, n, j] = round_T(sum_{r in [offsets[e], offsets[e + 1])} sum_{k in group j}
    dYw[r, n] * input[r, k] * L_e[k, n]), L_e the `table2[e]` pair lookup of expert e's codes.  `grad_output` [R, N] and
    `input` [R, K] hold the rows sorted by expert; `offsets`, `weight` [E, P, K] and `table2` as `qgemm_grouped` takes them.
    dYw is `grad_output`, or with `row_weight` [R] fp32 round_T(row_weight[r] * grad_output[r, n]) (the product in fp32) -
    the gradient that reaches `qgemm_grouped_weighted`'s product.  Returns [E, N, K / g] in input.dtype, every element
    written: an expert without rows gets zeros and its codes and table are not read; rows from offsets[E] on are never
    read; offsets are clamped to [0, R].  Sums in fp32 in `qgemm_scale_grad`'s order with one rounding: an expert's slice
    has that op's bits on the expert's rows wherever it does not split M.  The host never reads `offsets` (no
    synchronise, capturable); no scratch, no atomics, equal arguments give equal bits; a native HIP kernel on the current
    stream (param_grad.hip).  Not differentiable itself: it raises when grad mode is on and an argument requires
    grad."""
    _validate_grouped_scale_grad(grad_output, input, offsets, weight, table2, num_bits, group_size, row_weight)
    tensors = (grad_output, input, offsets, weight, table2, row_weight)
    if _records_grad(*tensors):
        raise RuntimeError("flute_amd.qgemm_grouped_scale_grad: the backward is once-differentiable (no double backward)")
    R, K = input.shape
    E, N = weight.shape[0], grad_output.shape[1]
    return _launch_grouped("qgemm_grouped_scale_grad", tensors, weight, (R,), N, (E, N, K // group_size),
                           (num_bits, group_size, template_id, num_sms), row_limit=2 ** 31 - 64)


def _validate_grouped_table_grad(grad_output, input, offsets, weight, scales, table2, num_bits, group_size,
                                 with_scale_grad, row_weight):
    _check_ranks((grad_output, 2), (input, 2), (offsets, 1), (weight, 3), (scales, 3),
                 *(((table2, 4),) if table2 is not None else ()))
    _check_dtypes(input.dtype, like=(grad_output, scales), int16=(weight,),
                  fp32=(table2,) if table2 is not None else (), int32=(offsets,))
    E, N, K = weight.shape[0], grad_output.shape[1], input.shape[1]
    _check_packed(weight, num_bits, group_size, N, K, lead=(E,), table2=table2, offsets=offsets, n_multiple=128)
    if grad_output.shape[0] != input.shape[0] or tuple(scales.shape) != (E, N, K // group_size):
        raise ValueError
    if with_scale_grad and table2 is None:
        raise ValueError("qgemm_grouped_table_grad: with_scale_grad needs table2 (the scale gradient reads the tables)")
    if row_weight is not None:
        _check_row_weight(row_weight, input.shape[0])


def qgemm_grouped_table_grad(grad_output: torch.Tensor, input: torch.Tensor, offsets: torch.Tensor, weight: torch.Tensor,
                             scales: torch.Tensor, num_bits: int, group_size: int, template_id: int, num_sms=None, *,
                             table2=None, with_scale_grad: bool = False, row_weight=None):
    """The gradient of the pair codebooks of `qgemm_grouped`'s stack with the codes fixed: `qgemm_table_grad` for every
    expert over the rows the device-side table gives it, dT2[e, i, j, h] = sum over the pairs (kappa, n) of expert e with
    codes (i, j) at rows (2 kappa, 2 kappa + 1) of sum_{r in [offsets[e], offsets[e + 1])} dYw[r, n] * input[r, 2 kappa + h]
    * scales[e, n, 2 kappa / g], as [E, 2^b, 2^b, 2] fp32; `grouped_pair_grad_to_table_grad` folds it for scalar tables.
    `grad_output` [R, N] and `input` [R, K] hold the rows sorted by expert; `offsets`, `weight` [E, P, K] and `scales`
    [E, N, K / g] as `qgemm_grouped` takes them; dYw is `grad_output`, or with `row_weight` [R] fp32
    round_T(row_weight[r] * grad_output[r, n]) (the product in fp32).  The tables are not read.  With `with_scale_grad`
    (needs `table2` [E, 2^b, 2^b, 1]) the same launch also computes the stack's scale gradient and (dT2, dS) is returned,
    dS bit for bit `qgemm_grouped_scale_grad`'s.  Every element is written: an expert without rows gets zeros and nothing
    of it is read; rows from offsets[E] on are never read; offsets are clamped to [0, R].  An expert's dT2 has
    `qgemm_table_grad`'s bits on the expert's rows wherever that op does not split M.  The host never reads `offsets` (no
    synchronise, capturable): the scratch - `flute_qgemm_grouped_table_grad_scratch_bytes`, one partial per (expert, block)
    - is sized from the shapes alone.  No atomics on global memory, equal arguments give equal bits; native HIP kernels on
    the current stream (param_grad.hip).  Not differentiable itself: it raises when grad mode is on and an argument
    requires grad."""
    _validate_grouped_table_grad(grad_output, input, offsets, weight, scales, table2, num_bits, group_size,
                                 with_scale_grad, row_weight)
    tensors = (grad_output, input, offsets, weight, scales, table2 if with_scale_grad else None, row_weight)
    if _records_grad(*tensors, table2):
        raise RuntimeError("flute_amd.qgemm_grouped_table_grad: the backward is once-differentiable (no double backward)")
    dev = _same_gpu("qgemm_grouped_table_grad", tensors)
    R, K = input.shape
    E, P, N = weight.shape[0], weight.shape[1], grad_output.shape[1]
    if R >= 2 ** 31 - 64:
        raise ValueError
    n = 2 ** num_bits
    dT2 = torch.empty((E, n, n, 2), dtype=torch.float32, device=dev)
    dS = torch.empty((E, N, K // group_size), dtype=input.dtype, device=dev) if with_scale_grad else None
    if E > 0:
        lib = _lib.get()
        nbytes = lib.flute_qgemm_grouped_table_grad_scratch_bytes(num_bits, group_size, E, N, K)
        if nbytes == 0:
            raise ValueError(f"flute_amd.qgemm_grouped_table_grad: no kernel for E = {E}, N = {N}, K = {K}, "
                             f"group size {group_size}")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _abi_call("qgemm_grouped_table_grad", lib.flute_qgemm_grouped_table_grad,
                  (_DTYPE_ID[input.dtype], num_bits, group_size, E, R, N, K, P, template_id),
                  tensors, (dT2, dS, scratch), (nbytes, _num_sms(num_sms, dev)), dev)
    return (dT2, dS) if with_scale_grad else dT2


_INDEX_DTYPE_ID = {torch.int32: 0, torch.int64: 1}
_ROUTE_WEIGHT_DTYPE_ID = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
MOE_ROUTE_MAX_EXPERTS = 1024            # include/flute_amd.h FLUTE_MOE_ROUTE_MAX_EXPERTS
MOE_ROUTE_MAX_PAIRS = 1 << 27           # FLUTE_MOE_ROUTE_MAX_PAIRS


def _validate_moe_route(topk_ids, topk_weights, num_experts):
    if topk_ids.ndim != 2:
        raise ValueError
    if topk_ids.dtype not in _INDEX_DTYPE_ID:
        raise TypeError
    if topk_weights is not None:
        if topk_weights.dtype not in _ROUTE_WEIGHT_DTYPE_ID:
            raise TypeError
        if tuple(topk_weights.shape) != tuple(topk_ids.shape):
            raise ValueError
    if not 0 <= num_experts <= MOE_ROUTE_MAX_EXPERTS:
        raise ValueError
    if topk_ids.shape[0] * topk_ids.shape[1] >= MOE_ROUTE_MAX_PAIRS:
        raise ValueError


def moe_route(topk_ids: torch.Tensor, topk_weights, num_experts: int):
    """The routing of a mixture-of-experts step in one launch: from the router's choice `topk_ids` [T, k] (int32 or
    int64, as `torch.topk` returns them) and `topk_weights` [T, k] (fp16 / bf16 / fp32, or None) to
    (offsets [E + 1] int32, rows [T k] int32, row_weight [T k] fp32 or None, pos [T, k] int32, perm [T k] int32):
    `offsets` and `perm` are `integrations.moe.sort_by_expert`'s (a stable sort by expert; ids outside [0, E) behind
    every expert, past offsets[E]), rows = perm // k is the token of each sorted row (`qgemm_grouped_glu`'s `rows`),
    row_weight = topk_weights.flatten()[perm].float() (`qgemm_grouped_weighted`'s), pos.flatten()[perm] = arange(T k)
    (`moe_combine`'s).  E <= 1024, T k < 2^27; a counting sort in one workgroup, meant for decode-sized T k.  The host
    reads nothing (no synchronise, capturable); a native HIP kernel on the current stream (moe_route.hip); equal
    arguments give equal bits."""
    _validate_moe_route(topk_ids, topk_weights, num_experts)
    if _records_grad(topk_weights):
        return _MoeRouteFunction.apply(topk_ids, topk_weights, num_experts, None)
    return _moe_route_call(topk_ids, topk_weights, num_experts)


MOE_ROUTE_MAX_CHUNKS = 8192             # FLUTE_MOE_ROUTE_MAX_CHUNKS


def _validate_chunk_tokens(chunk_tokens, T):
    """`chunk_tokens` of the wide routing ops: None (automatic) or an int >= 1 that leaves at most MOE_ROUTE_MAX_CHUNKS chunks;
    returns the ABI's value, 0 for automatic."""
    if chunk_tokens is None:
        return 0
    if isinstance(chunk_tokens, bool) or not isinstance(chunk_tokens, int):
        raise TypeError
    if chunk_tokens < 1 or -(-T // chunk_tokens) > MOE_ROUTE_MAX_CHUNKS:
        raise ValueError
    return chunk_tokens


def moe_route_wide(topk_ids: torch.Tensor, topk_weights, num_experts: int, chunk_tokens=None):
    """`moe_route` over many workgroups, for prefill and training token counts: the same five arrays (offsets, rows,
    row_weight, pos, perm), bit for bit, from three launches - count, scan, place (moe_route_wide.hip) - in which chunk c
    of `chunk_tokens` consecutive tokens is one workgroup's and no workgroup waits on another.  `chunk_tokens` None: the
    automatic chunk, the tokens of 512 pairs; an int >= 1 (at most 8192 chunks) is for tests and sweeps.  One chunk (T <=
    chunk_tokens) is served by `moe_route`'s own launch.  The workspace is allocated per call; the host reads nothing
    (no synchronise, capturable); equal arguments give equal bits; autograd as `moe_route`.
    `flute_amd.dev.moe_route_form(T, k, E, gated=False)` says where this form pays."""
    _validate_moe_route(topk_ids, topk_weights, num_experts)
    wide = _validate_chunk_tokens(chunk_tokens, topk_ids.shape[0])
    if _records_grad(topk_weights):
        return _MoeRouteFunction.apply(topk_ids, topk_weights, num_experts, wide)
    return _moe_route_call(topk_ids, topk_weights, num_experts, wide)


class _MoeRouteFunction(torch.autograd.Function):
    """`moe_route` / `moe_route_wide` (`wide`: its chunk_tokens, None for the one-workgroup launch) under autograd: row_weight
    is a permutation of topk_weights, so d topk_weights = d row_weight[pos]."""

    @staticmethod
    def forward(ctx, topk_ids, topk_weights, num_experts, wide):
        offsets, rows, row_weight, pos, perm = _moe_route_call(topk_ids, topk_weights, num_experts, wide)
        ctx.save_for_backward(pos)
        ctx.dtype = topk_weights.dtype
        ctx.mark_non_differentiable(offsets, rows, pos, perm)
        return offsets, rows, row_weight, pos, perm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_offsets, d_rows, d_row_weight, d_pos, d_perm):
        (pos,) = ctx.saved_tensors
        return None, d_row_weight.index_select(0, pos.reshape(-1).long()).view(pos.shape).to(ctx.dtype), None, None


def _moe_route_call(topk_ids, topk_weights, num_experts, wide=None):
    """One routing call: flute_moe_route, or with `wide` (the ABI's chunk_tokens, 0 automatic) flute_moe_route_wide."""
    dev = _same_gpu("moe_route", (topk_ids, topk_weights))      # (refused before anything is allocated)
    T, k = topk_ids.shape
    E = int(num_experts)
    outputs, tail = _routing_arrays(T, k, E, dev, topk_weights is not None, wide)
    _abi_call("moe_route", _lib.get().flute_moe_route if wide is None else _lib.get().flute_moe_route_wide,
              (_INDEX_DTYPE_ID[topk_ids.dtype], 0 if topk_weights is None else _ROUTE_WEIGHT_DTYPE_ID[topk_weights.dtype],
               T, k, E), (topk_ids, topk_weights), outputs, tail, dev)
    offsets, perm, rows, row_weight, pos = outputs[:5]
    return offsets, rows, row_weight, pos, perm


def _routing_arrays(T, k, E, dev, weighted, wide=None):
    """What a routing launch writes, in the ABI's order, and the ABI's arguments behind them: (offsets [E + 1], perm [T k],
    rows [T k], row_weight [T k] fp32 - None unless `weighted` -, pos [T, k]), (); with `wide` (the ABI's chunk_tokens, 0
    automatic) the wide launches' workspace comes behind pos - the queried size, from the caching allocator per call
    (capturable); the kernels write every word they read, so it is not cleared - and the tail is (its bytes, chunk_tokens)."""
    P = T * k
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(P, dtype=torch.int32, device=dev)
    rows = torch.empty(P, dtype=torch.int32, device=dev)
    pos = torch.empty((T, k), dtype=torch.int32, device=dev)
    arrays = (offsets, perm, rows, torch.empty(P, dtype=torch.float32, device=dev) if weighted else None, pos)
    if wide is None:
        return arrays, ()
    nbytes = _lib.get().flute_moe_route_wide_workspace(T, k, E, wide)
    return arrays + (torch.empty(nbytes, dtype=torch.uint8, device=dev),), (nbytes, wide)


_GATE_SCORING_ID = {"softmax": 0, "sigmoid": 1}     # include/flute_amd.h flute_gate_scoring
MOE_GATE_MAX_TOPK = 64                              # FLUTE_MOE_GATE_MAX_TOPK


def _validate_moe_gate(logits, k, scoring, bias, num_experts=None):
    if logits.ndim != 2:
        raise ValueError
    if logits.dtype not in _ROUTE_WEIGHT_DTYPE_ID:
        raise TypeError
    if scoring not in _GATE_SCORING_ID:
        raise ValueError
    T, E = logits.shape
    if num_experts is not None and num_experts != E:
        raise ValueError
    if bias is not None:
        if bias.dtype != torch.float32:
            raise TypeError
        if tuple(bias.shape) != (E,):
            raise ValueError
    if not 1 <= k <= min(E, MOE_GATE_MAX_TOPK) or E > MOE_ROUTE_MAX_EXPERTS:
        raise ValueError
    if T * k >= MOE_ROUTE_MAX_PAIRS:
        raise ValueError


def _moe_gate_call(logits, k, scoring, renormalize, bias, scale, routed, groups=None, wide=None):
    """One gating call: flute_moe_gate, with `routed` _route, with `groups` = (n_group, topk_group, group_score) _limited; with `wide`
    (the ABI's chunk_tokens, 0 automatic; needs `routed`) flute_moe_gate_route_wide, the one entry of both gatings."""
    if wide is not None and groups is None:
        groups = (1, 1, "max")                                  # topk_group == n_group: the unlimited gating
    name = "moe_gate_route_wide" if wide is not None else \
        "moe_gate" + ("_route" if routed else "") + ("" if groups is None else "_limited")
    dev = _same_gpu(name, (logits, bias))                       # (refused before anything is allocated)
    T, E = logits.shape
    k = int(k)
    ids = torch.empty((T, k), dtype=torch.int32, device=dev)
    weights = torch.empty((T, k), dtype=torch.float32, device=dev)
    routing, tail = _routing_arrays(T, k, E, dev, True, wide) if routed else ((), ())
    group_args = () if groups is None else (int(groups[0]), int(groups[1]), _GATE_GROUP_SCORE_ID[groups[2]])
    _abi_call(name, getattr(_lib.get(), "flute_" + name),
              (_ROUTE_WEIGHT_DTYPE_ID[logits.dtype], T, E, k, *group_args, _GATE_SCORING_ID[scoring], int(bool(renormalize)),
               float(scale)), (logits, bias), (ids, weights, *routing), tail, dev)
    if not routed:
        return ids, weights
    offsets, perm, rows, row_weight, pos = routing[:5]
    return ids, weights, offsets, rows, row_weight, pos, perm


class _MoeGateFunction(torch.autograd.Function):
    """The gating ops under autograd: `ids` (and the routing arrays) stay non-differentiable, `weights` - and `row_weight`,
    a permutation of it - get a gradient to `logits`.  The backward differentiates the documented formula in fp32 with
    the kernel's ids held fixed: softmax over all E (or the sigmoid), the gather of the chosen, the optional division by
    their sum, times `scale`; the bias enters the choice only.  `native` (the ops' `native_router_grad`): the same
    derivative from one `moe_gate_grad` launch, which also folds d row_weight back through `pos`; `_moe_gate_entry` carries it."""

    @staticmethod
    def forward(ctx, logits, run, scoring, renormalize, scale, native=False):
        outs = run()
        routed = len(outs) > 2
        ctx.save_for_backward(logits, outs[0], *((outs[5],) if routed else ()))
        ctx.formula = (scoring, bool(renormalize), float(scale))
        ctx.native = native
        ctx.mark_non_differentiable(*[o for o in outs if not o.is_floating_point()])
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        logits, ids, *rest = ctx.saved_tensors
        scoring, renormalize, scale = ctx.formula
        if ctx.native:                                          # one launch: the fold through pos is the kernel's
            dx = moe_gate_grad(logits, ids, grads[1], scoring, renormalize, scale,
                               grad_row_weight=grads[4] if rest else None, pos=rest[0] if rest else None)
            return dx, None, None, None, None, None
        d_weights = grads[1]
        if rest:                                                # row_weight[i] = weights.flatten()[perm[i]], pos the inverse of perm
            d_weights = d_weights + grads[4].index_select(0, rest[0].reshape(-1).long()).view_as(d_weights)
        with torch.enable_grad():
            x = logits.detach().float().requires_grad_(True)
            s = torch.softmax(x, dim=1) if scoring == "softmax" else torch.sigmoid(x)
            w = s.gather(1, ids.long())
            if renormalize:
                w = w / w.sum(dim=1, keepdim=True)
            (dx,) = torch.autograd.grad(w * scale, x, d_weights)
        return dx.to(logits.dtype), None, None, None, None, None


def _moe_gate_op(logits, run, scoring, renormalize, scale, native=False):
    if _records_grad(logits):
        return _MoeGateFunction.apply(logits, run, scoring, renormalize, scale, bool(native))
    return run()


def _moe_gate_entry(logits, k, scoring, renormalize, bias, scale, routed, num_experts=None, groups=None,
                    native_router_grad=False, wide=None):
    """What the four gating ops share: the validation, the launch and, when `logits` records a gradient, `_MoeGateFunction`.
    `groups` = (n_group, topk_group, group_score) or None.  `native_router_grad` is read by the backward only: False (the four
    ops' own) differentiates the formula with torch ops; True - `FluteExperts(native_router_grad=True)` passes it - runs one
    `moe_gate_grad` launch (router_grad.hip) in their place.  The forward's bits do not depend on it.  `wide` (with `routed`):
    `moe_gate_route_wide`'s checked chunk_tokens, None for the one-workgroup launch; the backward is the same either way."""
    if groups is None:
        _validate_moe_gate(logits, k, scoring, bias, num_experts)
    else:
        _validate_moe_gate_limited(logits, k, groups[0], groups[1], scoring, bias, groups[2], num_experts)
    return _moe_gate_op(logits, lambda: _moe_gate_call(logits, k, scoring, renormalize, bias, scale, routed=routed, groups=groups,
                                                       wide=wide),
                        scoring, renormalize, scale, native_router_grad)


def moe_gate(logits: torch.Tensor, k: int, scoring: str = "softmax", renormalize: bool = False, bias=None,
             scale: float = 1.0):
    """The gating of a mixture-of-experts step in one launch: from the router's `logits` [T, E] (fp16 / bf16 / fp32) to
    (ids [T, k] int32, weights [T, k] fp32) - what `moe_route` takes.  In fp32: the score s of an expert is the softmax
    over all E logits (`scoring="softmax"`) or 1 / (1 + exp(-x)) (`"sigmoid"`); slot j holds the expert with the j-th
    largest key, equal keys in ascending expert index (a total order: unlike `torch.topk`, ties are defined), where the
    key is the logit itself or, with `bias` [E] fp32 (DeepSeek-V3's correction bias), s + bias - the bias decides the
    choice only; the weight is s, with `renormalize` divided by the sum of the k chosen scores, then times `scale`.
    1 <= k <= min(E, 64), E <= 1024, T k < 2^27.  The choice is over all E experts; DeepSeek's group-limited
    selection (n_group, topk_group) is `moe_gate_limited`.  One wave per token, no atomics, no host synchronise (capturable); a native HIP kernel on the current
    stream (moe_gate.hip); equal arguments give equal bits, and a token's result does not depend on T or its row."""
    return _moe_gate_entry(logits, k, scoring, renormalize, bias, scale, routed=False)


def moe_gate_route(logits: torch.Tensor, k: int, num_experts=None, scoring: str = "softmax", renormalize: bool = False,
                   bias=None, scale: float = 1.0):
    """`moe_gate` and `moe_route` in one launch: (ids, weights, offsets, rows, row_weight, pos, perm), the first two
    bit for bit `moe_gate(logits, k, ...)`'s and the other five bit for bit `moe_route(ids, weights, E)`'s.
    `num_experts`, when given, must be logits.shape[1].  One workgroup of 16 waves gates the tokens and sorts the
    pairs: meant for decode-sized T, correct for every T the limits admit (moe_gate.hip)."""
    return _moe_gate_entry(logits, k, scoring, renormalize, bias, scale, routed=True, num_experts=num_experts)


_GATE_GROUP_SCORE_ID = {"max": 0, "top2sum": 1}     # include/flute_amd.h flute_gate_group_score
MOE_GATE_MAX_GROUPS = 64                            # FLUTE_MOE_GATE_MAX_GROUPS


def _validate_moe_gate_limited(logits, k, n_group, topk_group, scoring, bias, group_score, num_experts=None):
    if group_score not in _GATE_GROUP_SCORE_ID:
        raise ValueError
    _validate_moe_gate(logits, k, scoring, bias, num_experts)
    E = logits.shape[1]
    if not 1 <= n_group <= MOE_GATE_MAX_GROUPS or E % n_group != 0:
        raise ValueError
    if not 1 <= topk_group <= n_group:
        raise ValueError
    gs = E // n_group
    if k > topk_group * gs:
        raise ValueError
    if group_score == "top2sum" and gs < 2:
        raise ValueError


def moe_gate_limited(logits: torch.Tensor, k: int, n_group: int, topk_group: int, scoring: str = "softmax",
                     renormalize: bool = False, bias=None, scale: float = 1.0, group_score: str = "max"):
    """`moe_gate` with DeepSeek's group-limited selection, in one launch: the E experts are `n_group` contiguous groups of
    gs = E / n_group, the `topk_group` best groups are chosen (equal group keys to the lower group), and the k experts
    are `moe_gate`'s choice among the experts of those groups only - an expert of another group is never chosen,
    whatever its key (vLLM's -inf mask, not the HF code's 0.0 fill).  A group's key is, with `group_score="max"`
    (DeepSeek-V2), its largest expert key (the logit, or s + bias), with `"top2sum"` (DeepSeek-V3) the fp32 sum of its
    two largest s (+ bias), which needs gs >= 2; there a softmax is always normalised over all E, also under
    `renormalize` without a bias.  Scores, keys, tie order, weights, `renormalize` and `scale` are `moe_gate`'s.
    1 <= n_group <= 64, E % n_group == 0, 1 <= topk_group <= n_group, k <= topk_group gs, and `moe_gate`'s limits.
    With topk_group == n_group the result is bit for bit `moe_gate`'s.  Returns (ids [T, k] int32, weights [T, k]
    fp32); no host synchronise (capturable), a native HIP kernel on the current stream (moe_gate.hip), equal arguments
    give equal bits."""
    return _moe_gate_entry(logits, k, scoring, renormalize, bias, scale, routed=False, groups=(n_group, topk_group, group_score))


def moe_gate_route_limited(logits: torch.Tensor, k: int, n_group: int, topk_group: int, num_experts=None,
                           scoring: str = "softmax", renormalize: bool = False, bias=None, scale: float = 1.0,
                           group_score: str = "max"):
    """`moe_gate_limited` and `moe_route` in one launch: (ids, weights, offsets, rows, row_weight, pos, perm), the first
    two bit for bit `moe_gate_limited(logits, k, n_group, topk_group, ...)`'s and the other five bit for bit
    `moe_route(ids, weights, E)`'s.  `num_experts`, when given, must be logits.shape[1].  One workgroup of 16 waves, as
    `moe_gate_route`: meant for decode-sized T, correct for every T the limits admit (moe_gate.hip)."""
    return _moe_gate_entry(logits, k, scoring, renormalize, bias, scale, routed=True, num_experts=num_experts,
                           groups=(n_group, topk_group, group_score))


def moe_gate_route_wide(logits: torch.Tensor, k: int, num_experts=None, scoring: str = "softmax", renormalize: bool = False,
                        bias=None, scale: float = 1.0, n_group: int = 1, topk_group: int = 1, group_score: str = "max",
                        chunk_tokens=None):
    """`moe_gate_route` - with `n_group` > 1 `moe_gate_route_limited` - over many workgroups, for prefill and training
    token counts: (ids, weights, offsets, rows, row_weight, pos, perm), all seven bit for bit the one-workgroup op's.
    Three launches (moe_gate.hip, moe_route_wide.hip): workgroup c gates the `chunk_tokens` tokens of chunk c, one wave per
    token, and counts their experts; a scan over the chunks; every workgroup places its chunk's pairs.  No workgroup
    waits on another.  `chunk_tokens` None: automatic, 16 tokens; an int >= 1 (at most 8192 chunks) is for tests and
    sweeps; one chunk is served by the one-workgroup launch.  topk_group == n_group is the unlimited gating.  The
    workspace is allocated per call; no host synchronise (capturable); equal arguments give equal bits; autograd as
    `moe_gate_route`.  `flute_amd.dev.moe_route_form(T, k, E)` says where this form pays."""
    wide = _validate_chunk_tokens(chunk_tokens, logits.shape[0] if logits.ndim == 2 else 0)
    return _moe_gate_entry(logits, k, scoring, renormalize, bias, scale, routed=True, num_experts=num_experts,
                           groups=(n_group, topk_group, group_score), wide=wide)


def _validate_moe_combine(y, pos, offsets, rows=None):
    _check_ranks((y, 2), (pos, 2), (offsets, 1))
    _check_dtypes(y.dtype, int32=(pos, offsets) if rows is None else (pos, offsets, rows))
    if rows is not None and (rows.ndim != 1 or rows.shape[0] != y.shape[0]):
        raise ValueError
    if y.shape[0] != pos.shape[0] * pos.shape[1] or offsets.shape[0] < 1 or y.shape[1] % 8 != 0 or y.shape[0] >= 2 ** 31:
        raise ValueError


def moe_combine(y: torch.Tensor, pos: torch.Tensor, offsets: torch.Tensor, rows=None) -> torch.Tensor:
    """The end of a mixture-of-experts step in one launch: out[t] = sum over the slots j, ascending, of y[pos[t, j]], in
    fp32 with one rounding to y.dtype.  `y` [T k, N] are the down projection's rows in sorted order (N % 8 == 0), `pos`
    [T, k] int32 and `offsets` [E + 1] int32 are `moe_route`'s.  A slot whose position is outside [0, offsets[E]) - an id
    no expert serves - adds nothing and its row is never read; every element of the [T, N] result is written (a token
    with no served slot is zeros).  No atomics: equal arguments give equal bits for every k.  No host synchronise; a
    native HIP kernel on the current stream (moe_combine.hip).

    `rows` (`moe_route`'s [T k] int32 tensor, or None) is read by the backward only: with it the gradient of `y` is
    `moe_gather(grad_output, rows, offsets)`, one launch, where the default derives the token of every sorted row from `pos`
    with torch ops.  The two have the same bits when `rows`, `pos` and `offsets` are what one routing kernel wrote
    (`moe_route`, `moe_gate_route[_limited]`): then every row below offsets[E] is named by one entry of `pos` and `rows`
    holds its token.  Arrays that do not belong together give the gather of the `rows` handed in."""
    _validate_moe_combine(y, pos, offsets, rows)
    if _records_grad(y):
        return _MoeCombineFunction.apply(y, pos, offsets, rows)
    return _moe_combine_call(y, pos, offsets)


class _MoeCombineFunction(torch.autograd.Function):
    """`moe_combine` under autograd: a gather, dY[r] = dOut[token of sorted row r] for the rows below offsets[E], zero from
    there on (the forward never reads those).  With `rows` (the routing kernel's own token of every sorted row) that is one
    `moe_gather` launch."""

    @staticmethod
    def forward(ctx, y, pos, offsets, rows=None):
        ctx.save_for_backward(pos, offsets, *(() if rows is None else (rows,)))
        return _moe_combine_call(y, pos, offsets)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        pos, offsets, *rows = ctx.saved_tensors
        if rows:
            return moe_gather(grad_output, rows[0], offsets), None, None, None
        T, k = pos.shape
        R = T * k
        dev = pos.device
        p = pos.reshape(-1).long()
        inside = (p >= 0) & (p < R)
        token = torch.arange(T, device=dev).repeat_interleave(k)
        # the token of every sorted row (pos is a permutation of the rows; an entry outside [0, R) names no row)
        rows = torch.full((R + 1,), T, dtype=torch.long, device=dev).scatter_(0, torch.where(inside, p, R), token)[:R]
        named = (rows < T) & (torch.arange(R, device=dev) < offsets[-1].clamp(0, R))
        dy = grad_output.index_select(0, rows.clamp(max=T - 1))
        return dy.masked_fill_(~named[:, None], 0), None, None, None


def _moe_combine_call(y, pos, offsets):
    T, k = pos.shape
    N = y.shape[1]
    out = torch.empty((T, N), dtype=y.dtype, device=y.device)
    _abi_call("moe_combine", _lib.get().flute_moe_combine, (_DTYPE_ID[y.dtype], T, k, offsets.shape[0] - 1, N),
              (y, pos, offsets), (out,))
    return out


def _validate_row_stream_offsets(offsets):
    """`offsets` of the row-stream ops: None, or int32 of E + 1 >= 1 entries - rank, type, length, in that order, a run of
    ValueError, TypeError, ValueError that the callers' three phases cannot hold: written out."""
    if offsets is None:
        return
    if offsets.ndim != 1:
        raise ValueError
    if offsets.dtype != torch.int32:
        raise TypeError
    if offsets.shape[0] < 1:
        raise ValueError


def _refuse_grad(name, *tensors):
    if _records_grad(*tensors):
        raise RuntimeError(f"flute_amd.{name} is not differentiable: it is a piece of a backward (call it on detached tensors "
                           "or under torch.no_grad())")


def _validate_swiglu_grad(g, u, grad_output, offsets):
    _check_ranks((g, 2), (u, 2), (grad_output, 2))
    _check_dtypes(g.dtype, like=(u, grad_output))
    _validate_row_stream_offsets(offsets)
    if not u.shape == grad_output.shape == g.shape or g.shape[1] % 8 != 0 or g.shape[0] >= 2 ** 31:
        raise ValueError


def swiglu_grad(g: torch.Tensor, u: torch.Tensor, grad_output: torch.Tensor, offsets=None):
    """The SwiGLU derivative of the fused GLU launch's backward in one launch: (dg, du) with dg = grad_output u ds(g),
    ds(g) = sigma(g) (1 + g (1 - sigma(g))), and du = grad_output silu(g) - in fp32, in the order include/flute_amd.h states at
    flute_swiglu_grad, one rounding per output.  `g`, `u`, `grad_output` [R, F] of one 16-bit type, F % 8 == 0.  `offsets`
    (an int32 CUDA tensor of E + 1 entries, `moe_route`'s) or None: the rows from offsets[E] on are written as zeros and
    never read; None serves every row.  Every element of both results is written.  Not differentiable (it is a piece of a
    backward: an argument that requires grad, with grad mode on, raises RuntimeError).  No host synchronise (capturable); a
    native HIP kernel on the current stream (swiglu_grad.hip); equal arguments give equal bits."""
    _validate_swiglu_grad(g, u, grad_output, offsets)
    _refuse_grad("swiglu_grad", g, u, grad_output)
    R, F = g.shape
    dg = torch.empty((R, F), dtype=g.dtype, device=g.device)
    du = torch.empty((R, F), dtype=g.dtype, device=g.device)
    _abi_call("swiglu_grad", _lib.get().flute_swiglu_grad,
              (_DTYPE_ID[g.dtype], R, F, 0 if offsets is None else offsets.shape[0] - 1),
              (g, u, grad_output, offsets), (dg, du))
    return dg, du


def _validate_moe_gather(input, rows, offsets):
    _check_ranks((input, 2), (rows, 1))
    _check_dtypes(input.dtype, int32=(rows,))
    _validate_row_stream_offsets(offsets)
    if input.shape[1] % 8 != 0 or (input.shape[0] == 0 and rows.shape[0] > 0) or \
            max(input.shape[0], rows.shape[0]) >= 2 ** 31:
        raise ValueError


def moe_gather(input: torch.Tensor, rows: torch.Tensor, offsets=None) -> torch.Tensor:
    """The row gather of a mixture-of-experts step in one launch, the transpose of `moe_combine`:
    out[r] = input[clamp(rows[r], 0, Tsrc - 1)].  `input` [Tsrc, K] of a 16-bit type, K % 8 == 0, `rows` an int32 CUDA
    tensor of R entries (`moe_route`'s); `offsets` as `swiglu_grad`'s: the rows from offsets[E] on are zeros and their
    `rows[r]` is never read.  A copy: a served row is bit for bit `input.index_select`'s.  Not differentiable (an `input`
    that requires grad, with grad mode on, raises RuntimeError).  No host synchronise (capturable); a native HIP kernel
    on the current stream (swiglu_grad.hip)."""
    _validate_moe_gather(input, rows, offsets)
    _refuse_grad("moe_gather", input)
    Tsrc, K = input.shape
    R = rows.shape[0]
    out = torch.empty((R, K), dtype=input.dtype, device=input.device)
    _abi_call("moe_gather", _lib.get().flute_moe_gather,
              (_DTYPE_ID[input.dtype], R, Tsrc, K, 0 if offsets is None else offsets.shape[0] - 1),
              (input, rows, offsets), (out,))
    return out


def _validate_moe_weight_grad(grad_unweighted, input, row_weight, offsets, want_input_grad):
    _check_ranks((grad_unweighted, 2), (input, 2))
    _check_dtypes(grad_unweighted.dtype, like=(input,))
    _validate_row_stream_offsets(offsets)
    if input.shape != grad_unweighted.shape or input.shape[1] % 8 != 0 or input.shape[0] >= 2 ** 31:
        raise ValueError
    if row_weight is None:
        if want_input_grad:
            raise ValueError("moe_weight_grad: the input gradient needs row_weight")
    else:
        _check_row_weight(row_weight, input.shape[0])


def moe_weight_grad(grad_unweighted: torch.Tensor, input: torch.Tensor, row_weight, offsets=None,
                    want_input_grad: bool = True):
    """The routing weight's share of the weighted launch's backward in one launch: from dH' = `grad_unweighted` [R, K] (the
    unweighted input gradient, `qgemm_grouped_input_grad` without `row_weight`) and h = `input` [R, K] (the weighted launch's
    input), of one 16-bit type, K % 8 == 0, and `row_weight` [R] fp32:
    (d_row_weight [R] fp32 = sum_k dH'[r, k] h[r, k], d_input [R, K] = round_T(row_weight[r] dH'[r, k]) or None).
    The products are exact in fp32 and the sum is taken in the fixed order include/flute_amd.h states at flute_moe_weight_grad (no
    atomics: a row's results depend neither on R nor on its position).  `offsets` as `swiglu_grad`'s: the rows from offsets[E]
    on are +0 in both results and nothing of theirs is read; None serves every row.  `want_input_grad=False` forms the sums
    only (`row_weight` may then be None).  Not differentiable (a piece of a backward).  No host synchronise (capturable); a
    native HIP kernel on the current stream (router_grad.hip); equal arguments give equal bits."""
    _validate_moe_weight_grad(grad_unweighted, input, row_weight, offsets, want_input_grad)
    _refuse_grad("moe_weight_grad", grad_unweighted, input, row_weight)
    R, K = input.shape
    dev = _same_gpu("moe_weight_grad", (input, grad_unweighted, row_weight, offsets))
    d_weight = torch.empty((R,), dtype=torch.float32, device=dev)
    d_input = torch.empty((R, K), dtype=input.dtype, device=dev) if want_input_grad else None
    # (the sums alone read no `row_weight`: the ABI takes row_weight and d_input together or not at all)
    _abi_call("moe_weight_grad", _lib.get().flute_moe_weight_grad,
              (_DTYPE_ID[input.dtype], R, K, 0 if offsets is None else offsets.shape[0] - 1),
              (grad_unweighted, input, row_weight if want_input_grad else None, offsets), (d_weight, d_input), dev=dev)
    return d_weight, d_input


def _validate_moe_gate_grad(logits, ids, grad_weights, scoring, grad_row_weight, pos):
    _check_ranks((logits, 2), (ids, 2))
    _check_dtypes(logits.dtype, int32=(ids,), allowed=_ROUTE_WEIGHT_DTYPE_ID)
    if scoring not in _GATE_SCORING_ID:
        raise ValueError
    (T, E), k = logits.shape, ids.shape[1]
    if ids.shape[0] != T or not 1 <= k <= min(E, MOE_GATE_MAX_TOPK) or E > MOE_ROUTE_MAX_EXPERTS or \
            T * k >= MOE_ROUTE_MAX_PAIRS:
        raise ValueError
    if (grad_row_weight is None) != (pos is None):
        raise ValueError("moe_gate_grad: grad_row_weight and pos are given together")
    if grad_weights is None and pos is None:
        raise ValueError("moe_gate_grad: no incoming gradient (grad_weights, or grad_row_weight with pos)")
    if grad_weights is not None:
        if grad_weights.dtype != torch.float32:
            raise TypeError
        if tuple(grad_weights.shape) != (T, k):
            raise ValueError
    if pos is not None:
        if grad_row_weight.dtype != torch.float32 or pos.dtype != torch.int32:
            raise TypeError
        if tuple(grad_row_weight.shape) != (T * k,) or tuple(pos.shape) != (T, k):
            raise ValueError


def moe_gate_grad(logits: torch.Tensor, ids: torch.Tensor, grad_weights, scoring: str = "softmax",
                  renormalize: bool = False, scale: float = 1.0, grad_row_weight=None, pos=None) -> torch.Tensor:
    """The backward of the four gating ops in one launch: d_logits [T, E] in logits.dtype from `logits` [T, E] (fp16 / bf16 /
    fp32), the forward's `ids` [T, k] int32 held fixed, and the incoming gradient of slot (t, j): `grad_weights`[t, j]
    ([T, k] fp32, or None: 0) plus, with `grad_row_weight` [T k] fp32 and `pos` [T, k] int32 (the routed forms' arrays, given
    together), grad_row_weight[pos[t, j]] where pos[t, j] is in [0, T k).  The scores are recomputed by the forward's device
    function (softmax over all E, or the sigmoid), and the derivative of gather / renormalise / scale is include/flute_amd.h's
    formula at flute_moe_gate_grad, in fp32 in slot order; the bias enters the choice only, so there is none here.  A slot whose
    id is outside [0, E) is skipped; slots that name one expert add.  Every element of the result is written.  Not
    differentiable.  One wave per token, no atomics, no host synchronise (capturable); a native HIP kernel on the current
    stream (router_grad.hip); equal arguments give equal bits, and a token's result does not depend on T or its row."""
    _validate_moe_gate_grad(logits, ids, grad_weights, scoring, grad_row_weight, pos)
    _refuse_grad("moe_gate_grad", logits, grad_weights, grad_row_weight)
    T, E = logits.shape
    out = torch.empty((T, E), dtype=logits.dtype, device=logits.device)
    _abi_call("moe_gate_grad", _lib.get().flute_moe_gate_grad,
              (_ROUTE_WEIGHT_DTYPE_ID[logits.dtype], T, E, ids.shape[1], _GATE_SCORING_ID[scoring], int(bool(renormalize)),
               float(scale)), (logits, ids, grad_weights, grad_row_weight, pos), (out,))
    return out


def _validate_moe_aux_logits(logits, scoring):
    """The values every auxiliary-loss op asks of `logits` [T, E] (ranks and types are checked): T >= 1, 1 <= E <= 1024, T < 2^27."""
    if scoring not in _GATE_SCORING_ID:
        raise ValueError
    T, E = logits.shape
    if T < 1 or not 1 <= E <= MOE_ROUTE_MAX_EXPERTS or T >= MOE_ROUTE_MAX_PAIRS:
        raise ValueError


def _validate_moe_aux_loss(logits, ids, scoring, chunk_tokens):
    """Ranks, then types, then values; returns the ABI's chunk_tokens (0: automatic)."""
    _check_ranks((logits, 2), (ids, 2))
    _check_dtypes(logits.dtype, int32=(ids,), allowed=_ROUTE_WEIGHT_DTYPE_ID)
    if chunk_tokens is not None and (isinstance(chunk_tokens, bool) or not isinstance(chunk_tokens, int)):
        raise TypeError
    _validate_moe_aux_logits(logits, scoring)
    (T, E), k = logits.shape, ids.shape[1]
    if ids.shape[0] != T or not 1 <= k <= min(E, MOE_GATE_MAX_TOPK) or T * k >= MOE_ROUTE_MAX_PAIRS:
        raise ValueError
    return _validate_chunk_tokens(chunk_tokens, T)


def _validate_moe_aux_loss_grad(logits, load, grads, scoring):
    _check_ranks((logits, 2), (load, 1), (grads, 1))
    _check_dtypes(logits.dtype, fp32=(grads,), int32=(load,), allowed=_ROUTE_WEIGHT_DTYPE_ID)
    _validate_moe_aux_logits(logits, scoring)
    if load.shape[0] != logits.shape[1] or grads.shape[0] != 2:
        raise ValueError


def _moe_aux_loss_call(logits, ids, scoring, wide):
    """One flute_moe_aux_loss call: (losses [2] fp32 = (balance, z), load [E] int32, importance [E] fp32); the workspace is the
    queried size, from the caching allocator per call (capturable), and is not cleared: the kernels write every word they read."""
    dev = _same_gpu("moe_aux_loss", (logits, ids))              # (refused before anything is allocated)
    (T, E), k = logits.shape, ids.shape[1]
    load = torch.empty(E, dtype=torch.int32, device=dev)
    importance = torch.empty(E, dtype=torch.float32, device=dev)
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    workspace = torch.empty(_lib.get().flute_moe_aux_loss_workspace(T, E, wide), dtype=torch.uint8, device=dev)
    _abi_call("moe_aux_loss", _lib.get().flute_moe_aux_loss,
              (_ROUTE_WEIGHT_DTYPE_ID[logits.dtype], T, E, k, _GATE_SCORING_ID[scoring], wide), (logits, ids),
              (workspace, load, importance, losses), dev=dev)
    return losses, load, importance


class _MoeAuxLossFunction(torch.autograd.Function):
    """`moe_aux_loss` under autograd: balance and z get a gradient to `logits` from one `moe_aux_loss_grad` launch; the two incoming
    gradients are stacked on the device (a missing one is 0), so nothing synchronises.  load and importance carry none."""

    @staticmethod
    def forward(ctx, logits, ids, scoring, wide):
        losses, load, importance = _moe_aux_loss_call(logits, ids, scoring, wide)
        ctx.save_for_backward(logits, load)
        ctx.scoring = scoring
        ctx.mark_non_differentiable(load, importance)
        return losses[0], losses[1], load, importance

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_balance, d_z, d_load, d_importance):
        logits, load = ctx.saved_tensors
        zero = torch.zeros((), dtype=torch.float32, device=logits.device)
        grads = torch.stack([zero if g is None else g.to(torch.float32).reshape(()) for g in (d_balance, d_z)])
        return moe_aux_loss_grad(logits, load, grads, ctx.scoring), None, None, None


def moe_aux_loss(logits: torch.Tensor, ids: torch.Tensor, scoring: str = "softmax", chunk_tokens=None):
    """The router's auxiliary losses and the per-expert load in two launches: from the router's `logits` [T, E] (fp16 / bf16 /
    fp32) and the gate's picks `ids` [T, k] int32, held fixed, to (balance, z, load, importance).  With p[t, e] the softmax over
    all E as the gate computes it (`scoring="softmax"`) or s / sum_j s_j of s = 1 / (1 + exp(-x)) (`"sigmoid"`), and lse_t the
    log-sum-exp of token t's logits (for either scoring):
    load [E] int32 = the slots that name each expert (an id outside [0, E) counts nowhere: `diff(moe_route(ids).offsets)`; what
    DeepSeek-V3's aux-loss-free balancing updates `moe_gate`'s `bias` from); importance [E] fp32 = sum_t p[t, e];
    balance = E sum_e (load_e / T) (importance_e / T), a 0-dim fp32 tensor - the load-balance loss of Switch / Mixtral, Hugging
    Face's `load_balancing_loss_func` without an attention mask; DeepSeek's is this divided by k; z = mean_t lse_t^2, 0-dim
    fp32 - ST-MoE's router z-loss.  1 <= k <= min(E, 64), E <= 1024, T k < 2^27, T >= 1.
    balance and z are differentiable with respect to `logits` (load is a constant): the backward is one `moe_aux_loss_grad`
    launch, once-differentiable.  load and importance carry no gradient.  Use fp32 or bf16 logits where the losses train: in
    fp16 their gradients, of order E / T^2, fall into the subnormal range.
    Partial sums per chunk of `chunk_tokens` tokens (None: automatic, from T alone; an int >= 1 with at most 8192 chunks is for
    tests and sweeps), then one workgroup that adds the chunks in ascending order in fp64 (moe_aux.hip; include/flute_amd.h,
    flute_moe_aux_loss states the order): no float atomics, equal arguments give equal bits, load does not depend on
    `chunk_tokens`.  The workspace is allocated per call; no host synchronise (capturable); native HIP kernels on the current
    stream.  Out of scope: token masks and padding weights, sequence-wise losses per batch row, and the bias update rule
    itself (two torch ops on `load`)."""
    wide = _validate_moe_aux_loss(logits, ids, scoring, chunk_tokens)
    if _records_grad(logits):
        return _MoeAuxLossFunction.apply(logits, ids, scoring, wide)
    losses, load, importance = _moe_aux_loss_call(logits, ids, scoring, wide)
    return losses[0], losses[1], load, importance


def moe_aux_loss_grad(logits: torch.Tensor, load: torch.Tensor, grads: torch.Tensor, scoring: str = "softmax") -> torch.Tensor:
    """The backward of `moe_aux_loss` in one launch: d_logits [T, E] in logits.dtype from `logits` [T, E] (fp16 / bf16 / fp32),
    `load` [E] int32 (the forward's, a constant) and `grads` [2] fp32 on the GPU = the incoming gradients (g_b, g_z) of balance
    and z.  With a_e = g_b E load_e / T^2 and sm the softmax of the token: softmax scoring p_te (a_e - sum_j a_j p_tj) +
    g_z (2 / T) lse_t p_te; sigmoid scoring s_te (1 - s_te) (a_e - sum_j a_j p_tj) / sum_j s_tj + g_z (2 / T) lse_t sm_te -
    in fp32 in the order include/flute_amd.h states at flute_moe_aux_loss_grad, one rounding to the logits' type; every
    element is written and a zero is +0.  Not differentiable.  One wave per token, no atomics, no host synchronise
    (capturable); a native HIP kernel on the current stream (moe_aux.hip); equal arguments give equal bits, and a token's
    result depends on its own logits, load, grads, T and E only.  Folding this into `moe_gate_grad`'s launch is out of scope."""
    _validate_moe_aux_loss_grad(logits, load, grads, scoring)
    _refuse_grad("moe_aux_loss_grad", logits, grads)
    T, E = logits.shape
    out = torch.empty((T, E), dtype=logits.dtype, device=logits.device)
    _abi_call("moe_aux_loss_grad", _lib.get().flute_moe_aux_loss_grad,
              (_ROUTE_WEIGHT_DTYPE_ID[logits.dtype], T, E, _GATE_SCORING_ID[scoring]), (logits, load, grads), (out,))
    return out
