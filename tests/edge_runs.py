"""How the hostile-operand tests (tests/op_edge_cases.py) launch: every call goes through the C ABI with its outputs and
row operands in the middle of poisoned buffers, and afterwards the guards are intact, the inputs unmodified and (clean
launches) no canary is left where the op promises to write."""
import torch

from tests import exact_cases as XC
from tests import op_edge_cases as OE
from tests.grouped_cases import stack_exact
from tests.qgemm_cases import GUARD, Carved
from tests.support import bits_by_size

F16 = torch.float16
FILL32 = {torch.int32: 0x5A5A5A5A, torch.float32: 0x7FC00000}      # around offsets / rows: a huge index; around row_weight: NaN


def carve(env, t, T):
    """A row operand in the middle of a poisoned buffer: NaN of T around floating data, a huge index around int32."""
    fill = FILL32[t.dtype] if t.element_size() == 4 else XC.NAN_BITS[T]
    return Carved(t, env.dev, fill)


class Out:
    """An output of `shape` in the middle of a canary-filled buffer (NaN bits of its type)."""

    def __init__(self, env, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        wide = dtype == torch.float32
        self.fill = FILL32[torch.float32] if wide else XC.NAN_BITS[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.fill, dtype=torch.int32 if wide else torch.int16, device=env.dev)
        self.mid = self.buf[GUARD:GUARD + n]
        self.t = self.mid.view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool(torch.all(self.buf[:GUARD] == self.fill) and torch.all(self.buf[GUARD + self.mid.numel():] == self.fill))

    def canaries(self):
        return int((self.mid == self.fill).sum())


def guarded(env, fn, args, carved, outs, nan_expected=False):
    """fn(*args) with the checks every launch gets.  carved: the Carved row operands; outs: the Out buffers."""
    before = [bits_by_size(c.t) for c in carved]
    with torch.cuda.device(env.dev):
        rc = fn(*args)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs), "write outside the output"
    assert all(torch.equal(b, bits_by_size(c.t)) for b, c in zip(before, carved)), "an input was modified"
    assert all(c.intact() for c in carved), "an operand's guard band was modified"
    if not nan_expected:
        assert all(o.canaries() == 0 for o in outs), "an element the op promises to write was left unwritten"
    return [o.t.clone() for o in outs]


class DevStack:
    def __init__(self, env, layers):
        self.Q, self.S, self.t2, self.tid = stack_exact(env, layers)
        self.bits, self.g, self.dtype = layers[0].bits, layers[0].g, layers[0].dtype


def dev_stack(env, layers):
    """The packed stack of a case's layers, built once per module (op_edge_cases.stack hands out one list per stack)."""
    if id(layers) not in env.cache:
        assert env.fa.ops.GROUPED_INPUT_GRAD_ROW_BLOCK == OE.ROW_BLOCK
        env.cache[id(layers)] = (layers, DevStack(env, layers))
    return env.cache[id(layers)][1]


FORWARD_FORM_BLOCKS = 2           # include/flute_amd.h FLUTE_GROUPED_FORM_BLOCKS
GRAD_FORM_SLABS, GRAD_FORM_BLOCKS = 1, 2      # FLUTE_GROUPED_INPUT_GRAD_FORM_SLABS / _BLOCKS


def carve_operands(env, operands, T):
    """(carved, pointers): host tensors among the operands are row operands and get carved, device tensors are the
    stack's, None is a null pointer."""
    carved = [carve(env, t, T) if (t is not None and not t.is_cuda) else None for t in operands]
    ptrs = [None if t is None else (c.t if c is not None else t).data_ptr() for t, c in zip(operands, carved)]
    return [c for c in carved if c is not None], ptrs


def grouped_call(env, name, st, rows, N, operands, out_shape, nan_expected=False, tail=()):
    """flute_<name>(dtype, num_bits, group_size, E, *rows, N, K, P, template_id, *operands, out, num_sms, stream, *tail): host
    tensors among the operands are row operands and get carved, device tensors are the stack's, None is a null pointer;
    tail: the trailing arguments of an _ex entry (the form).  A form that does not serve the shape is refused
    (FLUTE_ERR_SHAPE) and fails the launch's `rc == 0`: no other form answers in its place."""
    T = st.dtype
    E, P, K = st.Q.shape
    carved, ptrs = carve_operands(env, operands, T)
    out = Out(env, out_shape, T)
    args = (0 if T == F16 else 1, st.bits, st.g, E, *rows, N, K, P, st.tid, *ptrs, out.t.data_ptr(), env.num_sms,
            torch.cuda.current_stream(env.dev).cuda_stream, *tail)
    return guarded(env, getattr(env.lib, "flute_" + name), args, carved, [out], nan_expected)[0]


def grouped_table_grad_call(env, st, counts, dY, X, rw=None, nan_expected=False):
    """flute_qgemm_grouped_table_grad with the fused dS: (dT2 [E, 4^b, 2] fp32, dS [E, N, K / g] T), each from the middle of a
    canary-filled buffer; dY, X, offsets and row_weight carved; the scratch of exactly the queried size, prefilled with NaN
    bits, in the middle of a buffer whose guards stay intact."""
    T = st.dtype
    E, P, K = st.Q.shape
    R, N = dY.shape
    assert E == len(counts) and X.shape == (R, K)
    carved, ptrs = carve_operands(env, (dY, X, offsets_tensor(counts), st.Q, st.S, st.t2, rw), T)
    dT2, dS = Out(env, (E, 4 ** st.bits, 2), torch.float32), Out(env, (E, N, K // st.g), T)
    nbytes = env.lib.flute_qgemm_grouped_table_grad_scratch_bytes(st.bits, st.g, E, N, K)
    assert nbytes > 0 and nbytes % 4 == 0
    scratch = Out(env, (nbytes // 4,), torch.float32)
    args = (0 if T == F16 else 1, st.bits, st.g, E, R, N, K, P, st.tid, *ptrs, dT2.t.data_ptr(), dS.t.data_ptr(),
            scratch.t.data_ptr(), nbytes, env.num_sms, torch.cuda.current_stream(env.dev).cuda_stream)
    out = guarded(env, env.lib.flute_qgemm_grouped_table_grad, args, carved, [dT2, dS], nan_expected)
    assert scratch.intact(), "write outside the scratch"
    return out


def offsets_tensor(counts):
    return torch.tensor(OE.offsets_list(counts), dtype=torch.int32)


def _entry(name, form):
    """form None: the old entry (the automatic rule); otherwise the _ex entry with the form named."""
    return (name, ()) if form is None else (name + "_ex", (form,))


def run_forward(env, c, X, nan_expected=False, form=None, counts=None):
    """A forward case of op_edge_cases (plain, weighted or glu) on the activations X; counts: another table over the same
    rows (one that ends early leaves rows no expert serves)."""
    st = dev_stack(env, c.layers)
    off = offsets_tensor(c.counts if counts is None else counts)
    R = sum(c.counts)
    if c.op == "glu":
        up = dev_stack(env, c.up)
        rows = None if c.rows is None else c.rows.int()
        name, tail = _entry("qgemm_grouped_glu", form)
        return grouped_call(env, name, st, (R, X.shape[0]), c.N, (X, rows, off, st.Q, st.S, st.t2, up.Q, up.S, up.t2), (R, c.N),
                            nan_expected, tail)
    if c.op == "weighted":
        name, tail = _entry("qgemm_grouped_weighted", form)
        return grouped_call(env, name, st, (R,), c.N, (X, off, st.Q, st.S, st.t2, c.rw), (R, c.N), nan_expected, tail)
    name, tail = _entry("qgemm_grouped", form)
    return grouped_call(env, name, st, (R,), c.N, (X, off, st.Q, st.S, st.t2), (R, c.N), nan_expected, tail)


def run_grad(env, c, dY, dY2, nan_expected=False, form=None):
    """An input-gradient case of op_edge_cases (single, pair or row-weighted) on dY / dY2."""
    st = dev_stack(env, c.layers)
    off = offsets_tensor(c.counts)
    R = int(off[-1])
    second = (None,) * 4
    if dY2 is not None:
        s2 = dev_stack(env, c.layers2)
        second = (dY2, s2.Q, s2.S, s2.t2)
    name, tail = _entry("qgemm_grouped_input_grad", form)
    return grouped_call(env, name, st, (R,), c.N, (dY, off, st.Q, st.S, st.t2, c.rw, *second), (R, c.K), nan_expected, tail)


def forward_alternatives(c):
    """What a wrong forward result may equal, for diagnose(): an operand's subnormals flushed, saturation at 65504."""
    w = 1 if c.rw is None else c.rw.double()[:, None]
    alt = [("subnormal %s flushed" % n, OE.forward_exact(c.layers, c.counts, c.X, flush_w=fw, flush_x=fx)[0] * w)
           for n, fw, fx in (("w", True, False), ("x", False, True), ("w+x", True, True))]
    return alt + [("saturates at 65504", c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX))]


def grad_alternatives(c):
    alt = [("saturates at 65504", c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX))]
    for n, fw, fy in (("w", True, False), ("dY", False, True), ("w+dY", True, True)):
        R = OE.grad_exact(c.layers, c.counts, c.dY, flush_w=fw, flush_y=fy)[0]
        if c.dY2 is not None:
            R = R + OE.grad_exact(c.layers2, c.counts, c.dY2, flush_w=fw, flush_y=fy)[0]
        alt.append(("subnormal %s flushed" % n, R if c.rw is None else R * c.rw.double()[:, None]))
    return alt


def grad_reference(c):
    """The fp64 result of an input-gradient case on its unpoisoned operands."""
    R = OE.grad_exact(c.layers, c.counts, c.dY)[0]
    if c.dY2 is not None:
        R = R + OE.grad_exact(c.layers2, c.counts, c.dY2)[0]
    return R if c.rw is None else R * c.rw.double()[:, None]


def diagnose(D, dtype, alternatives):
    """Which other result D equals, for the failure message: an operand's subnormals flushed, or saturation at 65504."""
    out = [name for name, R in alternatives if XC.exact_equal(D, R, dtype)]
    out.append("%d NaN, %d inf in D" % (int(torch.isnan(D).sum()), int(torch.isinf(D).sum())))
    return out


def differing(D, R, dtype):
    return int((D.double().cpu() != R.to(dtype).double()).sum())


def check_rule(D, exp, what):
    if not XC.nonfinite_equal(D, exp):
        D = D.cpu()
        rows = [r for r in range(D.shape[0]) if not XC.nonfinite_equal(D[r], exp[r])]
        raise AssertionError((what, "rows that differ", rows[:20], len(rows)))
