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


def grouped_call(env, name, st, rows, N, operands, out_shape, nan_expected=False):
    """flute_<name>(dtype, num_bits, group_size, E, *rows, N, K, P, template_id, *operands, out, num_sms, stream): host tensors
    among the operands are row operands and get carved, device tensors are the stack's, None is a null pointer."""
    T = st.dtype
    E, P, K = st.Q.shape
    carved = [carve(env, t, T) if (t is not None and not t.is_cuda) else None for t in operands]
    ptrs = [None if t is None else (c.t if c is not None else t).data_ptr() for t, c in zip(operands, carved)]
    out = Out(env, out_shape, T)
    args = (0 if T == F16 else 1, st.bits, st.g, E, *rows, N, K, P, st.tid, *ptrs, out.t.data_ptr(), env.num_sms,
            torch.cuda.current_stream(env.dev).cuda_stream)
    return guarded(env, getattr(env.lib, "flute_" + name), args, [c for c in carved if c is not None], [out], nan_expected)[0]


def offsets_tensor(counts):
    return torch.tensor(OE.offsets_list(counts), dtype=torch.int32)


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
