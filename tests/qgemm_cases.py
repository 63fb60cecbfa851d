"""What the dense qgemm tests share: the reference's supported shapes, layers of tests/exact_cases.py on the device
between poisoned guard bands, and the guarded launch through the C ABI with the checks every launch gets."""
import torch

from tests import exact_cases as E
from tests.support import bits_by_size, first_template

# the reference's tests/shapes.py:1-96, (N, K)
LLAMA3_8B = [(1024, 4096), (4096, 4096), (4096, 14336), (6144, 4096), (14336, 4096)]
LLAMA3_70B = [(1024, 8192), (8192, 8192), (8192, 28672), (10240, 8192), (28672, 8192)]
LLAMA3_70B_TP2 = [(5120, 8192), (8192, 4096), (8192, 14336), (14336, 8192)]
LLAMA3_70B_TP4 = [(2560, 8192), (7168, 8192), (8192, 2048), (8192, 7168)]
LLAMA3_405B = [(2048, 16384), (2560, 16384), (5120, 16384), (16384, 2048), (16384, 4096), (16384, 6656),
               (16384, 16384), (16384, 53248), (16384, 13312), (53248, 16384), (20480, 16384),
               (26624, 16384), (13312, 16384), (106496, 16384)]
LLAMA3_EXTRA_VLLM = [(28672, 4096), (57344, 8192)]
GEMMA2_9B = [(2048, 3584), (3584, 4096), (3584, 14336), (4096, 3584), (14336, 3584), (8192, 3584),
             (28672, 3584)]
GEMMA2_27B = [(2048, 4608), (4096, 4608), (4608, 4096), (4608, 36864), (36864, 4608), (8192, 4608),
              (73728, 4608), (4608, 2048), (4608, 18432), (4608, 1024), (4608, 9216), (18432, 4608)]
SUPPORTED_SHAPES = (LLAMA3_8B + LLAMA3_70B + LLAMA3_70B_TP2 + LLAMA3_70B_TP4 + LLAMA3_405B +
                    LLAMA3_EXTRA_VLLM + GEMMA2_9B + GEMMA2_27B)
assert len(SUPPORTED_SHAPES) == len(set(SUPPORTED_SHAPES)) == 53

FAMILIES = (0, 2, 3, 5, 6, 7, 8)       # the kernel families of the forced plan matrix (exact_cases.forced_matrix)
GUARD = 4096            # elements on each side of D and of every operand: a multiple of 16 B, the middle stays 16-B aligned
Q_GUARD_BITS = 0x5A5A   # the code pattern around the packed weight
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32}


def guard_bits(t, T):
    """What surrounds operand `t` of a layer in T: NaN in T (both halves of a table2 pair word), a code pattern for Q."""
    if t.dtype == torch.int16:
        return Q_GUARD_BITS
    nan = E.NAN_BITS[T]
    return nan << 16 | nan if t.element_size() == 4 else nan


class Carved:
    """A copy of `t` on the device in the middle of a larger buffer filled with `fill` bits, contiguous and 16-B aligned."""

    def __init__(self, t, dev, fill):
        n = t.numel()
        self.fill, self.n = fill, n
        self.buf = torch.full((GUARD + n + GUARD,), fill, dtype=_INT[t.element_size()], device=dev)
        self.buf[GUARD:GUARD + n] = t.contiguous().view(self.buf.dtype).reshape(-1).to(dev)
        self.t = self.buf[GUARD:GUARD + n].view(t.dtype).view(t.shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0 and self.t.shape == t.shape

    def intact(self):
        return bool(torch.all(self.buf[:GUARD] == self.fill) and torch.all(self.buf[GUARD + self.n:] == self.fill))


seed_of = E.seed_of


class DevLayer:
    """A Layer with its packed weight and tables on the device."""

    def __init__(self, env, lay):
        self.lay = lay
        self.tid = first_template(lay.bits, lay.tile_p)
        d = env.dev
        self.set_operands(d, env.utils.pack(lay.W.to(d), lay.bits, [self.tid], env.num_sms), lay.S, lay.table, lay.table2)
        self.witnessed = False

    def set_operands(self, d, Q, S, table, table2):
        T = S.dtype
        self.carved = [Carved(t, d, guard_bits(t, T)) for t in (Q, S, table, table2)]
        self.Q, self.S, self.table, self.table2 = (c.t for c in self.carved)

    def guards_intact(self):
        return all(c.intact() for c in self.carved)


def get_layer(env, kw):
    key = E.layer_key(kw)
    if key not in env.layers:
        env.layers.clear()                       # one layer at a time on the device (the matrix is grouped by layer)
        torch.cuda.empty_cache()
        lay = E.make_layer(kw, seed_of(key))
        env.layers[key] = DevLayer(env, lay)
    return env.layers[key]


def state_words_clean(env):
    return int(env.ws[:65536].view(torch.int32).abs().sum().item()) == 0


def guarded_qgemm(env, dl, X, ovr=None, hadamard_size=0, nan_expected=False):
    """flute_qgemm_ex with D and every operand in the middle of poisoned buffers; checks guards, coverage, inputs, state
    words.  nan_expected: X itself holds a NaN or an Inf (the coverage check then belongs to the clean launch)."""
    lay = dl.lay
    T = lay.dtype
    M, K, N = X.shape[0], lay.K, lay.N
    Xc = Carved(X, env.dev, guard_bits(X, T))
    X = Xc.t
    buf = torch.full((GUARD + M * N + GUARD,), E.NAN_BITS[T], dtype=torch.int16, device=env.dev)
    D = buf[GUARD:GUARD + M * N].view(T)
    assert D.data_ptr() % 16 == 0
    before = [bits_by_size(t) for t in (X, dl.Q, dl.S, dl.table, dl.table2)]
    scratch = torch.empty_like(X) if hadamard_size else None
    o = env.dev_mod.Overrides(**ovr) if ovr else None
    with torch.cuda.device(env.dev):
        rc = env.lib.flute_qgemm_ex(
            0 if T == torch.float16 else 1, lay.bits, lay.g, hadamard_size, M, N, K, dl.Q.shape[0],
            X.data_ptr(), dl.Q.data_ptr(), D.data_ptr(), dl.S.data_ptr(), dl.table.data_ptr(), dl.table2.data_ptr(),
            scratch.data_ptr() if scratch is not None else None, env.ws.data_ptr(), env.ws.numel(), dl.tid, env.num_sms,
            o, env.stream_ptr(env.dev))
    env.check(rc)
    torch.cuda.synchronize()
    assert torch.all(buf[:GUARD] == E.NAN_BITS[T]) and torch.all(buf[GUARD + M * N:] == E.NAN_BITS[T]), "write outside D"
    assert nan_expected or not torch.isnan(D).any(), "output element left unwritten"
    after = [bits_by_size(t) for t in (X, dl.Q, dl.S, dl.table, dl.table2)]
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "an input was modified"
    assert Xc.intact() and dl.guards_intact(), "an operand's guard band was modified"
    assert state_words_clean(env), "state words left set"
    return D.view(M, N).clone()


def check_plan(env, dl, M, ovr, exp):
    lay = dl.lay
    try:
        plan = env.dev_mod.get_plan(M, lay.N, lay.K, lay.bits, lay.g, dl.tid, env.num_sms, lay.dtype, env.dev_mod.Overrides(**ovr))
    except RuntimeError:
        if exp.get("may_refuse"):
            return None
        raise
    for k, v in exp.items():
        if k != "may_refuse":
            assert plan[k] in (v if isinstance(v, tuple) else (v,)), (lay, M, ovr, k, v, plan)
    return plan


def run_exact(env, dl, M, ovr, xseed, repeat=True):
    lay = dl.lay
    X = E.make_x(M, lay.K, xseed, lay.dtype)
    R, A = E.exact_product(X, lay, env.dev, abs_too=True)
    E.premise(X, lay, R.cpu(), A.cpu(), witness=not dl.witnessed)
    dl.witnessed = True
    D1 = guarded_qgemm(env, dl, X, ovr)
    assert E.exact_equal(D1, R, lay.dtype), (lay, M, ovr, int((D1.double().cpu() != R.to(lay.dtype).double().cpu()).sum()))
    if repeat:
        D2 = guarded_qgemm(env, dl, X, ovr)
        assert torch.equal(bits_by_size(D1), bits_by_size(D2)), ("repeat launch differs", lay, M, ovr)
    return D1


def onehot_x(M, K, h, seed, dtype):
    """Each h-block of every row: at most three one-hot vectors with integer coefficients in [-4, 4]."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.zeros(M, K // h, h, dtype=torch.float64)
    for _ in range(3):
        pos = torch.randint(0, h, (M, K // h, 1), generator=gen)
        c = torch.randint(-4, 5, (M, K // h, 1), generator=gen).double()
        X.scatter_add_(2, pos, c)
    return X.reshape(M, K).to(dtype)
