"""Every kernel family, bit for bit, on inputs whose exact product is representable (tests/exact_cases.py).

With integer activations, integer lookup tables and power-of-two scales every partial sum is exact in fp32, so the
documented arithmetic (fp32 accumulation, one rounding of the output) allows one answer only: round_T(X @ W_exact).
Each launch writes into the middle of a NaN-filled buffer, and every operand it reads (X, Q, S, table, table2) sits in
the middle of a poisoned buffer of its own - NaN around the floating operands, a non-zero code pattern around Q - so a
read past an operand's end that is only masked by a multiply with zero reaches the result; afterwards the guard bands
are untouched, no output element is left unwritten, the inputs are unchanged and the in-launch reduction state words
are zero again.  Before
each launch the plan is checked to be the family and variant the case asks for (overrides can fall back or clamp).
Where exactness is impossible (random NF4 data, the 1 / sqrt(512) rotation) a proven per-element bound is checked.
"""
import pytest
import torch

from tests import exact_cases as E

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def env():
    import flute_amd
    from flute_amd import _lib, dev, utils
    from flute_amd.ops import _stream_ptr
    from oracle import flute_oracle as O

    class Env:
        pass

    e = Env()
    e.fa, e.lib, e.dev_mod, e.utils, e.O = flute_amd, _lib.get(), dev, utils, O
    e.check, e.stream_ptr = _lib.check, _stream_ptr
    e.dev = torch.device("cuda:0")
    e.num_sms = utils.get_device_num_sms(e.dev)
    e.ws = utils.get_workspace_streamk(e.dev)
    e.layers = {}
    return e


def first_template(fa, bits, tile_p):
    return min(t for (b, t), c in fa.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == tile_p)


seed_of = E.seed_of


class DevLayer:
    """A Layer with its packed weight and tables on the device."""

    def __init__(self, env, lay):
        self.lay = lay
        self.tid = first_template(env.fa, lay.bits, lay.tile_p)
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


def _bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()]).clone()


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
    before = [_bits(t) for t in (X, dl.Q, dl.S, dl.table, dl.table2)]
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
    after = [_bits(t) for t in (X, dl.Q, dl.S, dl.table, dl.table2)]
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
        assert torch.equal(_bits(D1), _bits(D2)), ("repeat launch differs", lay, M, ovr)
    return D1


FAMILIES = (0, 2, 3, 5, 6, 7, 8)


@pytest.mark.parametrize("family", FAMILIES)
def test_forced_plan_matrix_exact(env, family):
    ran = {}
    for fam, kw, M, ovr, exp in E.forced_matrix():
        if fam != family:
            continue
        dl = get_layer(env, kw)
        plan = check_plan(env, dl, M, ovr, exp)
        if plan is None:
            continue
        run_exact(env, dl, M, ovr, seed_of(fam, M, tuple(sorted(ovr.items()))))
        v = tuple(sorted(ovr.items()))
        ran[v] = ran.get(v, 0) + 1
    assert ran, family
    if family == 6:
        assert len({dict(v).get("splitk") for v in ran}) >= 6, ran
    print("family %d: %d variants, %d launches" % (family, len(ran), sum(ran.values())))


def test_automatic_plans_exact(env):
    reached = {}
    for kw, M in E.auto_grid():
        dl = get_layer(env, kw)
        lay = dl.lay
        plan = env.dev_mod.get_plan(M, lay.N, lay.K, lay.bits, lay.g, dl.tid, env.num_sms, lay.dtype)
        X = E.make_x(M, lay.K, seed_of("auto", M), lay.dtype)
        R, A = E.exact_product(X, lay, env.dev, abs_too=True)
        E.premise(X, lay, R.cpu(), A.cpu(), witness=False)
        Xc = Carved(X, env.dev, guard_bits(X, lay.dtype))
        D = env.fa.qgemm(Xc.t, dl.Q, dl.S, dl.table, dl.table2, env.ws, lay.bits, lay.g, dl.tid, env.num_sms)
        assert E.exact_equal(D, R, lay.dtype), (lay, M, plan["family"])
        assert Xc.intact() and dl.guards_intact(), "an operand's guard band was modified"
        assert state_words_clean(env)
        reached.setdefault(plan["family"], []).append((lay.N, lay.K, M))
    print("automatic plans reached:", {f: len(v) for f, v in sorted(reached.items())})
    if env.num_sms == 256:
        assert set(reached) == E.AUTO_FAMILIES, sorted(reached)


def onehot_x(M, K, h, seed, dtype):
    """Each h-block of every row: at most three one-hot vectors with integer coefficients in [-4, 4]."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.zeros(M, K // h, h, dtype=torch.float64)
    for _ in range(3):
        pos = torch.randint(0, h, (M, K // h, 1), generator=gen)
        c = torch.randint(-4, 5, (M, K // h, 1), generator=gen).double()
        X.scatter_add_(2, pos, c)
    return X.reshape(M, K).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hadamard_exact(env, dtype):
    """h = 16 .. 1024: 1 / sqrt(h) is a power of two, so the rotation of one-hot combinations is exact; fused (decode kernel,
    M * K <= 8192) and two-launch forms, the operator and the rotate-then-multiply composition all return round_T(exact)."""
    K = 2048
    kw = dict(bits=4, K=K, N=3 * 512, g=64, dtype=dtype, tile_p=32, pair=False)
    dl = get_layer(env, kw)
    lay, d = dl.lay, env.dev
    for h in (16, 64, 256, 1024):
        Hm = env.O.hadamard_matrix(h)
        for M in (2, 4, 16):                                   # M * K <= 8192: the rotation can fuse; above: two launches
            X = onehot_x(M, K, h, seed_of("had", h, M), dtype)
            Xr = (X.double().reshape(-1, h) @ Hm).reshape(M, K)
            assert torch.equal(Xr.to(dtype).double(), Xr)
            R, A = E.exact_product(Xr, lay, d, abs_too=True)
            assert float(A.max()) * (h ** 0.5) * 8 < 2.0 ** 24          # multiples of 2^-3 / sqrt(h): every partial sum exact
            fused = env.lib.flute_qgemm_hadamard_fused(0 if dtype == torch.float16 else 1, 4, lay.g, h, M, lay.N, K, dl.tid,
                                                       env.num_sms, env.ws.numel())
            assert fused == (1 if (M * K <= 8192 and h <= 512) else 0), (h, M, fused)
            outs = {
                "operator": env.fa.qgemm_hadamard(X.to(d), dl.Q, dl.S, dl.table, dl.table2, env.ws, 4, lay.g, h, dl.tid, env.num_sms),
                "two": env.fa.qgemm(env.fa.hadamard_transform(X.to(d), h), dl.Q, dl.S, dl.table, dl.table2, env.ws, 4, lay.g, dl.tid, env.num_sms),
                "guarded": guarded_qgemm(env, dl, X, None, hadamard_size=h),
            }
            if M <= 4:
                outs["decode"] = guarded_qgemm(env, dl, X, dict(family=0), hadamard_size=h)
            for name, D in outs.items():
                assert E.exact_equal(D, R, dtype), (h, M, name)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hadamard_512_componentwise(env, dtype):
    """BASELINE.json configs[4]: pair codebook (HIGGS vector_size = 2), h = 512, Gemma-2-9B (N, K) = (4096, 3584).  1 / sqrt(512)
    is not a power of two, so the rotated activations are rounded: the part-4 bound plus the activations' own error."""
    K, N = 3584, 4096
    dl = get_layer(env, dict(bits=4, K=K, N=N, g=64, dtype=dtype, tile_p=32, pair=True))
    lay, d = dl.lay, env.dev
    u = E.U_T[dtype]
    Hm = env.O.hadamard_matrix(512)
    c = (1 + u) * (u + (1 + u) * E.gamma(K + 16))
    e_x = u + (1 + u) * E.gamma(10)                       # fp32 butterflies (log2 512 + 1 operations), one rounding
    for M in (1, 2, 16):
        X = E.make_x(M, K, seed_of("h512", M), dtype, witness=False)
        Xr = (X.double().reshape(-1, 512) @ Hm).reshape(M, K)
        AX = (X.double().abs().reshape(-1, 512) @ Hm.abs()).reshape(M, K)
        R = E.exact_product(Xr, lay, d)
        Abig = E.exact_product(AX, lay, d, abs_too=True)[1]
        D = env.fa.qgemm_hadamard(X.to(d), dl.Q, dl.S, dl.table, dl.table2, env.ws, 4, lay.g, 512, dl.tid, env.num_sms)
        ex = E.componentwise_excess(D, R, Abig, K, dtype, extra=u * e_x + c * e_x + e_x)
        assert ex <= 0, (M, ex)


def test_componentwise_random_nf4(env):
    """Random NF4 codes, randn scales and activations (not exact): one launch per (family, layer) of the forced matrix within
    the proven per-element bound (exact_cases.componentwise_excess)."""
    seen = set()
    for fam, kw, M, ovr, exp in E.forced_matrix():
        key = (fam, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key in seen or kw["N"] * kw["K"] > (64 << 20):
            continue
        dl = get_layer(env, kw)
        if check_plan(env, dl, M, ovr, exp) is None:
            continue
        seen.add(key)
        lay, d, dtype = dl.lay, env.dev, kw["dtype"]
        gen = torch.Generator().manual_seed(seed_of("nf4", key))
        table = torch.tensor(env.O.NF4_VALUES[:2 ** lay.bits], dtype=dtype) if lay.bits == 4 else torch.randn(2 ** lay.bits, generator=gen).to(dtype)
        S = torch.randn(lay.N, lay.K // lay.g, generator=gen).to(dtype)
        X = (torch.randn(M, lay.K, generator=gen) / 10).to(dtype)
        nf = E.Layer.__new__(E.Layer)
        nf.__dict__.update(lay.__dict__)
        n = 2 ** lay.bits
        t = table.double()
        nf.pairs = torch.stack([t[:, None].expand(n, n), t[None, :].expand(n, n)], dim=-1).reshape(n * n, 2)
        nf.S64 = S.double()
        ndl = DevLayer.__new__(DevLayer)
        ndl.__dict__.update(dl.__dict__)
        ndl.lay = nf
        ndl.set_operands(d, dl.Q, S, table, env.utils.make_qmap2_from_qmap(table))
        D = guarded_qgemm(env, ndl, X, ovr)
        R, A = E.exact_product(X, nf, d, abs_too=True)
        ex = E.componentwise_excess(D, R, A, lay.K, dtype)
        assert ex <= 0, (fam, lay, M, ovr, ex)
    assert {f for f, _ in seen} == set(FAMILIES)
