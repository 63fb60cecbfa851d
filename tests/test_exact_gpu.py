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
from tests.qgemm_cases import (FAMILIES, Carved, DevLayer, check_plan, get_layer, guard_bits, guarded_qgemm, onehot_x,
                               run_exact, seed_of, state_words_clean)
from tests.support import env  # noqa: F401

pytestmark = pytest.mark.gpu


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
