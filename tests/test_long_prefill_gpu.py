"""qgemm at long-prefill shapes, bit for bit, on both sides of the 32-bit offset limits (tests/test_size_limits_host.py
pins the same guards on the host).

A long-context prefill is one call with M = batch x prompt length: on a K = 28672 layer 37 450 rows of activations pass
2 GiB and 74 899 rows pass 4 GiB.  The block kernels read the activations through a descriptor with 32-bit byte offsets
(qgemm_block2.h:97,111, qgemm_block3.h:96,109) and the planner admits them only while (M + 256) K 2 < 0xfffffff0
(planner.hip choose_block: x32_ok); past it the per-wave kernel takes over.  The outputs, the Hadamard scratch and the binding's
flattening of batch dimensions use 64-bit offsets.  A wrap anywhere would corrupt only the rows beyond 2 or 4 GiB.

The data are exact by construction (tests/exact_cases.py): integer activations in [-4, 4], integer tables, +-2^e scales.
Every partial sum is then exact in fp32 while K 4 max|w| < 2^21, so each output element has one correct value,
round_T(X @ W_exact).  The activations are generated on the device, the premise is checked there, and the reference is
an fp32 torch.mm against the dense exact weight, checked bit for bit against fp64 on the first and last 64 rows and on
the rows whose bytes straddle 2^31 and 2^32.  The last row of X is the accumulator witness (every entry 4), so the
witness sits at the highest offsets.  Every launch through flute_qgemm_ex writes into a NaN-guarded buffer and must leave
the guard bands, the inputs and the workspace state words as they were and every output element written.  The operator
calls (the 3-D input of case e, qgemm_hadamard in case d) allocate their own output: those are compared element by
element with the reference, and case d also checks that X and the state words are unchanged.

Not covered: the backward pass through qgemm_hadamard, which rotates a dX of more than 4 GiB in place
(torch_binding.cpp:188-194).
"""
import math

import pytest
import torch

from tests import exact_cases as E
from tests.qgemm_cases import DevLayer, seed_of, state_words_clean
from tests.support import bits_by_size, make_env

pytestmark = pytest.mark.gpu

LIMIT = 0xFFFFFFF0
GUARD = 4096                    # elements on each side of D
ROWS = 4096                     # row chunk of the device-side checks
K_DEEP = 28672                  # Llama-3-70B's down projection
M_EDGE = (LIMIT - 1) // (2 * K_DEEP) - 256                 # 74 642: the last M x32_ok admits at K = 28672
ROW_2G = (1 << 31) // (2 * K_DEEP)                         # 37 449: its bytes straddle 2^31 (rows of 57 344 B)
ROW_4G = (1 << 32) // (2 * K_DEEP)                         # 74 898: ... and 2^32
M_LONG = 76000                  # X = 4.06 GiB at K = 28672
GIB = 1 << 30


@pytest.fixture(scope="module")
def env():
    e = make_env()
    torch.cuda.reset_peak_memory_stats(e.dev)
    yield e
    print("peak device memory: %.2f GiB" % (torch.cuda.max_memory_allocated(e.dev) / GIB))


def need(gib):
    """Skip when the device cannot hold the case (peak of this module: well under 24 GiB)."""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip("needs %.0f GiB of free device memory, %.1f GiB free" % (gib, free / GIB))


def device_x(M, K, seed, dtype, witness_rows):
    """Integer activations in [-4, 4] from a seeded device generator; `witness_rows` (the last row of every prefix a case
    uses) are the accumulator witness, every entry 4."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty(M, K, dtype=dtype, device="cuda")
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        X[r0:r1] = torch.randint(-4, 5, (r1 - r0, K), generator=gen, device="cuda", dtype=dtype)
    for r in witness_rows:
        X[r] = 4
    return X


class Exact:
    """A layer on the device with its dense exact weight in fp32 and the premise checked."""

    def __init__(self, env, bits, K, N, g, dtype, pair=False, table_max=8):
        lay = E.Layer(bits, K, N, g, dtype, seed_of("long", bits, K, N, g, str(dtype), pair), 32, pair)
        if table_max < 8:                       # a narrower integer table (the Hadamard bound)
            lay.pairs = torch.trunc(lay.pairs * table_max / 8)
            n = 2 ** bits
            lay.table = lay.pairs[:n, 1].to(dtype)
            lay.table2 = lay.pairs.to(dtype).view(n, n, 2).contiguous().view(torch.float32)
            assert not pair
        self.lay = lay
        self.dl = DevLayer(env, lay)
        self.W32 = torch.cat([lay.w_exact(n0, min(N, n0 + 4096), env.dev).float() for n0 in range(0, N, 4096)], 1)
        W = self.W32
        assert torch.equal(W.to(dtype).float(), W) and torch.equal(W * 8, (W * 8).round()), "weights: exact, multiples of 2^-3"
        self.wmax = float(W.abs().max())
        assert K * 4 * self.wmax < E.EXACT_SUM_LIMIT, ("sum |x w| may reach 2^21", K, self.wmax)

    def witness(self, x_row):
        E.assert_witness(x_row.double().cpu(), self.lay.w_exact(0, 64), self.lay.dtype)

    def reference(self, X):
        """round_T(X @ W_exact) from fp32 (exact under the premise), row chunk by row chunk."""
        T = self.lay.dtype
        R = torch.empty(X.shape[0], self.lay.N, dtype=T, device=X.device)
        for r0 in range(0, X.shape[0], ROWS):
            C = X[r0:r0 + ROWS].float() @ self.W32
            assert torch.isfinite(C).all()
            if T == torch.float16:
                assert float(C.abs().max()) <= E.FP16_MAX
            R[r0:r0 + ROWS] = C.to(T)
        return R

    def cross_check(self, X, R, rows):
        """On `rows`, the fp32 product equals the fp64 one and R = reference(X) is its rounding to T."""
        rows = torch.tensor(sorted(set(rows)), device=X.device)
        Xb = X[rows]
        R32 = (Xb.float() @ self.W32).double()
        for n0 in range(0, self.lay.N, 4096):
            n1 = min(self.lay.N, n0 + 4096)
            R64 = Xb.double() @ self.lay.w_exact(n0, n1, X.device)
            assert torch.equal(R32[:, n0:n1], R64), ("fp32 reference inexact", n0)
            assert torch.equal(R[rows, n0:n1], R64.to(self.lay.dtype)), ("reference rows differ from round_T(fp64)", n0)


def auto_block(env):
    """Where the block kernels are admitted, 256 CUs plan them (a partitioned part may plan another MFMA kernel)."""
    return (3,) if env.num_sms == 256 else (2, 3, 6)


def bands(M):
    """First and last 64 rows, and the rows whose bytes straddle 2^31 and 2^32 at 57 344-byte rows."""
    return list(range(64)) + list(range(M - 64, M)) + [r for r in (ROW_2G, ROW_4G) if r < M]


def assert_equal_rows(D, R, what):
    for r0 in range(0, D.shape[0], ROWS):
        bad = (D[r0:r0 + ROWS] != R[r0:r0 + ROWS])          # by value: -0.0 == +0.0; NaN never equal
        if bad.any():
            rr = torch.nonzero(bad.any(1))[:, 0] + r0
            pytest.fail("%s: %d elements differ, first row %d, last row %d" % (what, int(bad.sum()), int(rr[0]), int(rr[-1])))


def guarded_launch(env, ex, X, M, ovr, family, R, cfg=None):
    """flute_qgemm_ex on X[:M] with D in the middle of a NaN-filled buffer; checks the plan family (and the block
    configuration `cfg`) before the launch, then the guard bands, coverage, inputs, state words and every element against
    R[:M]."""
    dl, lay = ex.dl, ex.lay
    T, N, K = lay.dtype, lay.N, lay.K
    Xm = X[:M]
    o = env.dev_mod.Overrides(**ovr) if ovr else None
    plan = env.dev_mod.get_plan(M, N, K, lay.bits, lay.g, dl.tid, env.num_sms, T, o, env.ws.numel())
    assert plan["family"] in family and cfg in (None, plan["m_block"]), (M, ovr, plan)
    buf = torch.full((GUARD + M * N + GUARD,), E.NAN_BITS[T], dtype=torch.int16, device=env.dev)
    D = buf[GUARD:GUARD + M * N].view(T)
    before = [bits_by_size(t) for t in (Xm, dl.Q, dl.S, dl.table, dl.table2)]
    with torch.cuda.device(env.dev):
        rc = env.lib.flute_qgemm_ex(
            0 if T == torch.float16 else 1, lay.bits, lay.g, 0, M, N, K, dl.Q.shape[0],
            Xm.data_ptr(), dl.Q.data_ptr(), D.data_ptr(), dl.S.data_ptr(), dl.table.data_ptr(), dl.table2.data_ptr(),
            None, env.ws.data_ptr(), env.ws.numel(), dl.tid, env.num_sms, o, env.stream_ptr(env.dev))
    env.check(rc)
    torch.cuda.synchronize()
    assert torch.all(buf[:GUARD] == E.NAN_BITS[T]) and torch.all(buf[GUARD + M * N:] == E.NAN_BITS[T]), "write outside D"
    D = D.view(M, N)
    for r0 in range(0, M, ROWS):
        assert not torch.isnan(D[r0:r0 + ROWS]).any(), ("output element left unwritten", r0)
    after = [bits_by_size(t) for t in (Xm, dl.Q, dl.S, dl.table, dl.table2)]
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "an input was modified"
    del before, after
    assert state_words_clean(env), "state words left set"
    assert_equal_rows(D, R[:M], (lay, M, ovr, plan["family"]))
    print("%r M=%d %s: family %d m_block %d splitk %d exact" % (lay, M, ovr, plan["family"], plan["m_block"], plan["splitk"]))
    return plan["family"]


def test_x32_edge_and_past_4gib_deep_layers(env):
    """Cases a, b, e: K = 28672.  a: 4-bit fp16 x 1024 columns at M = 74 642 (forced family 3, 256- and 128-row blocks: the
    block kernels at the last M they are admitted for) and 74 643 (forced family 3 falls back to family 2; the automatic
    plan is not family 3).  b: M = 76 000 (X = 4.06 GiB), automatic plans of a 2-bit fp16, a 4-bit bf16 pair-codebook
    (and its forced family 3, which falls back to family 2) and a 3-bit bf16 layer; on the 3-bit layer at M = 74 642
    (X between 2 and 4 GiB) forced 128-row blocks and 16-row blocks, whose idle waves request the offset 0x80000000 -
    inside the descriptor at that size (qgemm_block3.h:104-122).  e: the operator on X shaped [3, 24 881, K] returns the
    bits of the 2-D call."""
    need(16)
    K = K_DEEP
    M_REF = M_EDGE + 1
    assert (M_EDGE + 256) * K * 2 < LIMIT <= (M_REF + 256) * K * 2
    for dtype in (torch.float16, torch.bfloat16):
        X = device_x(M_LONG, K, seed_of("long_x", str(dtype)), dtype, (M_EDGE - 1, M_REF - 1, ROW_4G, M_LONG - 1))
        assert torch.equal(X.abs().amax(), torch.tensor(4.0, dtype=dtype, device=env.dev))
        layers = ([dict(bits=4, N=1024), dict(bits=2, N=1024)] if dtype == torch.float16 else
                  [dict(bits=4, N=1024, pair=True), dict(bits=3, N=1536)])
        for kw in layers:
            ex = Exact(env, K=K, g=64, dtype=dtype, **kw)
            ex.witness(X[-1])
            R = ex.reference(X)
            ex.cross_check(X, R, bands(M_LONG) + [M_EDGE - 1, M_REF - 1])
            fams = {}
            if kw["bits"] == 4 and dtype == torch.float16:                       # case a
                fams["a m_tiles 8"] = guarded_launch(env, ex, X, M_EDGE, dict(family=3, m_tiles=8), (3,), R)
                fams["a m_tiles 4"] = guarded_launch(env, ex, X, M_EDGE, dict(family=3, m_tiles=4), (3,), R)
                fams["a auto"] = guarded_launch(env, ex, X, M_EDGE, None, auto_block(env), R)
                fams["a forced 3 past"] = guarded_launch(env, ex, X, M_REF, dict(family=3, m_tiles=8), (2,), R)
                fams["a auto past"] = guarded_launch(env, ex, X, M_REF, None, (2,), R)
                # case e: batch dimensions flattened by the binding
                dl = ex.dl
                X3 = X[:M_REF].view(3, M_REF // 3, K)
                D2 = env.fa.qgemm(X[:M_REF], dl.Q, dl.S, dl.table, dl.table2, env.ws, 4, 64, dl.tid, env.num_sms)
                D3 = env.fa.qgemm(X3, dl.Q, dl.S, dl.table, dl.table2, env.ws, 4, 64, dl.tid, env.num_sms)
                assert D3.shape == (3, M_REF // 3, ex.lay.N)
                assert torch.equal(bits_by_size(D3.reshape(M_REF, -1)), bits_by_size(D2)), "3-D call differs from the 2-D call"
                assert_equal_rows(D2, R[:M_REF], "operator")
                del D2, D3
            if kw["bits"] == 3:                                                   # 3-bit blocks, 2 GiB < X < 4 GiB
                assert 1 << 31 < M_EDGE * K * 2 < 1 << 32
                fams["b 3-bit m_tiles 4"] = guarded_launch(env, ex, X, M_EDGE, dict(family=3, m_tiles=4), (3,), R, cfg=5)
                fams["b 3-bit m_block 1"] = guarded_launch(env, ex, X, M_EDGE, dict(family=3, m_block=1), (3,), R, cfg=9)
            if kw["bits"] == 4 and dtype == torch.bfloat16:                      # case b, forced family 3
                fams["b forced 3"] = guarded_launch(env, ex, X, M_LONG, dict(family=3), (2,), R)
            fams["b auto"] = guarded_launch(env, ex, X, M_LONG, None, (2,), R)
            print(kw, str(dtype), fams)
            del ex, R
        del X
        torch.cuda.empty_cache()


@pytest.mark.parametrize("bits,dtype", [(4, torch.float16), (3, torch.bfloat16)])
def test_output_past_2_and_4_gib(env, bits, dtype):
    """Case c: 8192 x 28672 (K x N), so D passes 2 GiB at M = 37 450 and 4 GiB (2^31 elements) at M = 74 899, with the
    block kernels admitted (x32_ok holds to M = 261 887): the automatic plan, forced family 3 and forced family 2."""
    need(20)
    K, N = 8192, 28672
    M_HI = ROW_4G + 1
    assert ROW_4G * N < 1 << 31 < M_HI * N                     # the last row's element offsets cross 2^31
    X = device_x(M_HI, K, seed_of("long_c", bits, str(dtype)), dtype, (ROW_2G, ROW_4G))
    ex = Exact(env, bits, K, N, 64, dtype)
    ex.witness(X[-1])
    R = ex.reference(X)
    ex.cross_check(X, R, bands(M_HI) + [ROW_2G - 1, ROW_2G + 1])
    fams = {}
    for M in ((ROW_2G + 1, M_HI) if bits == 4 else (M_HI,)):
        fams[(M, "auto")] = guarded_launch(env, ex, X, M, None, auto_block(env), R)
        fams[(M, "forced 3")] = guarded_launch(env, ex, X, M, dict(family=3), (3,), R)
        fams[(M, "forced 2")] = guarded_launch(env, ex, X, M, dict(family=2), (2,), R)
    print(bits, str(dtype), fams)
    del ex, R, X
    torch.cuda.empty_cache()


def onehot_device(M, K, h, seed, dtype):
    """tests/test_exact_gpu.py:onehot_x on the device: every h-block of a row holds at most three one-hot vectors with
    integer coefficients in [-4, 4], so the 1 / sqrt(h) rotation of h = 256 / 1024 is exact."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty(M, K, dtype=dtype, device="cuda")
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        Y = torch.zeros(r1 - r0, K // h, h, dtype=torch.float32, device="cuda")
        for _ in range(3):
            pos = torch.randint(0, h, (r1 - r0, K // h, 1), generator=gen, device="cuda")
            c = torch.randint(-4, 5, (r1 - r0, K // h, 1), generator=gen, device="cuda").float()
            Y.scatter_add_(2, pos, c)
        X[r0:r1] = Y.view(r1 - r0, K).to(dtype)
    return X


@pytest.mark.parametrize("h", [256, 1024])
def test_hadamard_two_launch_past_4gib(env, h):
    """Case d: qgemm_hadamard at M = 76 000 on 28672 x 1024 (K x N), 4-bit fp16: the rotation runs over M K > 2^31
    elements into the binding's scratch tensor, then the automatic plan (family 2) multiplies."""
    need(16)
    from oracle import flute_oracle as O
    K, dtype, M = K_DEEP, torch.float16, M_LONG
    ex = Exact(env, 4, K, 1024, 64, dtype, table_max=4)          # |t| <= 4 keeps sum |x w| sqrt(h) 8 below 2^24
    dl, lay = ex.dl, ex.lay
    X = onehot_device(M, K, h, seed_of("long_had", h), dtype)
    Hm = torch.as_tensor(O.hadamard_matrix(h)).to(env.dev, torch.float64)
    # the rotated activations (multiples of 1 / sqrt(h), exact in fp16) and their bound, then the reference
    R = torch.empty(M, lay.N, dtype=dtype, device=env.dev)
    worst = 0.0
    for r0 in range(0, M, ROWS):
        Xr = (X[r0:r0 + ROWS].double().view(-1, h) @ Hm).view(-1, K)
        assert torch.equal(Xr.to(dtype).double(), Xr)
        worst = max(worst, float(Xr.abs().sum(1).max()) * ex.wmax)
        Xr32 = Xr.float()
        del Xr
        R[r0:r0 + ROWS] = (Xr32 @ ex.W32).to(dtype)
    assert worst * math.sqrt(h) * 8 < 2.0 ** 24, worst         # multiples of 2^-3 / sqrt(h): every partial sum exact
    for rows in (list(range(64)), list(range(M - 64, M)), [ROW_2G, ROW_4G]):
        Xr = (X[rows].double().view(-1, h) @ Hm).view(-1, K)
        assert torch.equal((Xr @ lay.w_exact(0, lay.N, env.dev)).to(dtype), R[rows]), rows
    assert env.lib.flute_qgemm_hadamard_fused(0, 4, 64, h, M, lay.N, K, dl.tid, env.num_sms, env.ws.numel()) == 0
    fam = env.dev_mod.get_plan(M, lay.N, K, 4, 64, dl.tid, env.num_sms, dtype)["family"]
    assert fam == 2, fam                                          # past x32_ok: the per-wave kernel
    before = bits_by_size(X)
    D = env.fa.qgemm_hadamard(X, dl.Q, dl.S, dl.table, dl.table2, env.ws, 4, 64, h, dl.tid, env.num_sms)
    torch.cuda.synchronize()
    assert torch.equal(before, bits_by_size(X)), "the activations were modified"
    del before
    assert state_words_clean(env)
    assert_equal_rows(D, R, ("hadamard", h))
    print("hadamard h=%d M=%d: family %d exact" % (h, M, fam))
    del ex, X, R, D
    torch.cuda.empty_cache()
