"""flute_amd.qgemm_grouped_scale_grad / flute_qgemm_grouped_scale_grad on the GPU, and the training of the experts'
scales built on it: dS[e] = the dense scale gradient of expert e over the rows a device-side table gives it, one launch.

Kernel level: every non-empty expert's slice is bit for bit `qgemm_scale_grad` on its rows (random data: the dense launch
never splits M at these counts), empty experts are zeros, NaN rows past offsets[E] stay out; the row weight is bit for
bit a pre-multiplied dY; exact layers equal the fp64 reference; random data stays within the componentwise bound of the
documented arithmetic; a direct ABI call writes exactly dS, also on malformed tables; two calls and a graph replay on
other contents give equal bits.  On top: the three learnable entry points return the plain ops' bits and the stated
compositions, `FluteExperts` / `FluteSparseMoeBlock` give the scales the gradient of fp64 autograd as closely as a
per-expert loop of dense learnable layers does, and a dozen Adam steps on the experts' scales learn a teacher."""
import pytest
import torch

from tests import exact_cases as XC
from tests import scale_grad_ref as SR
from tests.grouped_cases import (GRAD_COUNTS, HALF_SUB, MIN_NORMAL, PAD, dense_project, exact_layers, exact_seed,  # noqa: F401
                                 gate_formula, matrix, nan_padded, random_code_layer, restated_experts, scale_leaves,
                                 stack_exact, tiny)
from tests.support import bits16, env, first_template, ints, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16


def random_case_of(env, bits, tile_p, g, dtype, pair, K, N):
    """A random stack (codes, an NF-style table or a pair codebook per expert), its lookups L [K, N] in fp64, random dY
    and X with NaN rows past offsets[E], a row weight, and the launches every test of the case reads - computed once."""
    key = (bits, tile_p, g, dtype, pair, K, N)
    if key not in env.cache:
        d, E, Rs = env.dev, len(GRAD_COUNTS), sum(GRAD_COUNTS)
        assert max(GRAD_COUNTS) <= 224                                    # the dense launch splits M from 8 steps of 32 rows on
        Qs, t2s, Ls = [], [], []
        for e in range(E):
            Q, table2, L = random_code_layer(env, bits, tile_p, dtype, K, N, exact_seed(bits, tile_p, g) + 40 + e, pair)
            Qs.append(Q), t2s.append(table2), Ls.append(L)
        gen = torch.Generator().manual_seed(exact_seed(bits, tile_p, g) + 7)
        dY = nan_padded(torch.randn(Rs, N, generator=gen).to(dtype)).to(d)
        X = nan_padded(torch.randn(Rs, K, generator=gen).to(dtype)).to(d)
        rw = torch.cat([torch.rand(Rs, generator=gen) * 1.5 + 0.25, torch.full((PAD,), float("nan"))]).to(d)
        c = dict(Q=torch.stack(Qs), t2=torch.stack(t2s), L=Ls, dY=dY, X=X, rw=rw, off=offsets_of(GRAD_COUNTS, d),
                 tid=first_template(bits, tile_p), R=Rs + PAD)
        c["dS"] = env.fa.qgemm_grouped_scale_grad(dY, X, c["off"], c["Q"], c["t2"], bits, g, c["tid"])
        c["dSw"] = env.fa.qgemm_grouped_scale_grad(dY, X, c["off"], c["Q"], c["t2"], bits, g, c["tid"], row_weight=rw)
        env.cache[key] = c
    return env.cache[key]


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_bit_equal_with_dense_op(env, bits, tile_p, g, dtype, pair, K, N):
    c = random_case_of(env, bits, tile_p, g, dtype, pair, K, N)
    dS = c["dS"]
    assert dS.shape == (len(GRAD_COUNTS), N, K // g) and dS.dtype == dtype
    assert torch.isfinite(dS).all()                                  # the NaN rows past offsets[E] were not read
    off = offsets_of(GRAD_COUNTS).tolist()
    for e, n in enumerate(GRAD_COUNTS):
        if n == 0:
            assert torch.all(bits16(dS[e]) == 0), e
            continue
        r0, r1 = off[e], off[e + 1]
        dense = env.fa.qgemm_scale_grad(c["dY"][r0:r1], c["X"][r0:r1], c["Q"][e], c["t2"][e], bits, g, c["tid"])
        assert torch.equal(bits16(dS[e]), bits16(dense)), (e, n)
        assert float(dense.abs().max()) > 0


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_row_weight_is_a_premultiplied_grad_output(env, bits, tile_p, g, dtype, pair, K, N):
    """round_T(row_weight[r] * dY[r, n]) with the product in fp32, formed by the kernel, against the same rounding by torch."""
    c = random_case_of(env, bits, tile_p, g, dtype, pair, K, N)
    pre = (c["dY"].float() * c["rw"][:, None]).to(dtype)
    ref = env.fa.qgemm_grouped_scale_grad(pre, c["X"], c["off"], c["Q"], c["t2"], bits, g, c["tid"])
    assert torch.isfinite(c["dSw"]).all()
    assert torch.equal(bits16(c["dSw"]), bits16(ref))
    assert not torch.equal(bits16(c["dSw"]), bits16(c["dS"]))


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_random_within_componentwise_bound(env, bits, tile_p, g, dtype, pair, K, N):
    """Per element |dS - R| <= gamma(M_e g + 2) A + u_T |R|, M_e the expert's rows: fp32 products and sums of M_e g terms in
    any order and one rounding.  With a row weight the operand dYw is itself rounded once to T:
    (u + gamma) A (1 + u) + u |R|, A and R taken with the unrounded fp64 product row_weight dY.
    Both forms model a rounding to T as x (1 + d), |d| <= u, which holds down to T's smallest normal only (MIN_NORMAL,
    fp16: 2^-14); below it the error is absolute, at most HALF_SUB = half the spacing of T's subnormals (fp16: 2^-25).  A
    one-row expert reaches that range where its g terms cancel, or where a row-weighted dY element is itself that small.
    So exactly there the format's underflow term is written out and everywhere else the bounds stand as stated: an element
    with |R| < MIN_NORMAL gets + HALF_SUB for the result's rounding (at |R| >= MIN_NORMAL, u |R| >= HALF_SUB covers it),
    and the weighted form gets + (1 + gamma) HALF_SUB B, B = sum |X[r, k]| |L[k, n]| over the group and over those rows r
    only whose |row_weight[r] dY[r, n]| < MIN_NORMAL.  In bf16 (MIN_NORMAL 2^-126) neither occurs: the terms are zero."""
    c = random_case_of(env, bits, tile_p, g, dtype, pair, K, N)
    u = XC.U_T[dtype]
    sub, tiny = HALF_SUB[dtype], MIN_NORMAL[dtype]
    off = offsets_of(GRAD_COUNTS).tolist()
    for e, n in enumerate(GRAD_COUNTS):
        if n == 0:
            continue
        r0, r1 = off[e], off[e + 1]
        dY, X, L = c["dY"][r0:r1], c["X"][r0:r1], c["L"][e]
        gam = XC.gamma(n * g + 2)
        R, A = SR.scale_grad(dY, X, L, g), SR.scale_grad(dY, X, L, g, absolute=True)
        bound = gam * A + u * R.abs() + sub * (R.abs() < tiny)
        err = (c["dS"][e].double() - R).abs()
        assert torch.all(err <= bound), (e, float((err - bound).max()))
        dYw = dY.double() * c["rw"][r0:r1].double()[:, None]
        R, A = SR.scale_grad(dYw, X, L, g), SR.scale_grad(dYw, X, L, g, absolute=True)
        B = SR.scale_grad((dYw.abs() < tiny).double(), X, L, g, absolute=True)
        bound = (u + gam) * A * (1 + u) + u * R.abs() + sub * (R.abs() < tiny) + (1 + gam) * sub * B
        err = (c["dSw"][e].double() - R).abs()
        assert torch.all(err <= bound), ("weighted", e, float((err - bound).max()))


def check_exact(layers, counts, dY, X, dS, g, dtype):
    """Per expert: integer dY, X and table entries whose absolute sums stay below 2^24 - every partial sum in any order
    is exact in fp32 and round_T(R) is the only allowed answer - and dS[e] == round_T(R) by value."""
    off = offsets_of(counts).tolist()
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            assert torch.all(bits16(dS[e]) == 0), e
            continue
        L = SR.lut_of_codes(lay.W, lay.pairs, lay.bits)
        assert torch.equal(L, L.round())
        R = SR.scale_grad(dY[r0:r1], X[r0:r1], L, g)
        A = SR.scale_grad(dY[r0:r1], X[r0:r1], L, g, absolute=True)
        assert float(A.max()) < 2.0 ** 24 and torch.isfinite(R.to(dtype)).all()
        assert XC.exact_equal(dS[e], R, dtype), (e, lay)


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_exact_layers(env, bits, tile_p, g, dtype, pair, K, N):
    layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, len(GRAD_COUNTS), exact_seed(bits, tile_p, g) + 500)
    Q, _, t2, tid = stack_exact(env, layers)
    Rs = sum(GRAD_COUNTS)
    dY, X = ints(Rs, N, 4, 501 + g, dtype), ints(Rs, K, 2, 502 + g, dtype)
    dS = env.fa.qgemm_grouped_scale_grad(nan_padded(dY).to(env.dev), nan_padded(X).to(env.dev),
                                         offsets_of(GRAD_COUNTS, env.dev), Q, t2, bits, g, tid)
    check_exact(layers, GRAD_COUNTS, dY, X, dS.cpu(), g, dtype)


@pytest.fixture(scope="module")
def small(env):
    """One random 4-bit case shared by the ABI, determinism and graph tests."""
    bits, tile_p, g, dtype, pair, K, N = 4, 32, 64, F16, False, 320, 256
    return dict(random_case_of(env, bits, tile_p, g, dtype, pair, K, N), bits=bits, g=g, dtype=dtype, K=K, N=N)


def abi_call(env, c, off, dsbuf, guard, E=None, R=None, t2=None, row_weight=None):
    d = env.dev
    E = len(GRAD_COUNTS) if E is None else E
    t2 = c["t2"] if t2 is None else t2
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_scale_grad(
            0 if c["dtype"] == F16 else 1, c["bits"], c["g"], E, c["R"] if R is None else R, c["N"], c["K"], c["Q"].shape[1],
            c["tid"], c["dY"].data_ptr(), c["X"].data_ptr(), off.data_ptr(), c["Q"].data_ptr(), t2.data_ptr(),
            None if row_weight is None else row_weight.data_ptr(), dsbuf[guard:].data_ptr(), env.num_sms,
            torch.cuda.current_stream(d).cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_direct_abi_writes_exactly_dS(env, small):
    """dS in the middle of a canary-filled buffer.  offsets[E] in {R, 2R/3, 0}: every expert's slice is the dense op on its
    clamped range or zeros, every element is written, the canaries around it are intact.  A table of inf / NaN in the empty
    experts leaves their zeros.  Malformed tables (negative entries, entries above R, a decreasing pair) are memory-safe
    by the clamping, and the experts whose range is well-formed keep their bits."""
    c = small
    d, dtype, K, N, g, E = env.dev, c["dtype"], c["K"], c["N"], c["g"], len(GRAD_COUNTS)
    G = K // g
    guard, numel = 4096, E * N * G
    canary = XC.NAN_BITS[dtype]
    dsbuf = torch.empty(guard + numel + guard, dtype=torch.int16, device=d)
    full = offsets_of(GRAD_COUNTS)
    Rs = sum(GRAD_COUNTS)
    t2 = c["t2"].clone()
    t2[0] = float("inf")                                           # experts 0 and 5 have no rows
    t2[5] = float("nan")

    def run(off, **kw):
        dsbuf.fill_(canary)
        assert abi_call(env, c, off.to(d), dsbuf, guard, **kw) == 0
        assert torch.all(dsbuf[:guard] == canary) and torch.all(dsbuf[guard + numel:] == canary)
        out = dsbuf[guard:guard + numel].clone()
        assert not torch.any(out == canary)                        # every element of dS is written
        return out.view(dtype).view(E, N, G)

    def dense(e, r0, r1):
        return env.fa.qgemm_scale_grad(c["dY"][r0:r1], c["X"][r0:r1], c["Q"][e], c["t2"][e], c["bits"], g, c["tid"])

    for zb in (Rs, 2 * Rs // 3, 0):
        off = full.clamp(max=zb)                                   # a proper table whose last entry is zb
        dS = run(off, t2=t2)
        for e in range(E):
            r0, r1 = int(off[e]), int(off[e + 1])
            want = dense(e, r0, r1) if r1 > r0 else torch.zeros(N, G, dtype=dtype, device=d)
            assert torch.equal(bits16(dS[e]), bits16(want)), (zb, e)
    good = run(full)
    assert torch.equal(bits16(good), bits16(c["dS"]))
    weighted = run(full, row_weight=c["rw"])
    assert torch.equal(bits16(weighted), bits16(c["dSw"]))
    # malformed tables: memory safety, and the experts whose own two entries are untouched and ordered keep their bits
    neg = full.clone()
    neg[:3] = torch.tensor([-5, -1, -70])
    above = full.clone()
    above[-3:] = torch.tensor([c["R"] + 1, c["R"] + 1000, 2 ** 31 - 1])
    decreasing = full.clone()
    decreasing[3], decreasing[4] = full[4], full[3]
    for off, kept in ((neg, (3, 4, 5, 6, 7)), (above, (0, 1, 2, 3, 4)), (decreasing, (0, 1, 5, 6, 7))):
        dS = run(off)
        for e in kept:
            assert torch.equal(bits16(dS[e]), bits16(good[e])), (off.tolist(), e)
    dS = run(neg)
    assert torch.all(bits16(dS[:2]) == 0)                          # [clamp(-5), clamp(-1)) and [clamp(-1), clamp(-70)): empty
    dS = run(decreasing)
    assert torch.all(bits16(dS[3]) == 0)                           # a decreasing pair is an empty range
    # R == 0 writes zeros (a memset); E == 0 writes nothing
    dsbuf.fill_(canary)
    assert abi_call(env, c, full.to(d), dsbuf, guard, R=0) == 0
    assert torch.all(dsbuf[:guard] == canary) and torch.all(dsbuf[guard + numel:] == canary)
    assert torch.all(dsbuf[guard:guard + numel] == 0)
    dsbuf.fill_(canary)
    assert abi_call(env, c, full.to(d), dsbuf, guard, E=0) == 0
    assert torch.all(dsbuf == canary)


def test_equal_bits_over_two_calls_and_in_a_graph(env, small):
    """The host reads nothing: a captured launch replayed after `offsets`, dY and X were overwritten in place serves the
    new contents, bit for bit what an eager call on them returns."""
    c = small
    d, E, R = env.dev, len(GRAD_COUNTS), c["R"]
    counts2 = [40, 0, 3, 0, 60, 33, 1, sum(GRAD_COUNTS) - 137]
    assert sum(counts2) == sum(GRAD_COUNTS) and len(counts2) == E and min(counts2) >= 0
    gen = torch.Generator().manual_seed(77)
    dY2 = nan_padded(torch.randn(sum(GRAD_COUNTS), c["N"], generator=gen).to(c["dtype"])).to(d)
    X2 = nan_padded(torch.randn(sum(GRAD_COUNTS), c["K"], generator=gen).to(c["dtype"])).to(d)
    off2 = offsets_of(counts2, d)
    dy, x, off = c["dY"].clone(), c["X"].clone(), c["off"].clone()
    run = lambda a, b, o: env.fa.qgemm_grouped_scale_grad(a, b, o, c["Q"], c["t2"], c["bits"], c["g"], c["tid"], env.num_sms)
    first = run(dy, x, off).clone()
    assert torch.equal(bits16(first), bits16(c["dS"]))
    assert torch.equal(bits16(run(dy, x, off)), bits16(first))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds = run(dy, x, off)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(ds), bits16(first))
    off.copy_(off2)
    dy.copy_(dY2)
    x.copy_(X2)
    ds.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(dY2, X2, off2)
    assert torch.equal(bits16(ds), bits16(eager))
    assert torch.isfinite(eager).all() and not torch.equal(bits16(eager), bits16(first))
    assert torch.all(bits16(eager[1]) == 0) and torch.all(bits16(eager[3]) == 0)


# ---------------------------------------------------------------------------
# autograd, op level
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def op_case(env):
    """Three random 4-bit stacks of a gated MLP (gate, up: K -> F; down: F -> K) and tokens routed at top-2 by moe_route,
    one slot served by no expert."""
    d, dtype, bits, tile_p, g = env.dev, F16, 4, 32, 64
    E, T, k, K, F = 8, 50, 2, 256, 384
    tid = first_template(bits, tile_p)

    def stack(kk, nn, seed):
        parts = [random_code_layer(env, bits, tile_p, dtype, kk, nn, seed + e, pair=(e % 2 == 1)) for e in range(E)]
        Q, t2 = (torch.stack([p[i] for p in parts]) for i in range(2))
        S = (torch.randn(E, nn, kk // g, generator=torch.Generator().manual_seed(seed)) / 8).to(dtype).to(d)
        return Q, S, t2

    gen = torch.Generator().manual_seed(17)
    ids = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)]).to(torch.int32)
    ids[3, 1] = E                                                  # a slot no expert serves
    offsets, rows, row_weight, pos, _ = env.fa.moe_route(ids.to(d), torch.rand(T, k, generator=gen).to(d), E)
    hidden = (torch.randn(T, K, generator=gen) / 4).to(dtype).to(d)
    return dict(E=E, T=T, k=k, K=K, F=F, R=T * k, dtype=dtype, args=(bits, g, tid, env.num_sms), gate=stack(K, F, 9300),
                up=stack(K, F, 9400), down=stack(F, K, 9500), offsets=offsets, rows=rows, pos=pos, rw=row_weight,
                hidden=hidden, gen=gen)


def test_autograd_grouped_learnable_scales(env, op_case):
    c = op_case
    fa, ln, args, d = env.fa, env.ln, c["args"], env.dev
    Q, S, t2 = c["gate"]
    x = c["hidden"].index_select(0, c["rows"].long()).clone()
    dY = torch.randn(c["R"], c["F"], generator=c["gen"]).to(c["dtype"]).to(d)
    x0 = x.clone().requires_grad_()
    y0 = fa.qgemm_grouped(x0, c["offsets"], Q, S, t2, *args)
    y0.backward(dY)
    x1, S1 = x.clone().requires_grad_(), torch.nn.Parameter(S.clone())
    y1 = ln.qgemm_grouped_learnable_scales(x1, c["offsets"], Q, S1, t2, *args)
    assert y1.requires_grad and torch.equal(bits16(y1), bits16(y0))
    y1.backward(dY)
    assert torch.equal(bits16(x1.grad), bits16(x0.grad))
    by_hand = fa.qgemm_grouped_scale_grad(dY, x, c["offsets"], Q, t2, *args)
    assert S1.grad.shape == S.shape and S1.grad.dtype == S.dtype
    assert torch.equal(bits16(S1.grad), bits16(by_hand)) and float(by_hand.abs().max()) > 0
    # the scales alone: no input-gradient launch is needed, the same dS
    S2 = torch.nn.Parameter(S.clone())
    ln.qgemm_grouped_learnable_scales(x, c["offsets"], Q, S2, t2, *args).backward(dY)
    assert torch.equal(bits16(S2.grad), bits16(by_hand))
    # grad mode off: the plain op; a table requiring grad and the public op on learnable scales still raise
    with torch.no_grad():
        y = ln.qgemm_grouped_learnable_scales(x1, c["offsets"], Q, S1, t2, *args)
        assert not y.requires_grad
        served = int(c["offsets"][-1])
        assert torch.equal(bits16(y[:served]), bits16(y0[:served]))
    with pytest.raises(RuntimeError, match="no gradient for table2"):
        ln.qgemm_grouped_learnable_scales(x1, c["offsets"], Q, S1, t2.clone().requires_grad_(), *args)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped: gradients with respect to scales"):
        fa.qgemm_grouped(x1, c["offsets"], Q, S1, t2, *args)
    with pytest.raises(RuntimeError, match="once-differentiable"):
        fa.qgemm_grouped_scale_grad(dY.clone().requires_grad_(), x, c["offsets"], Q, t2, *args)


def test_autograd_grouped_weighted_learnable_scales(env, op_case):
    c = op_case
    fa, ln, args, d = env.fa, env.ln, c["args"], env.dev
    Q, S, t2 = c["down"]
    h = (torch.randn(c["R"], c["F"], generator=c["gen"]) / 4).to(c["dtype"]).to(d)
    h[-1] = float("nan")                                           # the row no expert serves may hold anything
    rw = c["rw"]
    dY = torch.randn(c["R"], c["K"], generator=c["gen"]).to(c["dtype"]).to(d)
    by_hand = fa.qgemm_grouped_scale_grad(dY, h, c["offsets"], Q, t2, *args, row_weight=rw)
    assert torch.isfinite(by_hand).all() and float(by_hand.abs().max()) > 0
    for rw_grad in (True, False):                                  # the plain op's two backward paths
        h0, rw0 = h.clone().requires_grad_(), rw.clone().requires_grad_(rw_grad)
        y0 = fa.qgemm_grouped_weighted(h0, c["offsets"], Q, S, t2, rw0, *args)
        y0.backward(dY)
        h1, rw1, S1 = h.clone().requires_grad_(), rw.clone().requires_grad_(rw_grad), torch.nn.Parameter(S.clone())
        y1 = ln.qgemm_grouped_weighted_learnable_scales(h1, c["offsets"], Q, S1, t2, rw1, *args)
        assert torch.equal(bits16(y1), bits16(y0))
        y1.backward(dY)
        assert torch.equal(bits16(h1.grad), bits16(h0.grad))
        if rw_grad:
            assert torch.equal(rw1.grad, rw0.grad)
        else:
            assert rw1.grad is None
        assert torch.equal(bits16(S1.grad), bits16(by_hand))
    S2 = torch.nn.Parameter(S.clone())
    ln.qgemm_grouped_weighted_learnable_scales(h, c["offsets"], Q, S2, t2, rw, *args).backward(dY)
    assert torch.equal(bits16(S2.grad), bits16(by_hand))
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_weighted: gradients with respect to scales"):
        fa.qgemm_grouped_weighted(h, c["offsets"], Q, S2, t2, rw, *args)


@pytest.mark.parametrize("native", [False, True])
def test_autograd_grouped_glu_learnable_scales(env, op_case, native):
    """dS_gate = scale_grad(dg, x_sorted), dS_up = scale_grad(du, x_sorted): x_sorted, dg and du as the op's backward forms
    them."""
    c = op_case
    fa, ln, args, d, dtype = env.fa, env.ln, c["args"], env.dev, c["dtype"]
    (Qg, Sg, tg), (Qu, Su, tu) = c["gate"], c["up"]
    hidden = c["hidden"]
    kw = dict(rows=c["rows"], pos=c["pos"] if native else None)
    dH = (torch.randn(c["R"], c["F"], generator=c["gen"]) / 8).to(dtype).to(d)
    x0 = hidden.clone().requires_grad_()
    y0 = fa.qgemm_grouped_glu(x0, c["offsets"], Qg, Sg, tg, Qu, Su, tu, *args, **kw)
    y0.backward(dH)
    x1, Sg1, Su1 = hidden.clone().requires_grad_(), torch.nn.Parameter(Sg.clone()), torch.nn.Parameter(Su.clone())
    y1 = ln.qgemm_grouped_glu_learnable_scales(x1, c["offsets"], Qg, Sg1, tg, Qu, Su1, tu, *args, **kw)
    assert torch.equal(bits16(y1), bits16(y0))
    y1.backward(dH)
    assert torch.equal(bits16(x1.grad), bits16(x0.grad))
    x = hidden.index_select(0, c["rows"].long())
    g = fa.qgemm_grouped(x, c["offsets"], Qg, Sg, tg, *args).float()
    u = fa.qgemm_grouped(x, c["offsets"], Qu, Su, tu, *args).float()
    sig = torch.sigmoid(g)
    dg = (dH.float() * u * sig * (1 + g * (1 - sig))).to(dtype)
    du = (dH.float() * (g * sig)).to(dtype)
    dSg = fa.qgemm_grouped_scale_grad(dg, x, c["offsets"], Qg, tg, *args)
    dSu = fa.qgemm_grouped_scale_grad(du, x, c["offsets"], Qu, tu, *args)
    assert torch.isfinite(dSg).all() and torch.isfinite(dSu).all() and float(dSg.abs().max()) > 0 and float(dSu.abs().max()) > 0
    assert torch.equal(bits16(Sg1.grad), bits16(dSg))
    assert torch.equal(bits16(Su1.grad), bits16(dSu))
    # one stack's scales alone, the input without grad
    Su2 = torch.nn.Parameter(Su.clone())
    ln.qgemm_grouped_glu_learnable_scales(hidden, c["offsets"], Qg, Sg, tg, Qu, Su2, tu, *args, **kw).backward(dH)
    assert torch.equal(bits16(Su2.grad), bits16(dSu))
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_glu: gradients with respect to scales"):
        fa.qgemm_grouped_glu(hidden, c["offsets"], Qg, Sg, tg, Qu, Su2, tu, *args, **kw)


# ---------------------------------------------------------------------------
# one autograd function per grouped op, shared by the op and its learnable entry
# ---------------------------------------------------------------------------

def through_autograd(env, c, form, learnable, scales_grad):
    """One forward and backward of a grouped op (`learnable`: through its *_learnable_scales entry) with the input - and the
    row weight - requiring grad: (out, dX, d row_weight or None, [dS_gate, dS_up] or None, whether the graph saved the input)."""
    (Qg, Sg, tg), (Qu, Su, tu) = c["gate"], c["up"]
    if scales_grad:
        Sg, Su = torch.nn.Parameter(Sg.clone()), torch.nn.Parameter(Su.clone())
    op = lambda name: getattr(env.ln, name + "_learnable_scales") if learnable else getattr(env.fa, name)
    rw = None
    if form == "plain":
        x = c["x_sorted"].clone().requires_grad_()
        y = op("qgemm_grouped")(x, c["off"], Qg, Sg, tg, *c["args"])
    elif form == "weighted":
        x, rw = c["x_sorted"].clone().requires_grad_(), c["rw"].clone().requires_grad_()
        y = op("qgemm_grouped_weighted")(x, c["off"], Qg, Sg, tg, rw, *c["args"])
    else:
        rows, pos = c["rows"] if "rows" in form else None, c["pos"] if "pos" in form else None
        x = (c["x_sorted"] if rows is None else c["tokens"]).clone().requires_grad_()
        y = op("qgemm_grouped_glu")(x, c["off"], Qg, Sg, tg, Qu, Su, tu, *c["args"], rows=rows, pos=pos)
    saves_input = any(t.data_ptr() == x.data_ptr() for t in y.grad_fn.saved_tensors)
    y.backward(c["dY"])
    return y.detach(), x.grad, None if rw is None else rw.grad, [Sg.grad, Su.grad] if scales_grad else None, saves_input


@pytest.mark.parametrize("form", ["plain", "weighted", "glu", "glu_rows", "glu_rows_pos"])
def test_op_and_learnable_entry_are_one_function(env, tiny, form):
    """The op and its learnable entry run one autograd function: equal bits for the output, dX and d row_weight whether or
    not the scales train, dS the direct scale-gradient call on the tensors the backward forms, and `input` saved only for dS."""
    c, fa = tiny, env.fa
    (Qg, Sg, tg), (Qu, Su, tu) = c["gate"], c["up"]
    y0, dx0, drw0, _, saves_input = through_autograd(env, c, form, learnable=False, scales_grad=False)
    assert torch.isfinite(dx0).all() and float(dx0.abs().max()) > 0 and float(y0.abs().max()) > 0
    assert (drw0 is not None) == (form == "weighted")
    for scales_grad in (False, True):
        y, dx, drw, dS, _ = through_autograd(env, c, form, learnable=True, scales_grad=scales_grad)
        assert torch.equal(bits16(y), bits16(y0)) and torch.equal(bits16(dx), bits16(dx0))
        if form == "weighted":
            assert torch.equal(drw.view(torch.int32), drw0.view(torch.int32)) and float(drw0.abs().max()) > 0
        else:
            assert drw is None
    x, dY = c["x_sorted"], c["dY"]
    if form == "plain":
        want = [fa.qgemm_grouped_scale_grad(dY, x, c["off"], Qg, tg, *c["args"]), None]
        assert not saves_input                                       # only the input requires grad: dS alone reads it
    elif form == "weighted":
        want = [fa.qgemm_grouped_scale_grad(dY, x, c["off"], Qg, tg, *c["args"], row_weight=c["rw"]), None]
    else:
        g = fa.qgemm_grouped(x, c["off"], Qg, Sg, tg, *c["args"]).float()
        u = fa.qgemm_grouped(x, c["off"], Qu, Su, tu, *c["args"]).float()
        sig = torch.sigmoid(g)
        dg = (dY.float() * u * sig * (1 + g * (1 - sig))).to(x.dtype)
        du = (dY.float() * (g * sig)).to(x.dtype)
        want = [fa.qgemm_grouped_scale_grad(dg, x, c["off"], Qg, tg, *c["args"]),
                fa.qgemm_grouped_scale_grad(du, x, c["off"], Qu, tu, *c["args"])]
    for got, w in zip(dS, want):
        if w is None:
            assert got is None                                       # (the up stack plays no part in this form)
        else:
            assert got.shape == Sg.shape and torch.equal(bits16(got), bits16(w))
            assert torch.isfinite(w).all() and float(w[0].abs().max()) > 0 and float(w[2].abs().max()) > 0
            assert not w[1].any()                                    # the empty expert: zeros


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------

def make_experts_case(env, dtype):
    """E = 4 experts from FluteLinear.from_codes (4-bit, g = 64, K = 256, F = 512), 37 tokens; expert 2 is never chosen,
    token 0 is routed only to ids outside [0, E), token 5 has one such slot.  `lut`: every layer's lookups [N, K] in fp64
    (the dense weight with unit scales)."""
    d = env.dev
    E, K, F, T, bits, g = 4, 256, 512, 37, 4, 64
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(41)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, bits=bits, g=g, tid=tid, dtype=dtype)
    c["layers"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)], [linear(F, K) for _ in range(E)])
    lut = lambda m: env.fa.dequantize(m.weight, torch.ones_like(m.scales), m.tables2, bits, g, tid).double()
    c["lut"] = [[lut(m) for m in ms] for ms in c["layers"]]
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["dOut"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["routing"] = {}
    for k in (2, 3):
        chosen = torch.tensor([0, 1, 3])
        ids = torch.stack([chosen[torch.randperm(3, generator=gen)[:k]] for _ in range(T)])
        ids[0] = torch.tensor([E, -1, E + 5][:k])
        ids[5, 1] = E
        weights = torch.rand(T, k, generator=gen)
        c["routing"][k] = (ids.to(d), (weights / weights.sum(1, keepdim=True)).to(dtype).to(d))
    c["refs"] = {}
    return c


@pytest.fixture(scope="module")
def experts_case(env):
    return make_experts_case(env, F16)


def learnable_loop(env, c):
    """The yardstick's layers: every expert's FluteLinear as a LearnableScalesFluteLinear (dense learnable layers in T)."""
    return [[env.ln.LearnableScalesFluteLinear(m) for m in ms] for ms in c["layers"]]


def loop_grads(loop):
    """The stacked scales.grad of the loop's layers, zeros for an expert that saw no row."""
    return [torch.stack([m.scales.grad if m.scales.grad is not None else torch.zeros_like(m.scales) for m in ms])
            for ms in loop]


def reference_scale_grads(env, c, k):
    """(fp64 gradients, the yardstick's gradients in T) of the three stacks' scales for dOut, computed once per k."""
    if k not in c["refs"]:
        ids, weights = c["routing"][k]
        S64 = scale_leaves(c)
        restated_experts(c, c["hidden"].double(), ids, weights.double(), dense_project(c, S64)).backward(c["dOut"].double())
        loop = learnable_loop(env, c)
        restated_experts(c, c["hidden"], ids, weights, lambda e, which, x: loop[which][e](x)).backward(c["dOut"])
        c["refs"][k] = ([s.grad for s in S64], loop_grads(loop))
    return c["refs"][k]


NAMES = ("gate", "up", "down")


def before_combine(env, experts, hidden, ids, weights):
    """(h, y) of a torch-routed FluteExperts - the rows an expert serves of the GLU's result and of the down projection's -
    through the launches its forward makes, before index_add_ sums a token's rows in an order it does not promise."""
    k = ids.shape[1]
    perm, offsets = env.moe.sort_by_expert(ids, experts.num_experts)
    token = perm // k
    gate, up, down = experts.gate, experts.up, experts.down
    if experts.fused:
        glu, weighted = experts._fused_ops()
        h = glu(hidden, offsets, gate.weight, gate.scales, gate.tables2, up.weight, up.scales, up.tables2, gate.num_bits,
                gate.group_size, gate.template_id, gate.num_sms, rows=token.to(torch.int32))
        y = weighted(h, offsets, down.weight, down.scales, down.tables2, weights.reshape(-1)[perm].float(), down.num_bits,
                     down.group_size, down.template_id, down.num_sms)
    else:
        x = hidden[token]
        h = torch.nn.functional.silu(gate(x, offsets)) * up(x, offsets)
        y = down(h, offsets)
    served = int(offsets[-1])
    return h[:served], y[:served]


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("fused,native", [(False, False), (True, False), (False, True), (True, True)])
def test_flute_experts_scale_grads(env, experts_case, fused, native, k):
    """The three scales.grad of a learnable FluteExperts in every configuration against fp64 autograd of the restated
    block on dense weights L * S with S an fp64 leaf, max-abs error relative to max|ref|; the yardstick is the per-expert
    loop over LearnableScalesFluteLinear in T and the bound twice its error (the operation orders differ, not the
    precision).  The figures are printed (-s) and tabulated in DESIGN.md 3.3i."""
    c = experts_case
    ids, weights = c["routing"][k]
    ref, yard = reference_scale_grads(env, c, k)
    experts = env.moe.FluteExperts.from_linears(*c["layers"], fused=fused, native_routing=native)
    with torch.no_grad():
        frozen_out = experts(c["hidden"], ids, weights)
        frozen_hy = None if native else before_combine(env, experts, c["hidden"], ids, weights)
    params = env.moe.make_experts_learnable(experts)
    assert len(params) == 3
    with torch.no_grad():                                          # grad mode off: the inference launches, the frozen bits
        out = experts(c["hidden"], ids, weights)
        hy = None if native else before_combine(env, experts, c["hidden"], ids, weights)
    assert not out.requires_grad
    if native or k == 2:                                           # (index_add_ at top-3: the order of a token's addends is free)
        assert torch.equal(bits16(out), bits16(frozen_out))
    h, w = c["hidden"].clone().requires_grad_(), weights.clone().requires_grad_()
    out = experts(h, ids, w)
    if native or k == 2:
        assert torch.equal(bits16(out), bits16(frozen_out))        # recording a graph does not change the forward
    if not native:                                                 # ... and at top-3 too, on the launches' results before index_add_
        recorded = before_combine(env, experts, h, ids, w)
        assert recorded[1].requires_grad
        for got in (hy, recorded):
            assert all(torch.equal(bits16(a), bits16(b)) and a.numel() > 0 for a, b in zip(got, frozen_hy))
    out.backward(c["dOut"])
    assert h.grad is not None and w.grad is not None
    for name, p, r, y in zip(NAMES, params, ref, yard):
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all()
        err, yerr = max_rel_err(p.grad, r), max_rel_err(y, r)
        print("FluteExperts scales.grad fused=%d native=%d k=%d %s: %.3e (yardstick %.3e)" % (fused, native, k, name, err, yerr))
        assert yerr > 0
        assert err <= 2 * yerr, (name, err, yerr)
        assert torch.all(p.grad[2] == 0) and torch.all(r[2] == 0)  # an expert no token chose


def test_sparse_moe_block_scale_grads(env, experts_case):
    """The same through FluteSparseMoeBlock with a group-limited sigmoid router (n_group = 2, topk_group = 1, renormalised,
    a bias, scale 2.5) on the fused, natively routed experts: against fp64 autograd of the whole block on dense weights
    L * S (the kernel's ids held fixed; the keys are separated by more than 2^-8, asserted), the bound twice the error of
    the whole block restated in T over LearnableScalesFluteLinear."""
    c = experts_case
    d, dtype, E, K, T = env.dev, c["dtype"], c["E"], c["K"], c["T"]
    k, n_group, topk_group, scoring, renorm, scale = 2, 2, 1, "sigmoid", True, 2.5
    gen = torch.Generator().manual_seed(53)
    bias = (torch.rand(E, generator=gen) * 0.2).to(d)
    for attempt in range(20):
        router = (torch.randn(E, K, generator=gen) * 0.08).to(dtype).to(d)
        logits = torch.nn.functional.linear(c["hidden"], router)
        keys = torch.sigmoid(logits.float()) + bias
        gkeys = keys.view(T, n_group, -1).max(dim=2).values.sort(dim=1, descending=True).values
        gap = gkeys[:, topk_group - 1] - gkeys[:, topk_group]
        if float(gap.min()) > 2.0 ** -8:
            break
    assert float(gap.min()) > 2.0 ** -8, float(gap.min())
    experts = env.moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
    block = env.moe.FluteSparseMoeBlock(router.clone(), experts, top_k=k, scoring=scoring, renormalize=renorm, bias=bias,
                                        scale=scale, n_group=n_group, topk_group=topk_group)
    with torch.no_grad():
        frozen_out = block(c["hidden"])
        ids, _ = env.fa.moe_gate_limited(logits, k, n_group, topk_group, scoring, renorm, bias, scale)
    params = env.moe.make_experts_learnable(block)
    assert len(params) == 3
    out = block(c["hidden"])
    assert out.requires_grad and torch.equal(bits16(out), bits16(frozen_out))
    out.backward(c["dOut"])
    S64 = scale_leaves(c)
    hd, rd = c["hidden"].double(), router.double()
    restated_experts(c, hd, ids, gate_formula(hd @ rd.T, ids, scoring, renorm, scale), dense_project(c, S64)) \
        .backward(c["dOut"].double())
    loop = learnable_loop(env, c)
    wT = gate_formula(torch.nn.functional.linear(c["hidden"], router).float(), ids, scoring, renorm, scale).to(dtype)
    restated_experts(c, c["hidden"], ids, wT, lambda e, which, x: loop[which][e](x)).backward(c["dOut"])
    for name, p, s, y in zip(NAMES, params, S64, loop_grads(loop)):
        err, yerr = max_rel_err(p.grad, s.grad), max_rel_err(y, s.grad)
        print("FluteSparseMoeBlock scales.grad %s: %.3e (yardstick %.3e)" % (name, err, yerr))
        assert yerr > 0
        assert err <= 2 * yerr, (name, err, yerr)


def test_train_experts_scales(env):
    """A dozen Adam steps on the experts' scales of the tiny block toward a teacher with perturbed scales: the loss falls
    below 0.8 of its start, every buffer but the scales keeps its bits, and the frozen block is plain GroupedFluteLinear
    stacks with the unchanged state-dict keys and the bits of the learnable forward under no_grad.  The block is built
    in bf16, as test_scale_grad_gpu's training run: Adam keeps its moments in the parameters' type, and fp16 holds
    neither its epsilon nor the square of a small gradient."""
    c = make_experts_case(env, BF16)
    d, dtype = env.dev, c["dtype"]
    moe = env.moe
    torch.manual_seed(0)
    ids, weights = c["routing"][2]
    student = moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
    teacher = moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
    with torch.no_grad():
        for m in (teacher.gate, teacher.up, teacher.down):
            m.scales.copy_((m.scales.float() * (1 + torch.randn_like(m.scales.float()) / 8)).to(dtype))
        target = teacher(c["hidden"], ids, weights).float()
    keys = list(student.state_dict())
    before = {k: v.clone() for k, v in student.state_dict().items() if not k.endswith("scales")}
    params = moe.make_experts_learnable(student)
    assert len(params) == 3 and all(type(m) is moe.LearnableGroupedFluteLinear for m in (student.gate, student.up, student.down))
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = []
    for _ in range(12):
        loss = (student(c["hidden"], ids, weights).float() - target).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("expert scales training: loss %.4e -> %.4e" % (losses[0], losses[-1]))
    assert losses[-1] < 0.8 * losses[0], losses
    for name, v in student.state_dict().items():
        if name in before:
            assert torch.equal(v, before[name]), name
    learned = [p.detach().clone() for p in params]
    with torch.no_grad():
        learnable_out = student(c["hidden"], ids, weights)
    moe.freeze_experts(student)
    stacks = (student.gate, student.up, student.down)
    assert all(type(m) is moe.GroupedFluteLinear for m in stacks)
    assert all(torch.equal(m.scales, s) for m, s in zip(stacks, learned))
    assert list(student.state_dict()) == keys and not list(student.parameters())
    out = student(c["hidden"], ids, weights)
    assert not out.requires_grad and torch.equal(bits16(out), bits16(learnable_out))
