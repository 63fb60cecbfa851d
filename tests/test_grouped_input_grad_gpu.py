"""flute_amd.qgemm_grouped_input_grad / flute_qgemm_grouped_input_grad on the GPU, and the backward of the expert path
built on it: dX = dY @ W_e per expert in one launch over the packed stacks, from row offsets the host never reads.

Exact inputs (tests/exact_cases) must come back bit for bit per expert, in the single, the row-weighted and the pair
form; a direct ABI call must write every row of dX - products below offsets[E], zeros from there on - and nothing else,
also on malformed tables; random data must stay within the componentwise bound of the documented arithmetic with
contraction length N; two calls and a graph replay on other contents give equal bits.  On top: every grouped op's
`input.grad` is bit for bit the composition its docstring names, and `FluteExperts` / `FluteSparseMoeBlock` backpropagate
to the hidden states, the routing weights and the router as closely to fp64 as their yardsticks do."""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import (counts_of, exact_layers, exact_matrix, exact_seed, gate_formula, random_stack,
                                 restated_experts, stack_exact)
from tests.support import bits16, env, first_template, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16


def row_block(env):
    return env.fa.ops.GROUPED_INPUT_GRAD_ROW_BLOCK


def exact_grad(dY, layer):
    """(R, A) = (dY @ W_exact^T, |dY| @ |W_exact|^T) in fp64: [rows, K]."""
    W = layer.w_exact()                                          # [K, N]: W_exact^T in the docstring's sense is [N, K]
    d = dY.double()
    return d @ W.T, d.abs() @ W.abs().T


def weight_premise(layer):
    w = layer.w_exact(0, min(layer.N, 256))
    assert torch.equal(w.to(layer.dtype).double(), w) and torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16


def check_exact_grad(layers, counts, dY, dX, dY2=None, layers2=None, row_weight=None):
    """Per expert: the premise (integer dY in [-4, 4], exact weights, sum |dY| |w| < 2^21 - then every partial sum in any
    order is exact in fp32 and round_T(R) is the only allowed answer) and dX[r0:r1] == round_T(w_r R) by value."""
    off = offsets_of(counts).tolist()
    dtype = layers[0].dtype
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        rows = dY[r0:r1]
        assert torch.equal(rows.double(), rows.double().round()) and rows.double().abs().max() <= 4
        weight_premise(lay)
        R, A = exact_grad(rows, lay)
        if dY2 is not None:
            weight_premise(layers2[e])
            R2, A2 = exact_grad(dY2[r0:r1], layers2[e])
            R, A = R + R2, A + A2
        assert float(A.max()) < XC.EXACT_SUM_LIMIT, ("sum |dY w| reaches 2^21", float(A.max()))
        if row_weight is not None:
            R = R * row_weight[r0:r1].double()[:, None]          # a power of two (or zero) times an exact fp32 sum: exact
        assert torch.isfinite(R.to(dtype)).all()
        assert XC.exact_equal(dX[r0:r1], R, dtype), (e, lay)


def grad_matrix():
    """bits 4 / 3 / 2 x TileP 32 / 64 (3 bits: 32) x the four (g, dtype, pair) rows of grouped_cases.exact_matrix; N = 3
    column blocks (>= 6 chunks of the kernel's 64 columns), K = 5 max(64, g): the last 128-k slab is half for g <= 64."""
    out = []
    for bits, tile_p, g, dtype, _, _, pair in exact_matrix():
        out.append((bits, tile_p, g, dtype, 5 * max(64, g), 3 * XC.cols_per_block(bits, tile_p), pair))
    return out


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,pair", grad_matrix())
def test_exact_per_expert(env, bits, tile_p, g, dtype, K, N, pair):
    counts = counts_of(row_block(env))
    layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, len(counts), exact_seed(bits, tile_p, g) + 300)
    Q, S, t2, tid = stack_exact(env, layers)
    R = sum(counts)
    dY = XC.make_x(R, N, exact_seed(bits, tile_p, g) + 377, dtype, witness=False)
    dX = env.fa.qgemm_grouped_input_grad(dY.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, bits, g, tid)
    assert dX.shape == (R, K) and dX.dtype == dtype
    check_exact_grad(layers, counts, dY, dX.cpu())


@pytest.fixture(scope="module")
def small_exact(env):
    """Two exact 4-bit stacks and two integer dY shared by the pair, row-weight, ABI, determinism and graph tests."""
    bits, tile_p, g, dtype, K, N = 4, 32, 64, F16, 320, 3 * 128
    counts = counts_of(row_block(env))
    layers = exact_layers(bits, tile_p, g, dtype, K, N, False, len(counts), 9100)
    layers2 = exact_layers(bits, tile_p, g, dtype, K, N, False, len(counts), 9200)
    Q, S, t2, tid = stack_exact(env, layers)
    Q2, S2, t22, _ = stack_exact(env, layers2)
    R = sum(counts)
    dY = XC.make_x(R, N, 9101, dtype, witness=False)
    dY2 = XC.make_x(R, N, 9201, dtype, witness=False)
    return dict(bits=bits, g=g, dtype=dtype, K=K, N=N, counts=counts, R=R, layers=layers, layers2=layers2, tid=tid,
                stack=(Q, S, t2), stack2=(Q2, S2, t22), dY=dY, dY2=dY2)


def test_pair_form_exact(env, small_exact):
    """Two different stacks and two dY against the fp64 sum of both products; 128 N < 2^21."""
    c = small_exact
    assert 128 * c["N"] < XC.EXACT_SUM_LIMIT
    Q2, S2, t22 = c["stack2"]
    dX = env.fa.qgemm_grouped_input_grad(c["dY"].to(env.dev), offsets_of(c["counts"], env.dev), *c["stack"], c["bits"], c["g"],
                                         c["tid"], grad_output2=c["dY2"].to(env.dev), weight2=Q2, scales2=S2, table22=t22)
    check_exact_grad(c["layers"], c["counts"], c["dY"], dX.cpu(), dY2=c["dY2"], layers2=c["layers2"])
    single = env.fa.qgemm_grouped_input_grad(c["dY"].to(env.dev), offsets_of(c["counts"], env.dev), *c["stack"], c["bits"],
                                             c["g"], c["tid"])
    assert not torch.equal(bits16(dX), bits16(single))


def test_row_weight_exact(env, small_exact):
    c = small_exact
    gen = torch.Generator().manual_seed(3)
    choice = torch.tensor([0.25, -0.25, 1.0, -1.0, 2.0, 0.0])
    rw = choice[torch.randint(0, len(choice), (c["R"],), generator=gen)]
    dX = env.fa.qgemm_grouped_input_grad(c["dY"].to(env.dev), offsets_of(c["counts"], env.dev), *c["stack"], c["bits"], c["g"],
                                         c["tid"], row_weight=rw.to(env.dev))
    check_exact_grad(c["layers"], c["counts"], c["dY"], dX.cpu(), row_weight=rw)


def abi_call(env, c, off, ybuf, xbuf, guard, pair=False, row_weight=None):
    d = env.dev
    Q, S, t2 = c["stack"]
    second = (None,) * 4
    if pair:
        Q2, S2, t22 = c["stack2"]
        second = (c["dY2_dev"].data_ptr(), Q2.data_ptr(), S2.data_ptr(), t22.data_ptr())
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_input_grad(
            0 if c["dtype"] == F16 else 1, c["bits"], c["g"], len(c["counts"]), c["R"], c["N"], c["K"], Q.shape[1], c["tid"],
            ybuf[guard:].data_ptr(), off.data_ptr(), Q.data_ptr(), S.data_ptr(), t2.data_ptr(),
            None if row_weight is None else row_weight.data_ptr(), *second, xbuf[guard:].data_ptr(), env.num_sms,
            torch.cuda.current_stream(d).cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_direct_abi_writes_exactly_what_it_says(env, small_exact):
    """dX and dY in the middle of canary-padded buffers, dX pre-filled with NaN bits.  offsets[E] in {R, 2R/3, 0}: the rows
    below are the products, the rows from offsets[E] on are zeros, the canaries are intact.  Malformed tables (negative
    entries, entries above R, a decreasing pair) are memory-safe by the clamping: canaries intact, nothing faults."""
    c = dict(small_exact)
    d, dtype, K, N, R, E = env.dev, c["dtype"], c["K"], c["N"], c["R"], len(c["counts"])
    guard = 16
    canary = XC.NAN_BITS[dtype]
    c["dY2_dev"] = c["dY2"].to(d)
    ybuf = torch.full((guard + R + guard, N), 3.0, dtype=dtype, device=d)
    ybuf[guard:guard + R] = c["dY"].to(d)
    xbuf = torch.empty((guard + R + guard, K), dtype=torch.int16, device=d)
    full = offsets_of(c["counts"])

    def run(off, **kw):
        xbuf.fill_(canary)
        assert abi_call(env, c, off.to(d), ybuf, xbuf, guard, **kw) == 0
        assert torch.all(xbuf[:guard] == canary) and torch.all(xbuf[guard + R:] == canary)
        return xbuf[guard:guard + R].view(dtype).cpu()

    for zb in (R, 2 * R // 3, 0):
        off = full.clamp(max=zb)                                   # a proper table whose last entry is zb
        counts = (off[1:] - off[:-1]).tolist()
        dX = run(off)
        check_exact_grad(c["layers"], counts, c["dY"], dX)
        assert torch.all(bits16(dX[zb:]) == 0), zb                 # every row is written: zeros where no expert serves
        assert not torch.any(bits16(dX) == canary)
    dX = run(full.clamp(max=2 * R // 3), pair=True)
    assert torch.all(bits16(dX[2 * R // 3:]) == 0) and not torch.any(bits16(dX) == canary)
    # malformed tables: only memory safety is promised
    neg = full.clone()
    neg[:3] = torch.tensor([-5, -1, -70])
    above = full.clone()
    above[-3:] = torch.tensor([R + 1, R + 1000, 2 ** 31 - 1])
    decreasing = full.clone()
    decreasing[3], decreasing[4] = full[4], full[3]
    for off in (neg, above, decreasing):
        run(off)
        run(off, pair=True)
    # R == 0 enqueues nothing; E == 0 writes zeros
    xbuf.fill_(canary)
    assert abi_call(env, dict(c, R=0), full.to(d), ybuf, xbuf, guard) == 0
    assert torch.all(xbuf == canary)
    assert abi_call(env, dict(c, counts=[]), full.to(d), ybuf, xbuf, guard) == 0
    assert torch.all(xbuf[:guard] == canary) and torch.all(xbuf[guard + R:] == canary) and torch.all(xbuf[guard:guard + R] == 0)


@pytest.mark.parametrize("bits,tile_p,g,dtype", [(4, 32, 64, F16), (3, 32, 32, BF16), (2, 64, 64, BF16)])
def test_random_componentwise(env, bits, tile_p, g, dtype):
    """Random codes, scales and tables against the fp64 product with the exact lut * s weight: the gamma bound of an fp32
    sum of N terms over weights rounded once to T, plus the one rounding of the output (XC.assert_componentwise with
    contraction length N)."""
    counts = [7, 0, row_block(env) + 12]
    K, N = 448, 3 * XC.cols_per_block(bits, tile_p)
    Q, S, t2, Ws = random_stack(env, bits, tile_p, g, dtype, K, N, len(counts), seed=bits * 100 + 31)
    gen = torch.Generator().manual_seed(6)
    dY = torch.randn(sum(counts), N, generator=gen).to(dtype)
    off = offsets_of(counts)
    dX = env.fa.qgemm_grouped_input_grad(dY.to(env.dev), off.to(env.dev), Q, S, t2, bits, g,
                                         first_template(bits, tile_p)).cpu()
    for e, W in enumerate(Ws):                                    # W [K, N]
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            XC.assert_componentwise(dX[r0:r1], dY[r0:r1], W.T, N, dtype, what=(bits, tile_p, g, dtype, e))


def test_equal_bits_over_two_calls_and_in_a_graph(env, small_exact):
    """The host reads nothing: a captured launch replayed after `offsets` and dY were overwritten in place serves the new
    contents, bit for bit what an eager call on them returns."""
    c = small_exact
    R, E = c["R"], len(c["counts"])
    counts2 = [40, 0, 3, 0, R - 40 - 3 - 2 * row_block(env) - 1, row_block(env), 1, row_block(env)]
    assert sum(counts2) == R and len(counts2) == E and min(counts2) >= 0
    dY2 = XC.make_x(R, c["N"], 9102, c["dtype"], witness=False).to(env.dev)
    off2 = offsets_of(counts2, env.dev)
    dy = c["dY"].to(env.dev).clone()
    off = offsets_of(c["counts"], env.dev)
    run = lambda a, o: env.fa.qgemm_grouped_input_grad(a, o, *c["stack"], c["bits"], c["g"], c["tid"], env.num_sms)
    first = run(dy, off).clone()
    assert torch.equal(bits16(run(dy, off)), bits16(first))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dx = run(dy, off)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(dx), bits16(first))
    off.copy_(off2)
    dy.copy_(dY2)
    dx.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(dY2, off2)
    assert torch.equal(bits16(dx), bits16(eager))
    check_exact_grad(c["layers"], counts2, dY2.cpu(), dx.cpu())
    assert not torch.equal(bits16(eager), bits16(first))


# ---------------------------------------------------------------------------
# autograd, op level
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def op_case(env, small_exact):
    """The exact stacks as a gated MLP's first half: tokens [T, K] -> sorted rows through moe_route at top-2."""
    c = small_exact
    d = env.dev
    E, T, k = len(c["counts"]), 50, 2
    gen = torch.Generator().manual_seed(17)
    ids = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)]).to(torch.int32)
    ids[3, 1] = E                                                  # a slot no expert serves
    offsets, rows, _, pos, _ = env.fa.moe_route(ids.to(d), None, E)
    hidden = XC.make_x(T, c["K"], 18, c["dtype"], witness=False).to(d)
    return dict(c, E=E, T=T, k=k, offsets=offsets, rows=rows, pos=pos, hidden=hidden)


def test_autograd_qgemm_grouped(env, op_case):
    c = op_case
    fa, args = env.fa, (c["bits"], c["g"], c["tid"], env.num_sms)
    R = c["T"] * c["k"]
    x = c["hidden"].index_select(0, c["rows"].long()).clone()
    plain = fa.qgemm_grouped(x, c["offsets"], *c["stack"], *args)
    xg = x.clone().requires_grad_()
    y = fa.qgemm_grouped(xg, c["offsets"], *c["stack"], *args)
    served = int(c["offsets"][-1])
    assert y.requires_grad and served == R - 1
    assert torch.equal(bits16(y[:served]), bits16(plain[:served]))           # (the last row is served by no expert)
    dY = XC.make_x(R, c["N"], 19, c["dtype"], witness=False).to(env.dev)
    y.backward(dY)
    by_hand = fa.qgemm_grouped_input_grad(dY, c["offsets"], *c["stack"], *args)
    assert torch.equal(bits16(xg.grad), bits16(by_hand))
    assert torch.all(xg.grad[served:] == 0)
    # the stacks are frozen: scales that require grad raise the documented message; so does a second differentiation
    Q, S, t2 = c["stack"]
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped: gradients with respect to scales, table or table2"):
        fa.qgemm_grouped(xg, c["offsets"], Q, S.clone().requires_grad_(), t2, *args)
    xh = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(fa.qgemm_grouped(xh, c["offsets"], *c["stack"], *args), xh, dY, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    with torch.no_grad():                                          # grad mode off: the plain path
        assert not fa.qgemm_grouped(xg, c["offsets"], *c["stack"], *args).requires_grad


def test_autograd_qgemm_grouped_weighted(env, op_case):
    """row_weight requiring grad: dH' = input_grad(dY), d row_weight[r] = sum_k dH'[r, k] h[r, k] in fp32 (zero from
    offsets[E] on), dH = round_T(row_weight dH'); without: the weight rides in the kernel's epilogue."""
    c = op_case
    fa, args, d = env.fa, (c["bits"], c["g"], c["tid"], env.num_sms), env.dev
    R = c["T"] * c["k"]
    h = c["hidden"].index_select(0, c["rows"].long()).clone()
    h[-1] = float("nan")                                           # the row no expert serves may hold anything
    gen = torch.Generator().manual_seed(23)
    rw = torch.tensor([0.25, -0.5, 1.0, 2.0])[torch.randint(0, 4, (R,), generator=gen)].to(d)
    dY = XC.make_x(R, c["N"], 24, c["dtype"], witness=False).to(d)
    plain = fa.qgemm_grouped_weighted(h, c["offsets"], *c["stack"], rw, *args)
    hg, rwg = h.clone().requires_grad_(), rw.clone().requires_grad_()
    y = fa.qgemm_grouped_weighted(hg, c["offsets"], *c["stack"], rwg, *args)
    assert torch.equal(bits16(y), bits16(plain))
    y.backward(dY)
    dHp = fa.qgemm_grouped_input_grad(dY, c["offsets"], *c["stack"], *args).float()
    served = torch.arange(R, device=d) < c["offsets"][-1]
    d_rw = torch.where(served, (dHp * h.float()).sum(dim=1), torch.zeros((), device=d))
    assert torch.equal(rwg.grad, d_rw) and rwg.grad.dtype == torch.float32 and float(rwg.grad[-1]) == 0
    assert torch.equal(bits16(hg.grad), bits16((rw[:, None] * dHp).to(c["dtype"])))
    # exact data: the fp32 sum is the exact one
    prod = dHp.double()[:-1] * h.double()[:-1]
    assert float(prod.abs().sum(dim=1).max()) < XC.EXACT_SUM_LIMIT and torch.equal(prod * 8, (prod * 8).round())
    assert torch.equal(rwg.grad[:-1].double(), prod.sum(dim=1))
    # row_weight without grad: one launch with the weight in the epilogue
    hg2 = h.clone().requires_grad_()
    fa.qgemm_grouped_weighted(hg2, c["offsets"], *c["stack"], rw, *args).backward(dY)
    assert torch.equal(bits16(hg2.grad), bits16(fa.qgemm_grouped_input_grad(dY, c["offsets"], *c["stack"], *args, row_weight=rw)))


@pytest.mark.parametrize("native", [False, True])
def test_autograd_qgemm_grouped_glu(env, op_case, native):
    """The fused GLU over `rows`: g, u recomputed by two plain grouped launches, dg and du in fp32, dx_sorted from one
    pair-form launch, then the sum over a token's slots - moe_combine with `pos`, index_add_ without."""
    c = op_case
    fa, args, d, dtype = env.fa, (c["bits"], c["g"], c["tid"], env.num_sms), env.dev, c["dtype"]
    hidden = (c["hidden"].float() / 16).to(dtype)                  # |x| <= 1 / 4: gate pre-activations of moderate size
    R, F = c["T"] * c["k"], c["N"]
    assert c["K"] == hidden.shape[1]
    # the op's stacks map K -> F, so the roles are: the exact stacks seen as [E, F = K', K = N']; build K -> F ones here
    layers_g = exact_layers(c["bits"], 32, c["g"], dtype, c["K"], 3 * 128, False, c["E"], 9300)
    layers_u = exact_layers(c["bits"], 32, c["g"], dtype, c["K"], 3 * 128, False, c["E"], 9400)
    Qg, Sg, tg, tid = stack_exact(env, layers_g)
    Qu, Su, tu, _ = stack_exact(env, layers_u)
    # scales of 2^-3 .. 2 on |w| <= 8 and |x| <= 1/4 over K = 320 keep |g| small enough for a meaningful silu
    kw = dict(rows=c["rows"], pos=c["pos"] if native else None)
    plain = fa.qgemm_grouped_glu(hidden, c["offsets"], Qg, Sg, tg, Qu, Su, tu, *args, **kw)
    xg = hidden.clone().requires_grad_()
    hh = fa.qgemm_grouped_glu(xg, c["offsets"], Qg, Sg, tg, Qu, Su, tu, *args, **kw)
    served = int(c["offsets"][-1])
    assert torch.equal(bits16(hh[:served]), bits16(plain[:served]))
    dH = (XC.make_x(R, 3 * 128, 29, dtype, witness=False).float() / 8).to(dtype).to(d)
    hh.backward(dH)
    x = hidden.index_select(0, c["rows"].long())
    g = fa.qgemm_grouped(x, c["offsets"], Qg, Sg, tg, *args).float()
    u = fa.qgemm_grouped(x, c["offsets"], Qu, Su, tu, *args).float()
    sig = torch.sigmoid(g)
    dg = (dH.float() * u * sig * (1 + g * (1 - sig))).to(dtype)
    du = (dH.float() * (g * sig)).to(dtype)
    dx_sorted = fa.qgemm_grouped_input_grad(dg, c["offsets"], Qg, Sg, tg, *args, grad_output2=du, weight2=Qu, scales2=Su,
                                            table22=tu)
    if native:
        by_hand = fa.moe_combine(dx_sorted, c["pos"], c["offsets"])
    else:
        by_hand = torch.zeros_like(hidden).index_add_(0, c["rows"].long(), dx_sorted)    # top-2: two addends, one order
    assert torch.isfinite(xg.grad).all() and float(xg.grad.abs().max()) > 0
    assert torch.equal(bits16(xg.grad), bits16(by_hand))
    # the pair launch itself against fp64 on the exact weights: one contraction of length 2 F over [dg, du]
    off = c["offsets"].cpu().tolist()
    both = torch.cat([dg, du], dim=1).cpu()
    for e in range(c["E"]):
        r0, r1 = off[e], off[e + 1]
        if r1 > r0:
            W = torch.cat([layers_g[e].w_exact().T, layers_u[e].w_exact().T], dim=0)      # [2 F, K]
            XC.assert_componentwise(dx_sorted[r0:r1].cpu(), both[r0:r1], W, 2 * F, dtype, what=("glu pair", e))
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_glu: gradients with respect to scales"):
        fa.qgemm_grouped_glu(xg, c["offsets"], Qg, Sg, tg, Qu, Su.clone().requires_grad_(), tu, *args, **kw)


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def experts_case(env):
    """E = 4 experts from FluteLinear.from_codes (4-bit, g = 64, K = 256, F = 512), 37 tokens; expert 2 is never chosen,
    token 0 is routed only to ids outside [0, E), token 5 has one such slot."""
    d, dtype = env.dev, F16
    E, K, F, T, bits, g = 4, 256, 512, 37, 4, 64
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(41)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, bits=bits, g=g, tid=tid, dtype=dtype)
    c["gates"], c["ups"], c["downs"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)],
                                        [linear(F, K) for _ in range(E)])
    deq = lambda m: env.fa.dequantize(m.weight, m.scales, m.tables2, bits, g, tid)
    c["dense"] = [tuple(deq(m[e]).double() for m in (c["gates"], c["ups"], c["downs"])) for e in range(E)]
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


def reference_grads(c, k):
    """(fp64 gradients, the yardstick's gradients in T) of hidden and topk_weights for dOut, computed once per k."""
    if k not in c["refs"]:
        ids, weights = c["routing"][k]
        h64, w64 = c["hidden"].double().requires_grad_(), weights.double().requires_grad_()
        restated_experts(c, h64, ids, w64, lambda e, which, x: x @ c["dense"][e][which].T).backward(c["dOut"].double())
        hT, wT = c["hidden"].clone().requires_grad_(), weights.clone().requires_grad_()
        layers = (c["gates"], c["ups"], c["downs"])
        restated_experts(c, hT, ids, wT, lambda e, which, x: layers[which][e](x)).backward(c["dOut"])
        c["refs"][k] = (h64.grad, w64.grad, hT.grad, wT.grad)
    return c["refs"][k]


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("fused,native", [(False, False), (True, False), (False, True), (True, True)])
def test_flute_experts_backward(env, experts_case, fused, native, k):
    """hidden.grad and topk_weights.grad of every FluteExperts configuration against fp64 autograd of the restated block
    on dense dequantized weights; the yardstick is the same loop in T over FluteLinear's dense autograd.  The operation
    orders differ, not the precision: each error is within twice the yardstick's, in max-abs relative to max|ref|.
    Measured (MI355X, fp16): hidden.grad 5.8e-4 .. 9.7e-4 against the yardstick's 6.9e-4 .. 7.3e-4, topk_weights.grad
    4.5e-4 against 4.5e-4; the table is in DESIGN.md 3.3h."""
    c = experts_case
    ids, weights = c["routing"][k]
    gh64, gw64, ghT, gwT = reference_grads(c, k)
    experts = env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused, native_routing=native)
    with torch.no_grad():
        plain = experts(c["hidden"], ids, weights)

    def backward():
        h, w = c["hidden"].clone().requires_grad_(), weights.clone().requires_grad_()
        out = experts(h, ids, w)
        out.backward(c["dOut"])
        return out, h.grad, w.grad

    out, gh, gw = backward()
    if native or k == 2:                                           # (index_add_ at top-3: the order of a token's addends is free)
        assert torch.equal(bits16(out), bits16(plain))             # recording a graph does not change the forward
    assert gh is not None and gw is not None and torch.isfinite(gh).all() and torch.isfinite(gw).all()
    err_h, err_w = max_rel_err(gh, gh64), max_rel_err(gw, gw64)
    yard_h, yard_w = max_rel_err(ghT, gh64), max_rel_err(gwT, gw64)
    print("FluteExperts backward fused=%d native=%d k=%d: hidden.grad %.3e (yardstick %.3e), topk_weights.grad %.3e "
          "(yardstick %.3e)" % (fused, native, k, err_h, yard_h, err_w, yard_w))
    assert yard_h > 0 and yard_w > 0
    assert err_h <= 2 * yard_h, (err_h, yard_h)
    assert err_w <= 2 * yard_w, (err_w, yard_w)
    # a token routed only to ids outside [0, E) gets a zero gradient, and so do the weights of slots no expert serves
    assert torch.all(gh[0] == 0) and torch.all(gw[0] == 0) and float(gw[5, 1]) == 0
    assert torch.all(gh64[0] == 0)
    if native:                                                     # (index_add_ makes no such promise at top-3)
        _, gh2, gw2 = backward()
        assert torch.equal(bits16(gh), bits16(gh2)) and torch.equal(bits16(gw), bits16(gw2))


# ---------------------------------------------------------------------------
# block level
# ---------------------------------------------------------------------------

BLOCK_CASES = [dict(top_k=2, scoring="softmax", renormalize=False, scale=1.0),
               dict(top_k=2, scoring="sigmoid", renormalize=True, scale=2.5, n_group=2, topk_group=1, bias=True)]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=["softmax_top2", "limited_sigmoid"])
def test_sparse_moe_block_backward(env, experts_case, case):
    """FluteSparseMoeBlock backpropagates to the hidden states and to the router: the gating ops differentiate their
    documented formula in fp32 with the kernel's ids held fixed.

    The k-th and (k + 1)-th keys of every token differ by more than 2^-8 (asserted), so holding the ids fixed is no
    assumption.  The restatement is the block with its gating written in torch ops: the router's linear in T as the block
    runs it, the formula on the kernel's ids, and the same FluteExperts behind it (whose own backward
    test_flute_experts_backward bounds against dense fp64 weights).  Its fp64 evaluation of the formula is the reference;
    the same restatement with the formula in fp32 is the yardstick - the block's gate backward is that formula in that
    precision in another operation order - and the block's hidden.grad and router_weight.grad are within four times the
    yardstick's error.  That reference is not independent of the expert path - it runs the same FluteExperts backward in T,
    so the bounded quantity isolates the gate's backward and the router's linear.  The independent check is the second
    assertion: against fp64 autograd of the whole block on dense dequantized weights, each gradient is within twice the
    error of the whole block restated in T (the router's linear, the formula in fp32, FluteLinear per expert through the
    dense autograd) - test_flute_experts_backward's rule.
    Measured (MI355X, fp16): DESIGN.md 3.3h."""
    c = experts_case
    d, dtype, E, K, T = env.dev, c["dtype"], c["E"], c["K"], c["T"]
    case = dict(case)
    k = case["top_k"]
    gen = torch.Generator().manual_seed(53)
    bias = (torch.rand(E, generator=gen) * 0.2).to(d) if case.pop("bias", False) else None
    limited = case.get("n_group", 1) > 1
    scoring, renorm, scale = case["scoring"], case["renormalize"], case["scale"]
    experts = env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=True, native_routing=True)
    # a router whose logits have well separated keys
    for attempt in range(20):
        router = (torch.randn(E, K, generator=gen) * 0.08).to(dtype).to(d)
        logits = torch.nn.functional.linear(c["hidden"], router)
        s = torch.softmax(logits.float(), 1) if scoring == "softmax" else torch.sigmoid(logits.float())
        keys = logits.float() if bias is None else s + bias
        if limited:                                                # the k allowed experts are the best group's: gaps between groups
            gkeys = keys.view(T, case["n_group"], -1).max(dim=2).values.sort(dim=1, descending=True).values
            gap = gkeys[:, case["topk_group"] - 1] - gkeys[:, case["topk_group"]]
        else:
            top = keys.sort(dim=1, descending=True).values
            gap = top[:, k - 1] - top[:, k]
        if float(gap.min()) > 2.0 ** -8:
            break
    assert float(gap.min()) > 2.0 ** -8, float(gap.min())
    block = env.moe.FluteSparseMoeBlock(router.clone(), experts, bias=bias, **case)
    with torch.no_grad():
        plain = block(c["hidden"])
        if limited:
            ids, _ = env.fa.moe_gate_limited(logits, k, case["n_group"], case["topk_group"], scoring, renorm, bias, scale)
        else:
            ids, _ = env.fa.moe_gate(logits, k, scoring, renorm, bias, scale)
    block.router_weight.requires_grad_()
    h = c["hidden"].clone().requires_grad_()
    out = block(h)
    assert torch.equal(bits16(out), bits16(plain))
    out.backward(c["dOut"])
    gh, gr = h.grad, block.router_weight.grad
    assert gh is not None and gr is not None and float(gr.abs().max()) > 0

    def restated(ftype):
        hh, rr = c["hidden"].clone().requires_grad_(), router.clone().requires_grad_()
        w = gate_formula(torch.nn.functional.linear(hh, rr).to(ftype), ids, scoring, renorm, scale).float()
        experts(hh, ids, w).backward(c["dOut"])
        return hh.grad, rr.grad

    gh64, gr64 = restated(torch.float64)
    gh32, gr32 = restated(torch.float32)
    # the whole block on dense weights in fp64 (figures only)
    hd, rd = c["hidden"].double().requires_grad_(), router.double().requires_grad_()
    wd = gate_formula(hd @ rd.T, ids, scoring, renorm, scale)
    restated_experts(c, hd, ids, wd, lambda e, which, x: x @ c["dense"][e][which].T).backward(c["dOut"].double())
    # ... and in T, the yardstick of that figure
    hT, rT = c["hidden"].clone().requires_grad_(), router.clone().requires_grad_()
    wT = gate_formula(torch.nn.functional.linear(hT, rT).float(), ids, scoring, renorm, scale).to(dtype)
    layers = (c["gates"], c["ups"], c["downs"])
    restated_experts(c, hT, ids, wT, lambda e, which, x: layers[which][e](x)).backward(c["dOut"])
    for name, g, g64, g32, dense, gT in (("hidden.grad", gh, gh64.double(), gh32, hd.grad, hT.grad),
                                         ("router_weight.grad", gr, gr64.double(), gr32, rd.grad, rT.grad)):
        err, yard = max_rel_err(g, g64), max_rel_err(g32, g64)
        err_dense, yard_dense = max_rel_err(g, dense), max_rel_err(gT, dense)
        print("FluteSparseMoeBlock %s %s: %.3e against the fp64 formula, the fp32 formula %.3e (ratio %s); %.3e against the "
              "dense fp64 block, the block in T %.3e" % (case["scoring"], name, err, yard, "%.2f" % (err / yard) if yard else "-",
                                                         err_dense, yard_dense))
        assert err <= 4 * yard, (name, err, yard)
        assert yard_dense > 0 and err_dense <= 2 * yard_dense, (name, err_dense, yard_dense)
