"""The block form of the grouped qgemm (qgemm_grouped_blocks.h: 128-row blocks of the dense prefill kernel behind a grouped
front end) on the GPU, `form="blocks"` unless said otherwise, at the smallest shapes at which it can still go wrong: empty
experts, both sides of a 128-row block edge, ragged last blocks, every exit of the K ring, one to three scale blocks, a block
map that crosses a 64-expert chunk, malformed tables, non-finite rows, graph replay on another table.

Exact inputs (tests/exact_cases) must come back bit for bit per expert and equal to the row form's bits; random data within
the componentwise bound of the documented arithmetic."""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import (check_exact, dense_project, draw_row_weights, exact_layers, random_stack, restated_experts,
                                 scale_leaves, stack_exact, weighted_expected)
from tests.support import bits16, env, first_template, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
# an empty first and middle expert, both sides of a block edge, three blocks with a ragged last one
COUNTS = [0, 1, 127, 128, 129, 0, 300]
# (K, g): 4, 8 and 12 K steps - every exit of the ring unrolled by three - with one to three blocks of 8 scale groups, and
# one case at group size 64
K_CASES = [(256, 32), (512, 32), (768, 32), (1024, 64)]


def exact_matrix():
    out = []
    i = 0
    for bits in (4, 2):
        for tile_p in (32, 64):
            for dtype in (F16, BF16):
                for K, g in K_CASES:
                    # N = 256 and 512 alternate (2 bits at TileP 64: a column block of the layout is 512 wide)
                    N = 512 if (XC.cols_per_block(bits, tile_p) == 512 or i % 2) else 256
                    out.append((bits, tile_p, dtype, K, g, N, i % 5 == 3))
                    i += 1
    return out


def test_matrix_covers_what_it_claims():
    m = exact_matrix()
    assert {(b, p, d) for b, p, d, *_ in m} == {(b, p, d) for b in (4, 2) for p in (32, 64) for d in (F16, BF16)}
    for b in (4, 2):
        assert {c[5] for c in m if c[0] == b} == {256, 512} and any(c[6] for c in m if c[0] == b)
        assert {(c[3], c[4]) for c in m if c[0] == b} == set(K_CASES)


def witnessed_layers(bits, tile_p, g, dtype, K, N, pair, E, seed0):
    """exact_layers from the first seed (seed0, seed0 + 1000, ..) whose last layer - the one the accumulator witness, the last
    row of X, meets - makes an accumulator in T go wrong (XC.assert_witness, which check_exact then asserts): at K = 256 not
    every draw of a table does."""
    for seed in range(seed0, seed0 + 50000, 1000):
        layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, E, seed)
        try:
            XC.assert_witness(torch.full((K,), 4.0, dtype=torch.float64), layers[-1].w_exact(0, min(N, 256)), dtype)
        except AssertionError:
            continue
        return layers
    raise AssertionError("no seed gives a witness")


@pytest.mark.parametrize("bits,tile_p,dtype,K,g,N,pair", exact_matrix())
def test_exact_per_expert_and_equal_to_the_row_form(env, bits, tile_p, dtype, K, g, N, pair):
    seed = 100000 + 1000 * bits + 10 * tile_p + K + (dtype == BF16)
    layers = witnessed_layers(bits, tile_p, g, dtype, K, N, pair, len(COUNTS), seed)
    Q, S, t2, tid = stack_exact(env, layers)
    T = sum(COUNTS)
    from flute_amd import dev
    assert dev.grouped_form("plain", len(COUNTS), T, N, K, bits, g, tid, env.num_sms, dtype) in ("rows", "blocks")
    X = XC.make_x(T, K, seed + 77, dtype)
    Xd, off = X.to(env.dev), offsets_of(COUNTS, env.dev)
    Y = env.fa.qgemm_grouped(Xd, off, Q, S, t2, bits, g, tid, form="blocks")
    assert Y.shape == (T, N) and Y.dtype == dtype
    check_exact(env, layers, COUNTS, X, Y.cpu())
    rows = env.fa.qgemm_grouped(Xd, off, Q, S, t2, bits, g, tid, form="rows")
    assert torch.equal(Y.double(), rows.double())            # (by value: exact inputs do not depend on the summation order)


@pytest.mark.parametrize("bits,tile_p,g,dtype", [(4, 32, 32, F16), (2, 64, 32, BF16)])
def test_random_componentwise(env, bits, tile_p, g, dtype):
    """K = 2304: 36 steps, and at group size 32 nine whole scale blocks (at 64 the 36 groups are no whole blocks of 8, and the
    block form does not serve the layer)."""
    counts = [7, 0, 140, 260]
    K, N = 2048 + 256, 512
    Q, S, t2, Ws = random_stack(env, bits, tile_p, g, dtype, K, N, len(counts), seed=bits * 100 + 7)
    X = torch.randn(sum(counts), K, generator=torch.Generator().manual_seed(5)).to(dtype)
    off = offsets_of(counts)
    Y = env.fa.qgemm_grouped(X.to(env.dev), off.to(env.dev), Q, S, t2, bits, g, first_template(bits, tile_p),
                             form="blocks").cpu()
    for e, W in enumerate(Ws):
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            XC.assert_componentwise(Y[r0:r1], X[r0:r1], W, K, dtype, what=(bits, tile_p, g, dtype, e))


# ---- weighted ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def weighted_case(env):
    bits, tile_p, g, dtype, K, N = 4, 32, 32, F16, 512, 256
    layers = witnessed_layers(bits, tile_p, g, dtype, K, N, False, len(COUNTS), 9300)
    Q, S, t2, tid = stack_exact(env, layers)
    T = sum(COUNTS)
    X, w = XC.make_x(T, K, 9301, dtype), draw_row_weights(T, 9302)       # multiples of 2^-2 below 2: w R is exact in fp32
    return dict(bits=bits, g=g, dtype=dtype, K=K, N=N, layers=layers, Q=Q, S=S, t2=t2, tid=tid, X=X, w=w,
                want=weighted_expected(layers, COUNTS, X, w))


def abi_call(env, c, off, weighted, E=None, form=2, xfill=3.0):
    """The direct call with X and Y in the middle of larger buffers and the form given: rows [0, T) of Y as int16, after
    asserting that the guard rows in front of Y and the rows >= T kept the canary."""
    d, dtype, K, N = env.dev, c["dtype"], c["K"], c["N"]
    T, guard = c["X"].shape[0], 160                                  # more guard rows than a block has
    E = len(off) - 1 if E is None else E
    canary = XC.NAN_BITS[dtype]
    ybuf = torch.full((guard + T + guard, N), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + T + guard, K), xfill, dtype=dtype, device=d)
    xbuf[guard:guard + T] = c["X"].to(d)
    off = off.to(d)
    head = (0 if dtype == F16 else 1, c["bits"], c["g"], E, T, N, K, c["Q"].shape[1], c["tid"], xbuf[guard:].data_ptr(),
            off.data_ptr(), c["Q"].data_ptr(), c["S"].data_ptr(), c["t2"].data_ptr())
    tail = (ybuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream, form)
    with torch.cuda.device(d):
        if weighted:
            w = c["w"].to(d)
            rc = env.lib.flute_qgemm_grouped_weighted_ex(*head, w.data_ptr(), *tail)
        else:
            rc = env.lib.flute_qgemm_grouped_ex(*head, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(ybuf[:guard] == canary), "front guard"
    assert torch.all(ybuf[guard + T:] == canary), "rows >= T"
    return ybuf[guard:guard + T].cpu()


def test_weighted_exact_and_equal_to_the_row_form(env, weighted_case):
    c = weighted_case
    args = (c["X"].to(env.dev), offsets_of(COUNTS, env.dev), c["Q"], c["S"], c["t2"], c["w"].to(env.dev), c["bits"], c["g"],
            c["tid"])
    Y = env.fa.qgemm_grouped_weighted(*args, form="blocks")
    assert XC.exact_equal(Y, c["want"], c["dtype"])
    assert torch.equal(Y.double(), env.fa.qgemm_grouped_weighted(*args, form="rows").double())


def test_weighted_zero_fill(env, weighted_case):
    """Rows [offsets[E], T) come back as zeros - also where no expert has a row - and rows >= T are never touched."""
    c, E = weighted_case, len(COUNTS)
    off = offsets_of(COUNTS)
    off[E] = off[E - 1]
    covered = int(off[E])
    Y = abi_call(env, c, off, weighted=True)
    assert covered < sum(COUNTS) and torch.all(Y[covered:] == 0)
    assert XC.exact_equal(Y[:covered].view(c["dtype"]), c["want"][:covered], c["dtype"])
    Y = abi_call(env, c, torch.zeros(E + 1, dtype=torch.int32), weighted=True)
    assert torch.all(Y == 0)
    off = offsets_of(COUNTS)
    off[E] += 4                                                       # past the end: clamped to T, nothing zeroed
    assert XC.exact_equal(abi_call(env, c, off, weighted=True).view(c["dtype"]), c["want"], c["dtype"])


# ---- the block map -----------------------------------------------------------------------------------------------------

def test_block_map_across_a_64_expert_chunk(env):
    """E = 130, rows in experts 0 and 129 only (129 each: two blocks, the second with one row): the scan over the table
    takes three rounds of 64 experts and the second expert's blocks are found in the last."""
    E, bits, tile_p, g, dtype, K, N = 130, 4, 32, 32, F16, 256, 256
    two = witnessed_layers(bits, tile_p, g, dtype, K, N, False, 2, 9400)
    Q2, S2, t22, tid = stack_exact(env, two)
    Q = torch.zeros((E,) + Q2.shape[1:], dtype=Q2.dtype, device=env.dev)
    S = torch.zeros((E,) + S2.shape[1:], dtype=S2.dtype, device=env.dev)
    t2 = torch.zeros((E,) + t22.shape[1:], dtype=t22.dtype, device=env.dev)
    for i, e in enumerate((0, 129)):
        Q[e], S[e], t2[e] = Q2[i], S2[i], t22[i]
    counts = [0] * E
    counts[0] = counts[129] = 129
    X = XC.make_x(258, K, 9401, dtype)
    Y = env.fa.qgemm_grouped(X.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, bits, g, tid, form="blocks").cpu()
    check_exact(env, two, [129, 129], X, Y)


def test_one_expert(env):
    bits, tile_p, g, dtype, K, N = 2, 32, 32, BF16, 256, 256
    layers = witnessed_layers(bits, tile_p, g, dtype, K, N, False, 1, 9410)
    Q, S, t2, tid = stack_exact(env, layers)
    for T in (1, 130):
        X = XC.make_x(T, K, 9411 + T, dtype)
        Y = env.fa.qgemm_grouped(X.to(env.dev), offsets_of([T], env.dev), Q, S, t2, bits, g, tid, form="blocks").cpu()
        check_exact(env, layers, [T], X, Y)


# ---- determinism, graphs, the direct ABI ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_exact(env):
    bits, tile_p, g, dtype, K, N = 4, 64, 32, BF16, 512, 512
    layers = witnessed_layers(bits, tile_p, g, dtype, K, N, False, len(COUNTS), 9500)
    Q, S, t2, tid = stack_exact(env, layers)
    X = XC.make_x(sum(COUNTS), K, 9501, dtype)
    return dict(bits=bits, g=g, dtype=dtype, K=K, N=N, layers=layers, Q=Q, S=S, t2=t2, tid=tid, X=X)


def test_two_calls_equal_bits(env, small_exact):
    c = small_exact
    Xd, off = c["X"].to(env.dev), offsets_of(COUNTS, env.dev)
    run = lambda: env.fa.qgemm_grouped(Xd, off, c["Q"], c["S"], c["t2"], c["bits"], c["g"], c["tid"], form="blocks")
    assert torch.equal(bits16(run()), bits16(run()))


def test_graph_replay_honours_new_offsets(env, small_exact):
    """The grid follows from (E, T, N) alone: a captured launch replayed after `offsets` and X were overwritten in place with
    another table of the same T returns, bit for bit, what an eager call on it returns.  One stream, no parallel branches."""
    c = small_exact
    T = sum(COUNTS)
    counts2 = [130, 255, 0, 0, 1, 299, 0]
    assert sum(counts2) == T and len(counts2) == len(COUNTS)
    X2 = XC.make_x(T, c["K"], 9502, c["dtype"]).to(env.dev)
    off2 = offsets_of(counts2, env.dev)
    x, off = c["X"].to(env.dev).clone(), offsets_of(COUNTS, env.dev)
    run = lambda xx, oo: env.fa.qgemm_grouped(xx, oo, c["Q"], c["S"], c["t2"], c["bits"], c["g"], c["tid"], env.num_sms,
                                              form="blocks")
    first = run(x, off).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run(x, off)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(first))
    off.copy_(off2)
    x.copy_(X2)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = run(X2, off2)
    assert torch.equal(bits16(y), bits16(eager))
    check_exact(env, c["layers"], counts2, X2.cpu(), y.cpu())
    assert not torch.equal(bits16(eager), bits16(first))


def test_direct_abi_writes_exactly_its_rows(env, small_exact):
    """X and Y in the middle of larger buffers.  A well-formed table whose last entry lies past T, then a table with a
    decreasing entry and one with overlapping ranges: the kernel clamps every bound to [0, T], so nothing outside Y's T rows
    is written (abi_call asserts the canaries), and every row only one expert names holds that expert's exact product."""
    c = small_exact
    T, E = sum(COUNTS), len(COUNTS)
    off = offsets_of(COUNTS)
    off[E] = T + 200
    Y = abi_call(env, c, off, weighted=False).view(c["dtype"])
    check_exact(env, c["layers"], COUNTS, c["X"], Y)

    def rows_of(e, r0, r1):
        R = XC.exact_product(c["X"][r0:r1], c["layers"][e])
        return XC.exact_equal(Y[r0:r1], R, c["dtype"])

    # a decreasing entry: expert 1 = [100, 50) has no rows, expert 2 = [50, 400) overlaps expert 0 = [0, 100) in rows [50, 100)
    # (unspecified contents there); a negative first entry and a last one far past T are clamped
    dec = torch.tensor([-5, 100, 50, 400, 400, 400, 400, T + 10 ** 6], dtype=torch.int32)
    Y = abi_call(env, c, dec, weighted=False).view(c["dtype"])
    assert rows_of(0, 0, 50) and rows_of(2, 100, 400) and rows_of(6, 400, T)
    # overlapping ranges that own more blocks than the grid holds: experts 1, 3 and 5 each claim every row (18 blocks, the
    # grid has 12 row blocks), the others [T, 0) - none
    abi_call(env, c, torch.tensor([T, 0, T, 0, T, 0, T, 0], dtype=torch.int32), weighted=False)
    # no expert has a row: the plain launch writes nothing at all
    Y = abi_call(env, c, torch.zeros(E + 1, dtype=torch.int32), weighted=False)
    assert torch.all(Y == XC.NAN_BITS[c["dtype"]])


# ---- non-finite rows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
def test_non_finite_rows_stay_in_their_rows(env, weighted_case, weighted):
    """A NaN row and an Inf row in the middle of a block, and a NaN in the last row before an expert's end (the rows after it
    in that block are read as zeros and never stored): exactly those output rows are non-finite, the others keep the bits
    of the clean launch.  The activations past the expert's end and around X are Inf in the buffer the direct call reads."""
    c = weighted_case
    off = offsets_of(COUNTS)
    clean = abi_call(env, c, off, weighted)
    assert torch.isfinite(clean.view(c["dtype"])).all()
    bad = {int(off[3]) + 40: float("nan"), int(off[3]) + 90: float("inf"), int(off[5]) - 1: float("nan"),
           int(off[7]) - 300 + 127: float("inf")}
    X = c["X"].clone()
    for r, v in bad.items():
        X[r, 17] = v
    poisoned = dict(c, X=X)
    Y = abi_call(env, poisoned, off, weighted, xfill=float("inf"))
    finite = torch.isfinite(Y.view(c["dtype"])).all(dim=1)
    assert sorted((~finite).nonzero().flatten().tolist()) == sorted(bad)
    assert not torch.isfinite(Y.view(c["dtype"])[sorted(bad)]).all(dim=1).any()
    assert torch.equal(Y[finite], clean[finite])


# ---- the module --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def module_case(env):
    """E = 2 experts (4-bit, g = 32, K = 256, N_ff = 256, fp16), top-1, 300 tokens: a mean of 150 rows per expert, above the
    rule's threshold, so the weighted down projection and the backward's recompute of gate and up take the block form (the
    fused GLU launch has none).  `lut`: every layer's lookups [N, K] in fp64 (test_grouped_scale_grad_gpu.py, make_experts_case)."""
    from flute_amd import dev
    d, dtype = env.dev, F16
    E, K, F, T, bits, g = 2, 256, 256, 300, 4, 32
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(51)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, bits=bits, g=g, tid=tid, dtype=dtype, chunk=60)
    c["layers"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)], [linear(F, K) for _ in range(E)])
    lut = lambda m: env.fa.dequantize(m.weight, torch.ones_like(m.scales), m.tables2, bits, g, tid).double()
    c["lut"] = [[lut(m) for m in ms] for ms in c["layers"]]
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["dOut"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["ids"] = torch.randint(0, E, (T, 1), generator=gen).to(d)
    c["weights"] = (torch.rand(T, 1, generator=gen) * 0.5 + 0.5).to(dtype).to(d)
    for mode, N, Kin in (("plain", F, K), ("weighted", K, F)):
        assert dev.grouped_form(mode, E, T, N, Kin, bits, g, tid, env.num_sms, dtype) == "blocks"
        assert dev.grouped_form(mode, E, c["chunk"], N, Kin, bits, g, tid, env.num_sms, dtype) == "rows"
    return c


def test_flute_experts_forward_on_the_block_form(env, module_case):
    """test_flute_experts_against_loop_and_fp64's bound at a token count whose down projection takes the block form:
    max|Y - R| <= 2 max|Y_loop - R|, R the fp64 result on the dequantized weights, Y_loop the per-expert loop over
    FluteLinear on rows selected on the host."""
    c = module_case
    gates, ups, downs = c["layers"]
    hidden, ids, weights = c["hidden"], c["ids"], c["weights"]
    experts = env.moe.FluteExperts.from_linears(gates, ups, downs, fused=True, native_routing=True)
    Y = experts(hidden, ids, weights)
    deq = lambda m: env.fa.dequantize(m.weight, m.scales, m.tables2, c["bits"], c["g"], c["tid"]).double()
    R = restated_experts(c, hidden.double(), ids, weights.double(), lambda e, which, x: x @ deq(c["layers"][which][e]).T)
    Y_loop = restated_experts(c, hidden, ids, weights, lambda e, which, x: c["layers"][which][e](x))
    err, err_loop = float((Y.double() - R).abs().max()), float((Y_loop.double() - R).abs().max())
    print("FluteExperts on the block form: max|Y - R| = %.3e, loop %.3e, max|R| = %.3e" % (err, err_loop, float(R.abs().max())))
    assert err_loop > 0
    assert err <= 2 * err_loop, (err, err_loop)
    assert torch.equal(bits16(Y), bits16(experts(hidden, ids, weights)))


def test_flute_experts_backward_on_the_block_form(env, module_case):
    """One backward with learnable scales at 300 tokens - the down projection and the recompute of gate and up on the block
    form - against the same step with the tokens split into chunks of 60, which fall on the row form (asserted in the fixture;
    the scale gradients of the chunks add up in the parameters' .grad).  The inputs are random, so neither is exact: the
    reference is fp64 autograd of the restated block on dense weights L * S with S an fp64 leaf, the chunked row-form step is
    the yardstick, and - the rule of test_flute_experts_scale_grads and test_flute_experts_backward - every gradient's max-abs
    error relative to max|ref| is within twice the yardstick's."""
    c = module_case
    hidden, ids, weights, dOut = c["hidden"], c["ids"], c["weights"], c["dOut"]
    S64 = scale_leaves(c)
    h64 = hidden.double().requires_grad_()
    restated_experts(c, h64, ids, weights.double(), dense_project(c, S64)).backward(dOut.double())
    ref = [s.grad for s in S64] + [h64.grad]

    def step(chunk):
        experts = env.moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
        params = env.moe.make_experts_learnable(experts)
        assert len(params) == 3
        hgrads = []
        for r0 in range(0, c["T"], chunk):
            h = hidden[r0:r0 + chunk].clone().requires_grad_()
            experts(h, ids[r0:r0 + chunk], weights[r0:r0 + chunk]).backward(dOut[r0:r0 + chunk])
            hgrads.append(h.grad)
        return [p.grad for p in params] + [torch.cat(hgrads)]

    got, yard = step(c["T"]), step(c["chunk"])
    for name, a, y, r in zip(("gate scales", "up scales", "down scales", "hidden"), got, yard, ref):
        assert a is not None and a.shape == r.shape and torch.isfinite(a).all()
        err, yerr = max_rel_err(a, r), max_rel_err(y, r)
        print("block-form step, %s.grad: %.3e (row-form chunks %.3e)" % (name, err, yerr))
        assert yerr > 0
        assert err <= 2 * yerr, (name, err, yerr)
