"""The 3-bit block form of the grouped qgemm (qgemm_block3.h behind the grouped front end; `qgemm_grouped_w3_blocks` and
`qgemm_grouped_weighted_w3_blocks`) on the GPU, at the smallest shapes at which it can still go wrong: empty experts, both sides
of a 128-row block edge, a ragged last block, every exit of the K ring, one to three scale blocks, a block map that crosses a
64-expert chunk, malformed tables, non-finite rows.  Exact inputs (tests/exact_cases) come back bit for bit per expert and equal
to the row form; random data within the componentwise bound of the documented arithmetic.  (N is 512 or 1024: a 3-bit layer's
column block is 512 wide, so no legal layer has 256 columns; 512 is two of the kernel's 256-column blocks.)"""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import check_exact, draw_row_weights, exact_layers, random_stack, stack_exact, weighted_expected
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
BITS, TILE_P = 3, 32
COUNTS = [0, 1, 127, 128, 129, 0, 300]           # empty first and middle experts, both sides of a block edge, a ragged third block
K_CASES = [(256, 32), (512, 32), (768, 32), (1024, 64)]     # 4, 8, 12, 16 K steps: every exit of the ring; one to three scale blocks
EXACT = [(dtype, K, g, 512 if i % 2 == 0 else 1024, i % 3 == 1)
         for i, (dtype, (K, g)) in enumerate((d, kg) for d in (F16, BF16) for kg in K_CASES)]


def witnessed_layers(g, dtype, K, N, pair, E, seed0):
    """exact_layers from the first seed whose last layer - the one the witness row of X meets - makes an accumulator in T go
    wrong (XC.assert_witness, which check_exact then asserts): at K = 256 not every draw of a table does."""
    for seed in range(seed0, seed0 + 50000, 1000):
        layers = exact_layers(BITS, TILE_P, g, dtype, K, N, pair, E, seed)
        try:
            XC.assert_witness(torch.full((K,), 4.0, dtype=torch.float64), layers[-1].w_exact(0, 256), dtype)
        except AssertionError:
            continue
        return layers
    raise AssertionError("no seed gives a witness")


@pytest.mark.parametrize("dtype,K,g,N,pair", EXACT)
def test_exact_per_expert_and_equal_to_the_row_form(env, dtype, K, g, N, pair):
    assert sum(c[4] for c in EXACT) >= 2 and {c[3] for c in EXACT} == {512, 1024}
    seed = 300000 + K + (dtype == BF16)
    layers = witnessed_layers(g, dtype, K, N, pair, len(COUNTS), seed)
    Q, S, t2, tid = stack_exact(env, layers)
    X = XC.make_x(sum(COUNTS), K, seed + 77, dtype)
    Xd, off = X.to(env.dev), offsets_of(COUNTS, env.dev)
    Y = env.fa.qgemm_grouped_w3_blocks(Xd, off, Q, S, t2, BITS, g, tid)
    assert Y.shape == (sum(COUNTS), N) and Y.dtype == dtype
    check_exact(env, layers, COUNTS, X, Y.cpu())
    assert torch.equal(Y.double(), env.fa.qgemm_grouped(Xd, off, Q, S, t2, BITS, g, tid, form="rows").double())


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_random_componentwise(env, dtype):
    """K = 2304 at group size 32: 36 steps, nine whole scale blocks."""
    counts, K, N, g = [7, 0, 140, 260], 2304, 512, 32
    Q, S, t2, Ws = random_stack(env, BITS, TILE_P, g, dtype, K, N, len(counts), seed=307)
    X = torch.randn(sum(counts), K, generator=torch.Generator().manual_seed(5)).to(dtype)
    off = offsets_of(counts)
    Y = env.fa.qgemm_grouped_w3_blocks(X.to(env.dev), off.to(env.dev), Q, S, t2, BITS, g, first_template(BITS, TILE_P)).cpu()
    for e, W in enumerate(Ws):
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            XC.assert_componentwise(Y[r0:r1], X[r0:r1], W, K, dtype, what=(dtype, e))


def make_case(env, dtype):
    if dtype in env.cache:
        return env.cache[dtype]
    g, K, N = 32, 512, 512
    layers = witnessed_layers(g, dtype, K, N, False, len(COUNTS), 309300)
    Q, S, t2, tid = stack_exact(env, layers)
    T = sum(COUNTS)
    X, w = XC.make_x(T, K, 309301, dtype), draw_row_weights(T, 309302)      # multiples of 2^-2 below 2: w R is exact in fp32
    env.cache[dtype] = dict(g=g, dtype=dtype, K=K, N=N, layers=layers, Q=Q, S=S, t2=t2, tid=tid, X=X, w=w,
                            want=weighted_expected(layers, COUNTS, X, w))
    return env.cache[dtype]


@pytest.fixture(params=[F16, BF16], ids=["f16", "bf16"])
def case(env, request):
    return make_case(env, request.param)


def abi_call(env, c, off, weighted, xfill=3.0):
    """The direct call with X and Y in the middle of larger buffers: rows [0, T) of Y as int16, after asserting that the 160
    guard rows in front of Y and behind row T kept the canary."""
    d, dtype, K, N = env.dev, c["dtype"], c["K"], c["N"]
    T, guard, canary = c["X"].shape[0], 160, XC.NAN_BITS[c["dtype"]]
    ybuf = torch.full((guard + T + guard, N), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + T + guard, K), xfill, dtype=dtype, device=d)
    xbuf[guard:guard + T] = c["X"].to(d)
    off, w = off.to(d), c["w"].to(d)
    head = (0 if dtype == F16 else 1, BITS, c["g"], len(off) - 1, T, N, K, c["Q"].shape[1], c["tid"], xbuf[guard:].data_ptr(),
            off.data_ptr(), c["Q"].data_ptr(), c["S"].data_ptr(), c["t2"].data_ptr())
    tail = (ybuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_weighted_w3_blocks(*head, w.data_ptr(), *tail) if weighted else \
            env.lib.flute_qgemm_grouped_w3_blocks(*head, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(ybuf[:guard] == canary) and torch.all(ybuf[guard + T:] == canary), "guard rows"
    return ybuf[guard:guard + T].cpu()


def test_weighted_exact_and_zero_fill(env, case):
    """round_T(w R) inside the table; with a last entry below T the rows from offsets[E] on are zeros."""
    c, E = case, len(COUNTS)
    Y = env.fa.qgemm_grouped_weighted_w3_blocks(c["X"].to(env.dev), offsets_of(COUNTS, env.dev), c["Q"], c["S"], c["t2"],
                                                c["w"].to(env.dev), BITS, c["g"], c["tid"])
    assert XC.exact_equal(Y, c["want"], c["dtype"])
    off = offsets_of(COUNTS)
    off[E] = off[E - 1]
    covered = int(off[E])
    Y = abi_call(env, c, off, weighted=True)
    assert covered < sum(COUNTS) and torch.all(Y[covered:] == 0)
    assert XC.exact_equal(Y[:covered].view(c["dtype"]), c["want"][:covered], c["dtype"])


@pytest.mark.parametrize("weighted", [False, True])
def test_direct_abi_writes_exactly_its_rows(env, case, weighted):
    c = case
    T, E = sum(COUNTS), len(COUNTS)
    want = c["want"] if weighted else weighted_expected(c["layers"], COUNTS, c["X"], torch.ones(T))
    assert XC.exact_equal(abi_call(env, c, offsets_of(COUNTS), weighted).view(c["dtype"]), want, c["dtype"])
    # a decreasing entry (expert 1 = [100, 50) has no rows, expert 2 overlaps expert 0 in [50, 100)), a negative first entry and
    # a last one far past T: rows one expert names hold its product; then ranges that claim 18 blocks of a grid of 12
    dec = torch.tensor([-5, 100, 50, 400, 400, 400, 400, T + 10 ** 6], dtype=torch.int32)
    Y = abi_call(env, c, dec, weighted).view(c["dtype"])
    for e, r0, r1 in ((0, 0, 50), (2, 100, 400), (6, 400, T)):
        R = XC.exact_product(c["X"][r0:r1], c["layers"][e]) * (c["w"][r0:r1].double()[:, None] if weighted else 1)
        assert XC.exact_equal(Y[r0:r1], R, c["dtype"]), e
    abi_call(env, c, torch.tensor([T, 0, T, 0, T, 0, T, 0], dtype=torch.int32), weighted)
    Y = abi_call(env, c, torch.zeros(E + 1, dtype=torch.int32), weighted)          # no expert has a row
    assert torch.all(Y == (0 if weighted else XC.NAN_BITS[c["dtype"]]))


def test_block_map_across_a_64_expert_chunk(env):
    """E = 66 with rows in experts 0, 63, 64 and 65 only: the scan over the table takes two rounds of 64 experts."""
    E, g, dtype, K, N, live = 66, 32, F16, 256, 512, (0, 63, 64, 65)
    some = witnessed_layers(g, dtype, K, N, False, len(live), 309400)
    Qs, Ss, t2s, tid = stack_exact(env, some)
    Q, S, t2 = (torch.zeros((E,) + t.shape[1:], dtype=t.dtype, device=env.dev) for t in (Qs, Ss, t2s))
    counts, rows = [0] * E, (129, 1, 130, 128)
    for i, e in enumerate(live):
        Q[e], S[e], t2[e], counts[e] = Qs[i], Ss[i], t2s[i], rows[i]
    X = XC.make_x(sum(rows), K, 309401, dtype)
    Y = env.fa.qgemm_grouped_w3_blocks(X.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, BITS, g, tid).cpu()
    check_exact(env, some, list(rows), X, Y)


@pytest.mark.parametrize("weighted", [False, True])
def test_non_finite_rows_stay_in_their_rows(env, case, weighted):
    """A NaN row and an Inf row inside a block, a NaN in the last row before an expert's end and an Inf in the ragged last block:
    exactly those output rows are non-finite, the others keep the clean launch's bits.  The activations around X - the rows a
    ragged block would read past `re` of the last expert - are Inf, and the guard rows behind them stay canary (abi_call)."""
    c, off = case, offsets_of(COUNTS)
    clean = abi_call(env, c, off, weighted)
    assert torch.isfinite(clean.view(c["dtype"])).all()
    bad = {int(off[3]) + 40: float("nan"), int(off[3]) + 90: float("inf"), int(off[5]) - 1: float("nan"),
           int(off[7]) - 300 + 127: float("inf"), int(off[7]) - 1: float("inf")}
    X = c["X"].clone()
    for r, v in bad.items():
        X[r, 17] = v
    Y = abi_call(env, dict(c, X=X), off, weighted, xfill=float("inf"))
    finite = torch.isfinite(Y.view(c["dtype"])).all(dim=1)
    assert sorted((~finite).nonzero().flatten().tolist()) == sorted(bad)
    assert torch.equal(Y[finite], clean[finite])


def test_autograd_equals_the_row_form(env):
    """The backward kernels are the same, so dX - and d row_weight of the weighted op - equal the row form's bit for bit."""
    c, d = make_case(env, F16), env.dev
    off, stack, tail = offsets_of(COUNTS, d), (c["Q"], c["S"], c["t2"]), (BITS, c["g"], c["tid"])
    dY = XC.make_x(sum(COUNTS), c["N"], 309500, c["dtype"]).to(d)

    def grads(op, weighted, **kw):
        x, w = c["X"].to(d).requires_grad_(), c["w"].to(d).requires_grad_()
        y = op(x, off, *stack, *((w,) if weighted else ()), *tail, **kw)
        y.backward(dY)
        return (y.detach(), x.grad) + ((w.grad,) if weighted else ())

    for new, old, weighted in ((env.fa.qgemm_grouped_w3_blocks, env.fa.qgemm_grouped, False),
                               (env.fa.qgemm_grouped_weighted_w3_blocks, env.fa.qgemm_grouped_weighted, True)):
        for a, b in zip(grads(new, weighted), grads(old, weighted, form="rows")):
            assert a is not None and torch.equal(a.double(), b.double())


def test_flute_experts_w3_blocks_equals_the_default(env):
    """Inputs on which every sum is exact in fp32 in any order, so the row and the block form must agree bit for bit: a token is
    4 at one position, the gate's table gives g = 4 t in [20, 30] (silu32(g) = g exactly from 18 on), the up's u in +-{1 .. 4},
    so h = g u is an integer below 128, and the down stack's weights are integers in [-4, 3] / 16: |sums| < 2^24 quanta.
    `w3_blocks=True` - fused: the weighted down launch; unfused: all three launches - returns what `w3_blocks=False` returns."""
    E, K, F, g, T, dtype, d = 2, 512, 512, 32, 300, F16, env.dev
    tid, gen = first_template(BITS, TILE_P), torch.Generator().manual_seed(309600)
    tables = (torch.tensor([5, 5.25, 5.5, 6, 6.25, 6.5, 7, 7.5]), torch.tensor([-1, -.75, -.5, -.25, .25, .5, .75, 1]),
              torch.arange(-4., 4.))

    def linear(kk, nn, table, scale):
        codes = torch.randint(0, 8, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        return env.FluteLinear.from_codes(codes, torch.full((nn, kk // g), scale, dtype=dtype, device=d), table.to(dtype).to(d),
                                          BITS, g, tid)

    layers = [[linear(kk, nn, table, scale) for _ in range(E)]
              for kk, nn, table, scale in ((K, F, tables[0], 1.0), (K, F, tables[1], 1.0), (F, K, tables[2], 2.0 ** -4))]
    hidden = torch.zeros(T, K, dtype=dtype)
    hidden[torch.arange(T), torch.randint(0, K, (T,), generator=gen)] = 4
    hidden, ids = hidden.to(d), torch.randint(0, E, (T, 1), generator=gen).to(d)
    weights = torch.ones(T, 1, dtype=dtype, device=d)
    for kw in (dict(fused=True, native_routing=True), dict()):
        new = env.moe.FluteExperts.from_linears(*layers, w3_blocks=True, **kw)(hidden, ids, weights)
        old = env.moe.FluteExperts.from_linears(*layers, w3_blocks=False, **kw)(hidden, ids, weights)
        assert torch.isfinite(new).all() and new.abs().max() > 0 and torch.equal(new.double(), old.double())
