"""flute_amd.moe_gate / moe_gate_route (moe_gate.hip), FluteExperts.forward_logits and FluteSparseMoeBlock on the GPU.

The yardstick is the contract in fp64 on the host (tests/moe_gate_ref.py: a stable descending sort of the keys).

Choice.  `ids` value for value, three logit dtypes x both scorings x with and without the selection bias, every output in
a canary-padded buffer.  Without a bias the keys are the logits themselves and nothing is conditioned; with a bias the key
is a rounded score plus the bias, so the inputs are drawn until, for every token, the fp64 keys of the chosen experts and
of the best one left out differ pairwise by more than 2^-16 (an fp32 key is within a few 2^-24 of the fp64 one).

Weights.  |w - w64| <= r |w64| element by element, r = four times the worst relative error of torch's own fp32 chain
(softmax / sigmoid, gather, sum, div) on the GPU on the same inputs against the same fp64 values - measured in the test,
per scoring and renormalisation, not fixed here.  Measured on an MI355X (worst over the test's inputs; torch's chain /
the kernel):

    softmax                 5.52e-07 / 5.98e-07      (r = 2.21e-06)
    softmax, renormalised   6.63e-07 / 5.57e-07      (r = 2.65e-06)
    sigmoid                 1.04e-07 / 1.04e-07      (r = 4.15e-07)
    sigmoid, renormalised   2.02e-07 / 1.63e-07      (r = 8.07e-07)

Equal bits, the module and the anchor to `torch.topk(softmax)` are described on the tests."""
import pytest
import torch

from tests import moe_gate_ref as R
from tests.moe_cases import (CANARY, canary_padded, draw_bias, draw_logits, gate_abi, host_route, intact, native, same_bits,  # noqa: F401
                             top3_case)
from tests.support import bits16, env  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
I32 = torch.int32
GAP = 2.0 ** -16

SHAPES = [
    (1, 1, 1),                  # the smallest case
    (1, 8, 2),
    (5, 60, 4),                 # E is not a multiple of 64
    (37, 64, 8),                # more tokens than the routed form has waves
    (3, 256, 8),                # four values per lane
    (2, 1000, 64),              # sixteen values per lane, the last ones past E; the largest k
    (2, 1024, 1),               # the cap on E
    (1030, 8, 2),               # the standalone grid: many workgroups, the last one not full
]


# ---- inputs and calls --------------------------------------------------------------------------------------------------------

def draw_separated(T, E, k, dtype, scoring, bias, seed, key_of=None):
    """Logits whose fp64 keys (score + bias, or `key_of`) satisfy the 2^-16 condition in every token: tokens that fail are
    drawn again with the next seed."""
    key_of = key_of or (lambda x: R.keys(x, scoring, bias))
    x = draw_logits(T, E, dtype, seed)
    for attempt in range(1, 200):
        bad = ~R.separated(key_of(x), k, GAP)
        if not bool(bad.any()):
            return x
        x[bad] = draw_logits(T, E, dtype, seed + 7919 * attempt)[bad]
    raise AssertionError("no separated draw for %s" % ((T, E, k, dtype, scoring),))


# ---- 1. the choice, value for value ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("T,E,k", SHAPES)
def test_ids_equal_the_reference(env, T, E, k, dtype):
    d = env.dev
    for scoring in ("softmax", "sigmoid"):
        for with_bias in (False, True):
            seed = 100 * T + E + k
            bias = draw_bias(E, seed + 1) if with_bias else None
            x = draw_separated(T, E, k, dtype, scoring, bias, seed) if with_bias else draw_logits(T, E, dtype, seed)
            want, _ = R.gate(x, k, scoring, bias=bias)
            xd, bd = x.to(d), None if bias is None else bias.to(d)
            what = (T, E, k, dtype, scoring, with_bias)
            for got in (gate_abi(env, xd, k, scoring, bias=bd)[0], gate_abi(env, xd, k, scoring, bias=bd, routed=True)[0],
                        env.fa.moe_gate(xd, k, scoring, bias=bd)[0], env.fa.moe_gate_route(xd, k, E, scoring, bias=bd)[0]):
                assert got.dtype == I32 and got.shape == (T, k)
                assert torch.equal(got.cpu().long(), want), what
            assert all(len(set(row)) == k for row in want.tolist())


# ---- 2. ties and edges: ids only ---------------------------------------------------------------------------------------------

def check_ids(env, x, k, want=None):
    ref = R.gate(x, k)[0]
    if want is not None:
        assert ref.tolist() == want, "the reference itself"
    xd = x.to(env.dev)
    for scoring in ("softmax", "sigmoid"):
        assert ref.tolist() == R.gate(x, k, scoring)[0].tolist()           # without a bias the key is the logit
        for got in (gate_abi(env, xd, k, scoring)[0], env.fa.moe_gate_route(xd, k, None, scoring)[0]):
            assert got.cpu().tolist() == ref.tolist(), (tuple(x.shape), k, x.dtype, scoring)


def test_all_logits_equal_gives_the_first_k(env):
    for dtype in (F16, F32):
        check_ids(env, torch.full((3, 200), 1.5, dtype=dtype), 5, [[0, 1, 2, 3, 4]] * 3)
        check_ids(env, torch.zeros(2, 64, dtype=dtype), 64, [list(range(64))] * 2)
        check_ids(env, torch.full((1, 1000), -7.0, dtype=dtype), 64, [list(range(64))])
    mixed = torch.zeros(1, 130)
    mixed[0, ::2] = -0.0                                                 # -0 equals +0
    check_ids(env, mixed, 6, [[0, 1, 2, 3, 4, 5]])


def test_ties_in_one_lane_and_in_neighbouring_lanes(env):
    x = draw_logits(4, 256, F32, 5)
    x[:, 5] = x[:, 69] = 50.0            # e and e + 64: the same lane, the next register
    x[:, 100] = x[:, 101] = 40.0         # e and e + 1: neighbouring lanes
    x[:, 255] = x[:, 63] = x[:, 64] = 30.0
    check_ids(env, x, 7, [[5, 69, 100, 101, 63, 64, 255]] * 4)
    y = draw_logits(2, 1000, F32, 6)
    y[:, 999] = y[:, 935] = y[:, 39] = 60.0                              # one lane (39), registers 0, 14 and 15
    y[:, 15] = y[:, 16] = y[:, 31] = y[:, 32] = 55.0                     # across the rows of 16 lanes and the halves of the wave
    assert R.gate(y, 8)[0][:, :7].tolist() == [[39, 935, 999, 15, 16, 31, 32]] * 2
    check_ids(env, y, 8)


def test_an_entirely_negative_row(env):
    """A maximum that started at 0, or an empty slot past E that held 0, would win here."""
    for E, k in ((60, 4), (100, 8), (8, 8)):
        for dtype in (F16, F32):
            x = (-300.0 - torch.rand(3, E, generator=torch.Generator().manual_seed(E)) * 8).to(dtype)
            check_ids(env, x, k)
            ids, w = env.fa.moe_gate(x.to(env.dev), k, "softmax", True)
            assert bool(torch.isfinite(w).all()) and bool((w > 0).all())


def test_minus_infinity_and_nan(env):
    inf, nan = float("inf"), float("nan")
    x = torch.full((2, 70), -inf)
    x[0, 3], x[0, 68], x[0, 40] = 1.0, 2.0, -5.0
    x[1, 69], x[1, 0], x[1, 64] = 0.5, 0.25, 0.75
    check_ids(env, x, 3, [[68, 3, 40], [64, 69, 0]])                      # -inf on all but k experts
    check_ids(env, x, 5, [[68, 3, 40, 0, 1], [64, 69, 0, 1, 2]])          # fewer than k numbers: -inf in index order behind them
    check_ids(env, torch.full((1, 9), -inf), 2, [[0, 1]])
    y = draw_logits(3, 130, F32, 9)
    y[:, 0] = y[:, 7] = y[:, 64] = y[:, 129] = nan                        # NaN is never chosen while k numbers remain
    y[1, 20] = -inf
    y[2, 30] = inf
    ids = R.gate(y, 8)[0]
    assert not (set(ids.reshape(-1).tolist()) & {0, 7, 64, 129}) and ids[2, 0] == 30
    check_ids(env, y, 8)
    z = torch.tensor([[nan, -5.0, -inf, nan, 2.0]])
    check_ids(env, z, 5, [[4, 1, 0, 2, 3]])                               # NaN ranks as -inf, in index order among its like
    check_ids(env, z.to(F16), 4, [[4, 1, 0, 2]])


def test_fp16_logits_with_many_exact_duplicates(env):
    gen = torch.Generator().manual_seed(12)
    for T, E, k in ((37, 200, 8), (5, 1024, 64)):
        x = (torch.randint(-3, 4, (T, E), generator=gen).float() / 2).to(F16)
        check_ids(env, x, k)
        check_ids(env, x.to(BF16), k)


# ---- 3. the weights against fp64 ---------------------------------------------------------------------------------------------

WEIGHT_SHAPES = [(1, 1, 1), (1, 8, 2), (5, 60, 4), (37, 64, 8), (3, 256, 8), (2, 1000, 64)]


@pytest.fixture(scope="module")
def weight_cases(env):
    """Every input of the weights test with its fp64 reference and the error of torch's own fp32 chain on the GPU, computed
    once: a list of dicts, and r[(scoring, renormalize)] = 4 x the worst relative error of the chain over all of them."""
    d = env.dev
    cases, worst = [], {}
    for T, E, k in WEIGHT_SHAPES:
        for dtype in (F16, BF16, F32):
            for scoring in ("softmax", "sigmoid"):
                for with_bias in (False, True):
                    seed = 7 * T + E + k
                    bias = draw_bias(E, seed + 1) if with_bias else None
                    x = draw_separated(T, E, k, dtype, scoring, bias, seed) if with_bias else draw_logits(T, E, dtype, seed)
                    if scoring == "softmax" and not with_bias and T > 1:
                        x[1::2] = (x[1::2].float() - 300.0).to(dtype)          # entirely negative rows (a sigmoid of -300 is 0)
                    xd = x.to(d)
                    for renorm in (False, True):
                        ids, w64 = R.gate(x, k, scoring, renorm, bias)
                        xf = x.double()
                        if scoring == "softmax":                                # nothing chosen underflows
                            assert bool(((xf.gather(1, ids) - xf.max(1, keepdim=True).values) >= -20).all())
                        else:
                            assert bool((xf.gather(1, ids) >= -20).all())
                        s32 = torch.softmax(xd.float(), dim=1) if scoring == "softmax" else torch.sigmoid(xd.float())
                        w32 = s32.gather(1, ids.to(d))
                        if renorm:
                            w32 = w32 / w32.sum(dim=1, keepdim=True)
                        err = float(((w32.cpu().double() - w64).abs() / w64).max())
                        worst[(scoring, renorm)] = max(worst.get((scoring, renorm), 0.0), err)
                        cases.append(dict(T=T, E=E, k=k, dtype=dtype, scoring=scoring, renorm=renorm, x=xd, ids=ids, w64=w64,
                                          bias=None if bias is None else bias.to(d)))
    return cases, {key: 4.0 * v for key, v in worst.items()}


def test_weights_against_fp64(env, weight_cases):
    cases, r = weight_cases
    kernel_worst = {}
    failures = []
    for c in cases:
        key = (c["scoring"], c["renorm"])
        ids, w = env.fa.moe_gate(c["x"], c["k"], c["scoring"], c["renorm"], c["bias"])
        assert w.dtype == F32 and torch.equal(ids.cpu().long(), c["ids"])
        w_d = w.cpu().double()
        rel = (w_d - c["w64"]).abs() / c["w64"]
        kernel_worst[key] = max(kernel_worst.get(key, 0.0), float(rel.max()))
        what = (c["T"], c["E"], c["k"], c["dtype"], c["scoring"], c["renorm"], c["bias"] is not None)
        if not bool((rel <= r[key]).all()):
            failures.append((what, float(rel.max()), r[key]))
        if c["renorm"]:
            off = float((w_d.sum(dim=1) - 1.0).abs().max())
            if not off <= c["k"] * r[key]:
                failures.append((what, "row sum", off, c["k"] * r[key]))
    for key in sorted(r):
        print("moe_gate weights %s renormalize=%s: torch fp32 chain worst rel err %.3e (r = %.3e), kernel %.3e"
              % (key[0], key[1], r[key] / 4, r[key], kernel_worst[key]))
    assert all(v > 0 for v in r.values())
    assert not failures, failures


def test_scale_is_one_more_rounding(env, weight_cases):
    cases, _ = weight_cases
    for c in cases:
        if c["dtype"] != F32 and c["E"] != 64:
            continue
        one = env.fa.moe_gate(c["x"], c["k"], c["scoring"], c["renorm"], c["bias"])[1]
        ids, scaled = env.fa.moe_gate(c["x"], c["k"], c["scoring"], c["renorm"], c["bias"], 2.5)
        assert torch.equal(ids.cpu().long(), c["ids"])
        assert same_bits(scaled, one * 2.5), (c["T"], c["E"], c["k"], c["dtype"], c["scoring"], c["renorm"])


# ---- 4. equal bits -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scoring,renorm,with_bias", [("softmax", True, False), ("softmax", False, True), ("sigmoid", True, True),
                                                      ("sigmoid", False, False)])
def test_equal_bits(env, scoring, renorm, with_bias):
    d = env.dev
    for (T, E, k), dtype in (((37, 64, 8), F16), ((37, 200, 6), F32), ((1030, 8, 2), BF16), ((3, 1000, 64), F32)):
        x = draw_logits(T, E, dtype, T + E).to(d)
        bias = draw_bias(E, 3).to(d) if with_bias else None
        args = (k, scoring, renorm, bias, 1.5)
        ids, w = env.fa.moe_gate(x, *args)
        again = env.fa.moe_gate(x, *args)
        assert same_bits(ids, again[0]) and same_bits(w, again[1])                   # two calls
        assert bool(torch.isfinite(w).all())
        for row in sorted({0, 17 % T, T - 1}):                                       # a row alone = the row in its place
            alone = env.fa.moe_gate(x[row:row + 1].contiguous(), *args)
            assert same_bits(alone[0], ids[row:row + 1]) and same_bits(alone[1], w[row:row + 1]), (T, E, k, row)
        for routed in (env.fa.moe_gate_route(x, k, E, scoring, renorm, bias, 1.5),
                       gate_abi(env, x, k, scoring, renorm, bias, 1.5, routed=True)):
            rids, rw, offsets, rows, row_weight, pos, perm = routed
            assert same_bits(rids, ids) and same_bits(rw, w), (T, E, k, "gate_route's ids / weights are moe_gate's")
            want = env.fa.moe_route(ids, w, E)                                       # (offsets, rows, row_weight, pos, perm)
            for name, a, b in zip(("offsets", "rows", "row_weight", "pos", "perm"), (offsets, rows, row_weight, pos, perm), want):
                assert same_bits(a, b), (T, E, k, name)
            h_off, h_perm, h_rows, h_pos = host_route(ids.reshape(-1).tolist(), k, E)
            assert offsets.tolist() == h_off and perm.tolist() == h_perm and rows.tolist() == h_rows
            assert pos.reshape(-1).tolist() == h_pos
            assert same_bits(row_weight, w.reshape(-1)[perm.long()])


def test_no_tokens(env):
    d = env.dev
    x = torch.empty(0, 6, dtype=F16, device=d)
    ids, w = env.fa.moe_gate(x, 2)
    assert ids.shape == (0, 2) and w.shape == (0, 2)
    out = env.fa.moe_gate_route(x, 2, 6)
    assert out[2].tolist() == [0] * 7 and all(t.numel() == 0 for i, t in enumerate(out) if i != 2)
    assert gate_abi(env, x, 2, routed=True)[2].tolist() == [0] * 7                  # the E + 1 zeros, nothing around them


# ---- 5. the module -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def router(env, top3_case):
    c = top3_case
    gen = torch.Generator().manual_seed(77)
    weight = (torch.randn(c["E"], c["K"], generator=gen) * 0.2).to(c["dtype"]).to(env.dev)
    return weight


GATINGS = [dict(scoring="softmax", renormalize=True, bias=None, scale=1.0),
           dict(scoring="sigmoid", renormalize=False, bias="draw", scale=2.5)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("native_routing", [True, False])
def test_forward_logits_and_block_bit_for_bit(env, top3_case, router, fused, native_routing):
    """forward_logits = forward(hidden, *moe_gate(...)) and the block = forward_logits on F.linear's output, bit for bit.
    With native_routing top-3; without it top-2, because the parent's forward ends in index_add_, whose order of additions -
    and so its bits - is defined for two addends only."""
    c, moe = top3_case, env.moe
    experts = moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused, native_routing=native_routing)
    hidden, k = c["hidden"], c["k"] if native_routing else 2
    logits = torch.nn.functional.linear(hidden, router)
    for g in GATINGS:
        g = dict(g, bias=draw_bias(c["E"], 5).to(env.dev) if g["bias"] is not None else None)
        ids, weights = env.fa.moe_gate(logits, k, g["scoring"], g["renormalize"], g["bias"], g["scale"])
        want = experts(hidden, ids, weights)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        got = experts.forward_logits(hidden, logits, k, **g)
        assert got.shape == (c["T"], c["K"]) and got.dtype == c["dtype"]
        assert torch.equal(bits16(got), bits16(want)), (fused, native_routing, g["scoring"])
        block = moe.FluteSparseMoeBlock(router, experts, k, **g)
        assert torch.equal(bits16(block(hidden)), bits16(got)), (fused, native_routing, g["scoring"])


def test_block_in_a_graph(env, top3_case, router):
    """The router GEMM, moe_gate_route, the two fused launches and moe_combine captured once (capture raises if anything
    reads the routing on the host); a replay on other hidden states returns the bits of an eager call on them."""
    c = top3_case
    block = env.moe.FluteSparseMoeBlock(router, native(env, c, True), c["k"], renormalize=True)
    hidden = c["hidden"].clone()
    first = block(hidden).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = block(hidden)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(first))
    other = (c["hidden"].flip(0) * 1.5).contiguous()
    hidden.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = block(other)
    assert torch.equal(bits16(y), bits16(eager))
    assert not torch.equal(bits16(eager), bits16(first))


def test_an_unreachable_expert_has_an_empty_range(env, top3_case, router):
    c = top3_case
    E, k = c["E"], c["k"]
    logits = torch.nn.functional.linear(c["hidden"], router)
    bias = torch.zeros(E)
    bias[2] = -1.0e4                                                    # expert 2 is the one left out of every top-3
    out = env.fa.moe_gate_route(logits, k, E, "softmax", True, bias.to(env.dev))
    ids, offsets = out[0], out[2].tolist()
    assert 2 not in ids.cpu().reshape(-1).tolist()
    assert offsets[2] == offsets[3] and offsets[E] == c["T"] * k and offsets[3] > 0
    experts = native(env, c, True)
    block = env.moe.FluteSparseMoeBlock(router, experts, k, renormalize=True, bias=bias.to(env.dev))
    y = block(c["hidden"])
    assert bool(torch.isfinite(y).all())
    assert torch.equal(bits16(y), bits16(experts(c["hidden"], out[0], out[1])))


# ---- 6. against the chain users run today ------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,E,k", [(5, 60, 4), (37, 64, 8), (1030, 8, 2)])
def test_ids_equal_torch_topk_of_softmax(env, T, E, k):
    """Where the fp32 probabilities are separated (the 2^-16 condition on the softmax), torch.topk has one answer, and it
    is the contract's."""
    x = draw_separated(T, E, k, F32, "softmax", None, 31 * T + E, key_of=lambda v: R.scores(v, "softmax"))
    xd = x.to(env.dev)
    values, want = torch.topk(torch.softmax(xd.float(), dim=1), k, dim=1)
    ids, w = env.fa.moe_gate(xd, k)
    assert torch.equal(ids.long(), want)
    assert torch.equal(ids.cpu().long(), R.gate(x, k)[0])
    routed = env.fa.moe_gate_route(xd, k, E)
    assert torch.equal(routed[0].long(), want)
