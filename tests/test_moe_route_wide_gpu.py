"""flute_amd.moe_route_wide / moe_gate_route_wide (moe_route_wide.hip, moe_gate.hip) and FluteExperts(wide_routing=...) on
the GPU.

The multi-workgroup routing promises the one-workgroup routing's outputs bit for bit, so every comparison here is exact:
integers value for value, floats by their bits.  The yardsticks are the routing contract as a host loop
(tests/moe_cases.py host_route) and the one-workgroup ops (`moe_route`, `moe_gate_route`, `moe_gate_route_limited`), which
their own tests hold against the contract.  Direct ABI calls put every output in a canary-padded buffer and the workspace
between canaries, poisoned - 0xFF bytes on one call, 0x5A on the next - so that a word of it read before it was written
shows.  Shapes are tiny: several chunks, ragged last chunks, chunks smaller than a wave's step, waves that walk their range
twice, LDS above 64 KB."""
import pytest
import torch

from tests.moe_cases import native, top3_case  # noqa: F401
from tests.moe_wide_cases import (GATE_WIDE_CASES, ROUTE_WIDE_CASES, draw_bias, draw_logits, draw_wide_ids, gate_route_wide_abi,
                                  host_route, poisoned_workspace, route_wide_abi, same_bits)
from tests.support import bits16, env, first_template  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
I32, I64 = torch.int32, torch.int64
NAMES5 = ("offsets", "rows", "row_weight", "pos", "perm")
NAMES7 = ("ids", "weights") + NAMES5


def assert_same(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(NAMES5 if len(got) == 5 else NAMES7, got, want):
        if b is None:
            assert a is None, (what, name)
        else:
            assert same_bits(a, b), (what, name)


# ---- 1. moe_route_wide against moe_route and the host loop -----------------------------------------------------------------

def check_route_wide(env, ids_host, E, chunk_tokens, widths=(I32,), weight_dtypes=(F32,)):
    """ids_host [T, k] int64 on the host: the direct call and flute_amd.moe_route_wide against the host loop, value for value,
    and against flute_amd.moe_route, bit for bit."""
    d = env.dev
    T, k = ids_host.shape
    P = T * k
    want_off, want_perm, want_rows, want_pos = host_route(ids_host.reshape(-1).tolist(), k, E)
    w_host = torch.randn(T, k, generator=torch.Generator().manual_seed(P + E))
    for width in widths:
        ids = ids_host.to(width).to(d)
        for wd in weight_dtypes:
            weights = None if wd is None else w_host.to(wd).to(d)
            one = env.fa.moe_route(ids, weights, E)
            for got in (route_wide_abi(env, ids, weights, E, chunk_tokens), env.fa.moe_route_wide(ids, weights, E, chunk_tokens)):
                what = (T, k, E, chunk_tokens, width, wd)
                offsets, rows, row_weight, pos, perm = got
                assert offsets.tolist() == want_off, what
                assert perm.tolist() == want_perm, what
                assert rows.tolist() == want_rows, what
                assert pos.reshape(-1).tolist() == want_pos, what
                assert (row_weight is None) == (wd is None)
                assert_same(got, one, what)


@pytest.mark.parametrize("T,k,E,chunk_tokens", ROUTE_WIDE_CASES)
def test_route_wide_is_moe_route(env, T, k, E, chunk_tokens):
    check_route_wide(env, draw_wide_ids(T, k, E, chunk_tokens, 500 + T + E), E, chunk_tokens)


def test_route_wide_id_widths_and_weight_types(env):
    T, k, E, ct = 37, 2, 4, 16
    check_route_wide(env, draw_wide_ids(T, k, E, ct, 9), E, ct, widths=(I32, I64), weight_dtypes=(F16, BF16, F32, None))


def test_route_wide_no_pairs_writes_the_zeros(env):
    for T, k in ((0, 2), (3, 0)):
        for ct in (None, 1, 4):
            check_route_wide(env, torch.zeros(T, k, dtype=I64), 6, ct, weight_dtypes=(F16, None))


# ---- 2. hostile routings ---------------------------------------------------------------------------------------------------

def test_route_wide_hostile_routings(env):
    T, k, E, ct = 261, 8, 256, 16                                   # 17 chunks of 128 pairs, the last of 40
    check_route_wide(env, torch.full((T, k), E - 1), E, ct)         # every pair to the last expert
    check_route_wide(env, torch.zeros(T, k, dtype=I64), E, ct)      # to expert 0: every chunk's base is one bucket's running count
    ids = draw_wide_ids(T, k, E, ct, 61)
    ids[2, 3], ids[40, 0], ids[100, 7], ids[250, 1] = -1, E, 2 ** 32 + 1, -2 ** 32       # chunks 0, 2, 6, 15
    check_route_wide(env, ids, E, ct, widths=(I64,))
    narrow = ids.clone()
    narrow[100, 7], narrow[250, 1] = E + 1, -7
    check_route_wide(env, narrow, E, ct, widths=(I32, I64))
    invalid = draw_wide_ids(T, k, E, ct, 62)
    invalid[48:64] = -1                                             # chunk 3 entirely outside
    invalid[260] = E                                                # and the ragged last one, one token of it
    check_route_wide(env, invalid, E, ct)
    single = draw_wide_ids(T, k, E, ct, 63)
    single[80:96] = 17                                              # chunk 5 entirely one expert
    check_route_wide(env, single, E, ct)


# ---- 3. a workspace that holds an earlier call's figures ---------------------------------------------------------------------

def test_route_wide_on_a_stale_workspace(env):
    d = env.dev
    big = draw_wide_ids(261, 8, 256, 16, 71).to(I32).to(d)
    small_host = draw_wide_ids(37, 2, 4, 16, 72)
    small = small_host.to(I32).to(d)
    w = torch.randn(37, 2, generator=torch.Generator().manual_seed(3)).to(d)
    ws = poisoned_workspace(env, env.lib.flute_moe_route_wide_workspace(261, 8, 256, 16))
    route_wide_abi(env, big, None, 256, 16, workspace=ws)
    again = route_wide_abi(env, small, w, 4, 16, workspace=ws)       # the same tensor, not cleared in between
    fresh = route_wide_abi(env, small, w, 4, 16)
    assert_same(again, fresh, "stale workspace")
    assert again[0].tolist() == host_route(small_host.reshape(-1).tolist(), 2, 4)[0]
    third = route_wide_abi(env, big, None, 256, 16, workspace=ws)    # and back: larger after smaller
    assert_same(third, env.fa.moe_route(big, None, 256), "stale workspace, larger again")


# ---- 4. moe_gate_route_wide: all seven arrays --------------------------------------------------------------------------------

@pytest.mark.parametrize("T,E,k,chunk_tokens", GATE_WIDE_CASES)
def test_gate_route_wide_is_moe_gate_route(env, T, E, k, chunk_tokens):
    d = env.dev
    logits = draw_logits(T, E, F16, 800 + T + E).to(d)
    bias = draw_bias(E, 5).to(d)
    for scoring, renorm, b, scale in (("softmax", False, None, 1.0), ("sigmoid", True, bias, 2.5)):
        want = env.fa.moe_gate_route(logits, k, E, scoring, renorm, b, scale)
        what = (T, E, k, chunk_tokens, scoring)
        assert_same(gate_route_wide_abi(env, logits, k, chunk_tokens, scoring, renorm, b, scale), want, what)
        assert_same(env.fa.moe_gate_route_wide(logits, k, E, scoring, renorm, b, scale, chunk_tokens=chunk_tokens), want, what)
        # every group allowed: the unlimited gating, whatever the group score
        assert_same(gate_route_wide_abi(env, logits, k, chunk_tokens, scoring, renorm, b, scale, n_group=1, topk_group=1,
                                        group_score="top2sum" if E > 1 else "max"), want, what)


@pytest.mark.parametrize("chunk_tokens", [16, 32])
def test_gate_route_wide_limited_is_moe_gate_route_limited(env, chunk_tokens):
    d = env.dev
    T, E, k, n_group, topk_group = 70, 256, 8, 8, 4
    logits = draw_logits(T, E, BF16, 31).to(d)
    bias = (draw_bias(E, 6) * 0.1).to(d)
    args = ("sigmoid", True, bias, 2.5)
    want = env.fa.moe_gate_route_limited(logits, k, n_group, topk_group, E, *args, "top2sum")
    assert len(set((want[0] // 32).reshape(-1).tolist())) > topk_group                 # the groups differ over the tokens
    assert not same_bits(want[0], env.fa.moe_gate_route(logits, k, E, *args)[0])       # and the limit changes the choice
    got = gate_route_wide_abi(env, logits, k, chunk_tokens, *args, n_group=n_group, topk_group=topk_group, group_score="top2sum")
    assert_same(got, want, chunk_tokens)
    got = env.fa.moe_gate_route_wide(logits, k, E, *args, n_group, topk_group, "top2sum", chunk_tokens)
    assert_same(got, want, chunk_tokens)
    assert got[2].tolist() == host_route(got[0].reshape(-1).tolist(), k, E)[0]


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
def test_gate_route_wide_logit_types(env, dtype):
    logits = draw_logits(37, 64, dtype, 41).to(env.dev)
    want = env.fa.moe_gate_route(logits, 8, 64, "softmax", True)
    assert_same(gate_route_wide_abi(env, logits, 8, 16, "softmax", True), want, dtype)


def test_gate_route_wide_all_logits_equal(env):
    """The ids come from the tie rule alone: experts 0 .. k - 1 in every token, so every chunk sends its pairs to the same buckets."""
    logits = torch.full((37, 64), 0.25, dtype=F16, device=env.dev)
    got = gate_route_wide_abi(env, logits, 8, 16)
    assert got[0].tolist() == [list(range(8))] * 37
    assert_same(got, env.fa.moe_gate_route(logits, 8, 64), "ties")
    assert got[2].tolist() == [37 * e for e in range(8)] + [37 * 8] * 57


def test_gate_route_wide_a_token_does_not_depend_on_its_row(env):
    d = env.dev
    base = draw_logits(37, 64, F16, 43)
    token = draw_logits(1, 64, F16, 44)
    alone = env.fa.moe_gate_route(token.to(d), 8, 64, "softmax", True)
    for row in (0, 17, 36):
        logits = base.clone()
        logits[row] = token[0]
        ids, weights = gate_route_wide_abi(env, logits.to(d), 8, 16, "softmax", True)[:2]
        assert same_bits(ids[row], alone[0][0]) and same_bits(weights[row], alone[1][0]), row


# ---- 5. graphs ---------------------------------------------------------------------------------------------------------------

def test_wide_ops_in_a_graph(env):
    """Both ops captured once (capture raises if anything reads on the host; the workspace comes from the graph's pool) and
    replayed on other inputs: the bits of an eager call on them."""
    d = env.dev
    logits = draw_logits(70, 64, F16, 51).to(d)
    other = draw_logits(70, 64, F16, 52).to(d)
    ids = draw_wide_ids(70, 4, 64, 16, 53).to(d)
    other_ids = draw_wide_ids(70, 4, 64, 16, 54).to(d)
    w = torch.randn(70, 4, generator=torch.Generator().manual_seed(5)).to(d)
    x, i = logits.clone(), ids.clone()
    env.fa.moe_gate_route_wide(x, 4, 64, chunk_tokens=16)
    env.fa.moe_route_wide(i, w, 64, chunk_tokens=16)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gated = env.fa.moe_gate_route_wide(x, 4, 64, chunk_tokens=16)
        routed = env.fa.moe_route_wide(i, w, 64, chunk_tokens=16)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(gated, env.fa.moe_gate_route(logits, 4, 64), "captured")
    assert_same(routed, env.fa.moe_route(ids, w, 64), "captured")
    x.copy_(other)
    i.copy_(other_ids)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(gated, env.fa.moe_gate_route(other, 4, 64), "replayed")
    assert_same(routed, env.fa.moe_route(other_ids, w, 64), "replayed")
    assert not same_bits(gated[0], env.fa.moe_gate_route(logits, 4, 64)[0])


# ---- 6. autograd -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("native_router_grad", [False, True])
def test_gate_route_wide_backward_is_moe_gate_route_s(env, native_router_grad):
    d = env.dev
    T, E, k = 37, 64, 8
    logits = draw_logits(T, E, F32, 61).to(d)
    gen = torch.Generator().manual_seed(62)
    d_weights, d_row_weight = torch.randn(T, k, generator=gen).to(d), torch.randn(T * k, generator=gen).to(d)
    grads = []
    for wide in (None, 16):
        x = logits.clone().requires_grad_()
        outs = env.fa.ops._moe_gate_entry(x, k, "softmax", True, None, 1.5, routed=True, num_experts=E,
                                          native_router_grad=native_router_grad, wide=wide)
        torch.autograd.backward([outs[1], outs[4]], [d_weights, d_row_weight])
        grads.append(x.grad)
    assert float(grads[0].abs().max()) > 0 and same_bits(grads[0], grads[1])
    if not native_router_grad:                                       # the public op is that entry
        x = logits.clone().requires_grad_()
        outs = env.fa.moe_gate_route_wide(x, k, E, "softmax", True, None, 1.5, chunk_tokens=16)
        torch.autograd.backward([outs[1], outs[4]], [d_weights, d_row_weight])
        assert same_bits(x.grad, grads[0])


def test_route_wide_backward_is_moe_route_s(env):
    d = env.dev
    ids = draw_wide_ids(37, 2, 4, 16, 65).to(d)
    w = torch.randn(37, 2, generator=torch.Generator().manual_seed(66)).to(F16).to(d)
    d_row_weight = torch.randn(74, generator=torch.Generator().manual_seed(67)).to(d)
    grads = []
    for route in (env.fa.moe_route, lambda *a: env.fa.moe_route_wide(*a, chunk_tokens=16)):
        wg = w.clone().requires_grad_()
        route(ids, wg, 4)[2].backward(d_row_weight)
        grads.append(wg.grad)
    assert grads[0].dtype == F16 and float(grads[0].abs().max()) > 0
    assert torch.equal(bits16(grads[0]), bits16(grads[1]))


# ---- 7. the module -----------------------------------------------------------------------------------------------------------

def experts_of(env, c, fused, wide_routing, **kw):
    return env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused, native_routing=True,
                                             wide_routing=wide_routing, **kw)


@pytest.fixture(scope="module")
def eight_experts_case(env):
    """E = 8 experts (4-bit, g = 64, K = 256, N_ff = 512), T = 37 tokens: two groups of four for the limited form."""
    d, dtype = env.dev, F16
    E, K, F, T, bits, g = 8, 256, 512, 37, 4, 64
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(34)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, dtype=dtype)
    c["gates"], c["ups"], c["downs"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)],
                                        [linear(F, K) for _ in range(E)])
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    return c


def router_of(env, c, seed):
    return (torch.randn(c["E"], c["K"], generator=torch.Generator().manual_seed(seed)) * 0.2).to(c["dtype"]).to(env.dev)


@pytest.mark.parametrize("fused", [True, False])
def test_module_forwards_bit_for_bit(env, top3_case, eight_experts_case, fused):
    """forward, forward_logits, forward_logits_limited and the block with wide_routing=True against wide_routing=False.  37 tokens:
    three chunks in the gated form; the ungated automatic chunk holds them all, so `forward` is also run with the op's chunk of 16."""
    c = top3_case
    hidden, ids, weights, k = c["hidden"], c["ids"], c["weights"], c["k"]
    one, wide = experts_of(env, c, fused, False), experts_of(env, c, fused, True)
    assert one.wide_routing is False and wide.wide_routing is True
    want = one(hidden, ids, weights)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    assert torch.equal(bits16(wide(hidden, ids, weights)), bits16(want))
    offsets, rows, row_weight, pos, _ = env.fa.moe_route_wide(ids, weights, c["E"], chunk_tokens=16)
    assert torch.equal(bits16(wide._forward_routed(hidden, offsets, rows, row_weight, pos)), bits16(want))
    router = router_of(env, c, 77)
    logits = torch.nn.functional.linear(hidden, router)
    bias = (draw_bias(c["E"], 5) * 0.25).to(env.dev)
    for g in (dict(scoring="softmax", renormalize=True), dict(scoring="sigmoid", renormalize=True, bias=bias, scale=2.5)):
        want = one.forward_logits(hidden, logits, k, **g)
        assert torch.equal(bits16(wide.forward_logits(hidden, logits, k, **g)), bits16(want)), g["scoring"]
        block = env.moe.FluteSparseMoeBlock(router, wide, k, **g)
        assert torch.equal(bits16(block(hidden)), bits16(want)), g["scoring"]
    # the limited form: E = 8, two groups of four, the better one allowed
    c = eight_experts_case
    hidden = c["hidden"]
    one, wide = experts_of(env, c, fused, False), experts_of(env, c, fused, True)
    router = router_of(env, c, 78)
    logits = torch.nn.functional.linear(hidden, router)
    bias = (draw_bias(c["E"], 7) * 0.25).to(env.dev)
    for g in (dict(scoring="softmax", renormalize=True, group_score="max"),
              dict(scoring="sigmoid", renormalize=True, bias=bias, scale=2.5, group_score="top2sum")):
        want = one.forward_logits_limited(hidden, logits, 3, 2, 1, **g)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        assert torch.equal(bits16(wide.forward_logits_limited(hidden, logits, 3, 2, 1, **g)), bits16(want)), g["scoring"]
        assert not torch.equal(bits16(one.forward_logits(hidden, logits, 3, g["scoring"], True, g.get("bias"), g.get("scale", 1.0))),
                               bits16(want))
        block = env.moe.FluteSparseMoeBlock(router, wide, 3, n_group=2, topk_group=1, **g)
        assert torch.equal(bits16(block(hidden)), bits16(want)), g["scoring"]


@pytest.mark.parametrize("native_router_grad", [False, True])
@pytest.mark.parametrize("limited", [False, True])
def test_block_gradients_bit_for_bit(env, top3_case, eight_experts_case, limited, native_router_grad):
    """hidden.grad and router_weight.grad of the block (fused: every sum over a token's slots is moe_combine's, in slot order)."""
    c = eight_experts_case if limited else top3_case
    groups = dict(n_group=2, topk_group=1, group_score="top2sum") if limited else {}
    dOut = torch.randn(c["T"], c["K"], generator=torch.Generator().manual_seed(81)).to(c["dtype"]).to(env.dev)
    got = []
    for wide_routing in (False, True):
        experts = experts_of(env, c, True, wide_routing, native_router_grad=native_router_grad)
        block = env.moe.FluteSparseMoeBlock(router_of(env, c, 79), experts, 3, scoring="sigmoid", renormalize=True, scale=2.5,
                                            **groups)
        block.router_weight.requires_grad_()
        h = c["hidden"].clone().requires_grad_()
        out = block(h)
        out.backward(dOut)
        got.append((out.detach(), h.grad, block.router_weight.grad))
    for name, a, b in zip(("out", "hidden.grad", "router_weight.grad"), *got):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert torch.equal(bits16(a), bits16(b)), (name, limited, native_router_grad)


def test_wide_block_in_a_graph(env, top3_case):
    c = top3_case
    block = env.moe.FluteSparseMoeBlock(router_of(env, c, 77), experts_of(env, c, True, True), 3, scoring="softmax", renormalize=True)
    plain = env.moe.FluteSparseMoeBlock(router_of(env, c, 77), experts_of(env, c, True, False), 3, scoring="softmax", renormalize=True)
    hidden = c["hidden"].clone()
    first = block(hidden).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = block(hidden)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(first)) and torch.equal(bits16(first), bits16(plain(c["hidden"])))
    other = (c["hidden"].flip(0) * 1.5).contiguous()
    hidden.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(plain(other)))
    assert not torch.equal(bits16(y), bits16(first))


def test_auto_takes_the_form_the_rule_names(env, top3_case, monkeypatch):
    """wide_routing="auto" asks flute_amd.dev.moe_route_form with the call's shapes: which routing op ran, by spying on the ops.  On
    each side of the rule's threshold where that is at most 64 tokens, else on the "one" side with the other side's answer asserted
    on the host."""
    c, fa = top3_case, env.fa
    E, k = c["E"], c["k"]
    form = env.dev_mod.moe_route_form
    assert form(1, k, E) == "one" and form(16384, k, E) == "wide" and form(16384, k, E, gated=False) == "wide"
    calls = []
    for real in (fa.moe_route, fa.moe_route_wide, fa.moe_gate_route, fa.moe_gate_route_wide):   # the module looks them up when it runs
        monkeypatch.setattr(fa, real.__name__, lambda *a, _real=real, **kw: calls.append(_real.__name__) or _real(*a, **kw))
    auto, one = experts_of(env, c, True, "auto"), experts_of(env, c, True, False)
    router = router_of(env, c, 77)
    gen = torch.Generator().manual_seed(91)
    for gated in (True, False):
        first_wide = next((T for T in range(1, 65) if form(T, k, E, gated=gated) == "wide"), None)
        tokens = [c["T"]] if first_wide is None else [first_wide - 1, first_wide]
        for T in tokens:
            hidden = torch.randn(T, c["K"], generator=gen).to(c["dtype"]).to(env.dev)
            logits = torch.nn.functional.linear(hidden, router)
            with torch.no_grad():
                ids, weights = fa.moe_gate(logits, k, "softmax", True)
            del calls[:]
            got = auto.forward_logits(hidden, logits, k, "softmax", True) if gated else auto(hidden, ids, weights)
            name = ("moe_gate_route" if gated else "moe_route") + ("_wide" if form(T, k, E, gated=gated) == "wide" else "")
            assert calls == [name], (gated, T, calls)
            want = one.forward_logits(hidden, logits, k, "softmax", True) if gated else one(hidden, ids, weights)
            assert torch.equal(bits16(got), bits16(want)), (gated, T)
