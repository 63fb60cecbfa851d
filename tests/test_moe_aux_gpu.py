"""flute_amd.moe_aux_loss / moe_aux_loss_grad (moe_aux.hip) and FluteSparseMoeBlock with aux_loss on on the GPU: exact cases bit
for bit, random data inside the derived bounds of tests/moe_aux_cases.py against the fp64 restatement (the worst ratio of every
case is printed), the backward's edges, hostile operands, canaries around every output with the workspace poisoned, equal bits
over two calls and in a replayed graph, and the wiring up to the block.

One wave takes one token and lane l the experts l, l + 64, ...: E = 8, 64 (one register), 160 (not a multiple of 64), 256, 1000
cover the five classes; T = 1 and 5 leave waves without a token, 257 and 513 are one token past an automatic chunk's edge."""
import math

import pytest
import torch

from tests import moe_aux_cases as AC
from tests.grouped_cases import experts_case  # noqa: F401
from tests.moe_cases import same_bits
from tests.support import bits16, bits32, bits_by_size, env, fp32_blas_reduction  # noqa: F401

pytestmark = pytest.mark.gpu
F16, BF16, F32 = AC.F16, AC.BF16, AC.F32
DTYPE_IDS = ["f16", "bf16", "f32"]


def on(env, *ts):
    return tuple(t.to(env.dev) for t in ts)


def grads_on(env, g_b, g_z):
    return torch.tensor([g_b, g_z], dtype=torch.float32, device=env.dev)


# ---------------------------------------------------------------------------
# 1. exact cases
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("chunk_tokens", [None, 100, 1])
def test_zero_logits_are_exact(env, dtype, chunk_tokens):
    """p = 1/64 everywhere, every expert is named by 8 slots: load = 8, importance = 256 / 64 = 4 and balance = 64 * 64 * (8 / 256)
    * (4 / 256) = 2, every intermediate a power of two (or a sum of equal powers of two below 2^24 of them), so any order of
    additions gives these bits.  z = log(64)^2 within its bound."""
    T, E = 256, 64
    logits = torch.zeros(T, E, dtype=dtype, device=env.dev)
    t = torch.arange(T)
    ids = torch.stack([(2 * t) % E, (2 * t + 1) % E], dim=1).int().to(env.dev)
    for got in (env.fa.moe_aux_loss(logits, ids, "softmax", chunk_tokens), AC.aux_loss_abi(env, logits, ids, "softmax", chunk_tokens)):
        balance, z, load, importance = got
        assert load.dtype == torch.int32 and torch.equal(load.cpu(), torch.full((E,), 8, dtype=torch.int32))
        assert same_bits(importance.cpu(), torch.full((E,), 4.0)) and same_bits(balance.cpu().reshape(1), torch.tensor([2.0]))
        ref = math.log(64.0) ** 2
        assert abs(float(z) - ref) <= 2 * AC.XC.gamma(T + E + 16) * ref


def test_load_is_the_routing_count(env):
    """load against torch.bincount and against the differences of moe_route's offsets, exactly, with ids outside [0, E) - -1, E,
    2^31 - 1 - that count nowhere; the same for every chunk_tokens, and equal bits on a second call."""
    for T, E, k in ((37, 4, 2), (300, 160, 6), (130, 1000, 8)):
        gen = torch.Generator().manual_seed(T)
        ids = torch.randint(0, E, (T, k), generator=gen).int()
        flat = ids.view(-1)
        flat[torch.randperm(T * k, generator=gen)[:9]] = torch.tensor([-1, E, 2 ** 31 - 1] * 3, dtype=torch.int32)
        want = AC.load_of(ids, E).int()
        assert int(want.sum()) == T * k - 9
        logits, ids = on(env, AC.draw(T, E, k, 2.0, F32, T + 1)[0], ids)
        offsets = env.fa.moe_route(ids, None, E)[0]
        assert torch.equal(offsets.diff().cpu(), want)
        first = None
        for chunk_tokens in (None, 1, 7, 64, T):
            got = env.fa.moe_aux_loss(logits, ids, "sigmoid", chunk_tokens)
            assert torch.equal(got[2].cpu(), want), (T, E, chunk_tokens)
            again = env.fa.moe_aux_loss(logits, ids, "sigmoid", chunk_tokens)
            assert all(same_bits(a, b) for a, b in zip(got, again))
            first = first or got
            assert torch.equal(got[2], first[2])


# ---------------------------------------------------------------------------
# 2. random data inside the derived bounds
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=AC.SHAPE_IDS)
def test_forward_random(env, shape, dtype):
    """Automatic and forced chunking, both scorings, through the op and through the direct call with canaries and a poisoned
    workspace: the two paths give equal bits, load is exact and the same across the chunkings, the three float results are inside
    their bounds."""
    T, E, k, spread, forced = shape
    for scoring in AC.SCORINGS:
        logits, ids = AC.draw(T, E, k, spread, dtype, 1000 + T + E)
        ref, bounds = AC.forward_bounds(logits, ids, scoring)
        logits, ids = on(env, logits, ids)
        for chunk_tokens in (None, forced):
            got = env.fa.moe_aux_loss(logits, ids, scoring, chunk_tokens)
            direct = AC.aux_loss_abi(env, logits, ids, scoring, chunk_tokens)
            assert all(same_bits(a, b) for a, b in zip(got, direct))
            balance, z, load, importance = (t.cpu() for t in got)
            assert balance.shape == () and z.shape == () and balance.dtype == z.dtype == importance.dtype == torch.float32
            assert torch.equal(load.long(), ref[2])
            ratios = (AC.worst_ratio(balance, ref[0], bounds[0]), AC.worst_ratio(z, ref[1], bounds[1]),
                      AC.worst_ratio(importance, ref[3], bounds[2]))
            print("moe_aux_loss %s %s T=%d E=%d k=%d chunk_tokens=%s: error / bound balance %.3f z %.3f importance %.3f"
                  % (scoring, dtype, T, E, k, chunk_tokens, *ratios))
            assert max(ratios) <= 1.0, (scoring, chunk_tokens, ratios)


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", AC.SHAPES, ids=AC.SHAPE_IDS)
def test_backward_random(env, shape, dtype):
    """d_logits through the op and through the direct call - the output pre-filled with NaN bits between canaries: every element
    is written - inside the bound per element; gradients of either sign."""
    T, E, k, spread, _ = shape
    for scoring in AC.SCORINGS:
        logits, ids = AC.draw(T, E, k, spread, dtype, 2000 + T + E)
        load = AC.load_of(ids, E)
        g_b, g_z = (float(g) for g in AC.draw_grads(3000 + T + E + len(scoring)))
        ref, bound = AC.backward_bound(logits, load, g_b, g_z, scoring)
        logits, load32 = on(env, logits, load.int())
        grads = grads_on(env, g_b, g_z)
        got = env.fa.moe_aux_loss_grad(logits, load32, grads, scoring)
        direct = AC.aux_grad_abi(env, logits, load32, grads, scoring)
        assert got.dtype == dtype and got.shape == (T, E) and same_bits(bits_by_size(got), bits_by_size(direct))
        assert torch.isfinite(got).all()
        ratio = AC.worst_ratio(got.cpu(), ref, bound)
        print("moe_aux_loss_grad %s %s T=%d E=%d g_b=%.2f g_z=%.2f: error / bound %.3f" % (scoring, dtype, T, E, g_b, g_z, ratio))
        assert ratio <= 1.0, (scoring, ratio)


# ---------------------------------------------------------------------------
# 3. the backward's edges and autograd
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
def test_backward_edges(env, dtype):
    """grads = (0, 0): every element +0; either gradient alone, and both negative: inside the bound."""
    T, E, k = 37, 72, 4
    for scoring in AC.SCORINGS:
        logits, ids = AC.draw(T, E, k, 3.0, dtype, 41)
        load = AC.load_of(ids, E)
        dl, dload = on(env, logits, load.int())
        zero = env.fa.moe_aux_loss_grad(dl, dload, grads_on(env, 0.0, 0.0), scoring)
        assert not bits_by_size(zero).any()
        assert not bits_by_size(AC.aux_grad_abi(env, dl, dload, grads_on(env, 0.0, 0.0), scoring)).any()
        for g_b, g_z in ((1.5, 0.0), (0.0, 0.75), (-2.0, -0.5), (-1.0, 0.0), (0.0, -3.0)):
            ref, bound = AC.backward_bound(logits, load, g_b, g_z, scoring)
            got = env.fa.moe_aux_loss_grad(dl, dload, grads_on(env, g_b, g_z), scoring)
            ratio = AC.worst_ratio(got.cpu(), ref, bound)
            print("moe_aux_loss_grad edges %s %s g_b=%.2f g_z=%.2f: error / bound %.3f" % (scoring, dtype, g_b, g_z, ratio))
            assert ratio <= 1.0 and float(got.float().abs().max()) > 0


@pytest.mark.parametrize("scoring", AC.SCORINGS)
def test_autograd(env, scoring):
    """balance and z under autograd: the backward is the grad op on the stacked incoming gradients, a missing one 0; load and
    importance carry no gradient; a double backward raises."""
    T, E, k = 37, 72, 4
    logits, ids = on(env, *AC.draw(T, E, k, 3.0, F32, 43))
    x = logits.clone().requires_grad_()
    balance, z, load, importance = env.fa.moe_aux_loss(x, ids, scoring)
    plain = env.fa.moe_aux_loss(logits, ids, scoring)
    assert all(same_bits(a.detach(), b) for a, b in zip((balance, z, load, importance), plain))
    assert balance.requires_grad and z.requires_grad and not load.requires_grad and not importance.requires_grad
    for loss, g in ((balance * 1.5, (1.5, 0.0)), (z * -0.25, (0.0, -0.25)), (2.0 * balance + 0.5 * z, (2.0, 0.5))):
        (dx,) = torch.autograd.grad(loss, x, retain_graph=True)
        assert same_bits(dx, env.fa.moe_aux_loss_grad(logits, load, grads_on(env, *g), scoring))
    (dx,) = torch.autograd.grad(balance + z, x, create_graph=True)
    with pytest.raises(RuntimeError):
        dx.sum().backward()


# ---------------------------------------------------------------------------
# 4. hostile operands
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
def test_masked_experts(env, dtype):
    """-infinity on some experts of every token: their p and d_logits are exactly +0, everything else finite and inside the
    bounds."""
    T, E, k = 70, 160, 6
    masked = torch.tensor([0, 5, 63, 64, 100, 159])
    for scoring in AC.SCORINGS:
        logits, ids = AC.draw(T, E, k, 2.5, dtype, 51)
        logits[:, masked] = float("-inf")
        ref, bounds = AC.forward_bounds(logits, ids, scoring)
        dref, dbound = AC.backward_bound(logits, ref[2], 1.25, -0.5, scoring)
        dl, dids = on(env, logits, ids)
        for chunk_tokens in (None, 24):
            balance, z, load, importance = (t.cpu() for t in env.fa.moe_aux_loss(dl, dids, scoring, chunk_tokens))
            assert not bits32(importance[masked]).any() and torch.isfinite(importance).all()
            assert torch.isfinite(balance) and torch.isfinite(z) and torch.equal(load.long(), ref[2])
            ratios = (AC.worst_ratio(balance, ref[0], bounds[0]), AC.worst_ratio(z, ref[1], bounds[1]),
                      AC.worst_ratio(importance, ref[3], bounds[2]))
            assert max(ratios) <= 1.0, (scoring, ratios)
        got = env.fa.moe_aux_loss_grad(dl, load.to(env.dev), grads_on(env, 1.25, -0.5), scoring).cpu()
        assert not bits_by_size(got[:, masked]).any() and torch.isfinite(got).all()
        ratio = AC.worst_ratio(got, dref, dbound)
        print("masked experts %s %s: forward %.3f %.3f %.3f backward %.3f" % (scoring, dtype, *ratios, ratio))
        assert ratio <= 1.0


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_fp16_range_edge(env, dtype):
    """Logits of +-65504, at least one +65504 per token: every result is finite."""
    T, E, k = 37, 72, 4
    gen = torch.Generator().manual_seed(61)
    logits = torch.where(torch.rand(T, E, generator=gen) < 0.5, 65504.0, -65504.0)
    logits[torch.arange(T), torch.randint(0, E, (T,), generator=gen)] = 65504.0
    _, ids = AC.draw(T, E, k, 1.0, dtype, 62)
    dl, dids = on(env, logits.to(dtype), ids)
    for scoring in AC.SCORINGS:
        balance, z, load, importance = env.fa.moe_aux_loss(dl, dids, scoring, 16)
        assert torch.isfinite(balance) and torch.isfinite(z) and torch.isfinite(importance).all() and float(z) > 65504.0 ** 2 * 0.99
        assert torch.equal(load.cpu().long(), AC.load_of(ids, E))
        got = env.fa.moe_aux_loss_grad(dl, load, grads_on(env, 1.0, 1e-6), scoring)
        assert torch.isfinite(got).all()


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
def test_a_nan_row(env, dtype):
    """One token row of NaN: importance, balance and z are NaN, load is unchanged, and the d_logits rows of every other token are
    bit for bit those of the clean run."""
    T, E, k, row = 37, 72, 4, 11
    for scoring in AC.SCORINGS:
        logits, ids = on(env, *AC.draw(T, E, k, 3.0, dtype, 71))
        bad = logits.clone()
        bad[row] = float("nan")
        clean = env.fa.moe_aux_loss(logits, ids, scoring, 8)
        balance, z, load, importance = env.fa.moe_aux_loss(bad, ids, scoring, 8)
        assert torch.isnan(balance) and torch.isnan(z) and torch.isnan(importance).all()
        assert torch.equal(load, clean[2])
        grads = grads_on(env, 1.5, -0.75)
        want = env.fa.moe_aux_loss_grad(logits, load, grads, scoring)
        got = env.fa.moe_aux_loss_grad(bad, load, grads, scoring)
        keep = torch.arange(T, device=env.dev) != row
        assert torch.equal(bits_by_size(got)[keep], bits_by_size(want)[keep]) and torch.isnan(got[row]).all()


# ---------------------------------------------------------------------------
# 5. a replayed graph
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DTYPE_IDS)
def test_equal_bits_in_a_replayed_graph(env, dtype):
    """Forward and backward captured on one stream, replayed after the logits changed in place: bit for bit the eager run."""
    T, E, k = 257, 160, 6
    logits, ids = on(env, *AC.draw(T, E, k, 2.5, dtype, 81))
    logits2, ids2 = on(env, *AC.draw(T, E, k, 5.0, dtype, 82))
    grads = grads_on(env, 1.5, -0.75)

    def run():
        balance, z, load, importance = env.fa.moe_aux_loss(logits, ids, "sigmoid", 100)
        return balance, z, load, importance, env.fa.moe_aux_loss_grad(logits, load, grads, "sigmoid")

    same = lambda xs, ys: all(torch.equal(bits_by_size(a), bits_by_size(b)) for a, b in zip(xs, ys))
    first = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    graph.replay()
    torch.cuda.synchronize()
    assert same(outs, first)
    logits.copy_(logits2)
    ids.copy_(ids2)
    grads.copy_(grads_on(env, -0.5, 2.0))
    eager = [t.clone() for t in run()]
    assert not same(eager[:1], first[:1]) and not same(eager[4:], first[4:])
    graph.replay()
    torch.cuda.synchronize()
    assert same(outs, eager)


# ---------------------------------------------------------------------------
# 6. the block
# ---------------------------------------------------------------------------

BLOCK_CASES = [dict(top_k=2, scoring="softmax", renormalize=False, scale=1.0),
               dict(top_k=2, scoring="sigmoid", renormalize=True, scale=2.5, n_group=2, topk_group=1, bias=True)]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=["softmax_top2", "limited_sigmoid"])
def test_sparse_moe_block_aux_loss(env, experts_case, case, monkeypatch):
    """FluteSparseMoeBlock with aux_loss on (E = 4, K = 256, F = 512, 37 tokens, top-2): the output bits are the default block's,
    `block.aux` is the op called by hand, the default block has no `aux`, and (out.float().sum() + 0.01 balance + 0.001 z)
    .backward() reaches router_weight: the aux share of router_weight.grad - the difference to the backward of out.float().sum()
    alone, which runs the same launches bit for bit - is within the backward bound propagated through F.linear
    (moe_aux_cases.propagated_bound) of the fp64 chain: d_logits by the header's formula at the block's logits, times hidden."""
    with fp32_blas_reduction():                                    # the router GEMM and its backward: fp32 partial sums
        c = experts_case
        d, E, K, T = env.dev, c["E"], c["K"], c["T"]
        case = dict(case)
        k, scoring = case["top_k"], case["scoring"]
        gen = torch.Generator().manual_seed(91)
        bias = (torch.rand(E, generator=gen) * 0.2).to(d) if case.pop("bias", False) else None
        router = (torch.randn(E, K, generator=gen) * 0.08).to(c["dtype"]).to(d)
        layers = (c["gates"], c["ups"], c["downs"])
        experts = env.moe.FluteExperts.from_linears(*layers, fused=True, native_routing=True)
        plain_block = env.moe.FluteSparseMoeBlock(router.clone(), experts, bias=bias, **case)
        block = env.moe.FluteSparseMoeBlock(router.clone(), experts, bias=bias, **case)
        block.aux_loss = True
        with torch.no_grad():
            plain = plain_block(c["hidden"])
            out = block(c["hidden"])
            logits = torch.nn.functional.linear(c["hidden"], router)
            if case.get("n_group", 1) > 1:
                ids, _ = env.fa.moe_gate_limited(logits, k, case["n_group"], case["topk_group"], scoring, case["renormalize"], bias,
                                                 case["scale"])
            else:
                ids, _ = env.fa.moe_gate(logits, k, scoring, case["renormalize"], bias, case["scale"])
            by_hand = env.fa.moe_aux_loss(logits, ids, scoring)
        assert torch.equal(bits16(out), bits16(plain)) and not hasattr(plain_block, "aux")
        assert type(block.aux) is env.moe.MoeAuxLosses and all(same_bits(a, b) for a, b in zip(block.aux, by_hand))
        assert torch.equal(block.aux.load.cpu().long(), AC.load_of(ids.cpu(), E))

        seen = {}
        real_linear = torch.nn.functional.linear

        def linear(x, w, *rest):                                       # the block's router GEMM: its logits and the gradient they get
            y = real_linear(x, w, *rest)
            if w is block.router_weight and y.requires_grad:
                seen["logits"] = y.detach()
                y.register_hook(lambda g: seen.__setitem__("d_logits", g.detach().clone()))
            return y

        monkeypatch.setattr(torch.nn.functional, "linear", linear)
        block.router_weight.requires_grad_()

        def backward(with_aux):
            block.router_weight.grad = None
            h = c["hidden"].clone().requires_grad_()
            o = block(h)
            assert torch.equal(bits16(o), bits16(plain)) and block.aux.balance.requires_grad and block.aux.z.requires_grad
            loss = o.float().sum()
            if with_aux:
                loss = loss + 0.01 * block.aux.balance + 0.001 * block.aux.z
            loss.backward()
            return block.router_weight.grad.clone(), seen["d_logits"], h.grad

        rg_out, dl_out, _ = backward(False)
        rg_out2, dl_out2, _ = backward(False)
        rg_full, dl_full, h_grad = backward(True)
        assert torch.equal(bits16(dl_out), bits16(dl_out2)) and torch.equal(bits16(rg_out), bits16(rg_out2))
        assert torch.isfinite(rg_full).all() and torch.isfinite(h_grad).all() and not torch.equal(bits16(dl_full), bits16(dl_out))

        logits16, hidden = seen["logits"].cpu(), c["hidden"].cpu()
        assert torch.equal(bits16(logits16), bits16(logits.cpu()))
        ref_dl, dl_bound = AC.backward_bound(logits16, AC.load_of(ids.cpu(), E), 0.01, 0.001, scoring)
        ut, floor = AC.UNIT[logits16.dtype], AC.FLOOR[logits16.dtype]
        share = dl_full.cpu().double() - dl_out.cpu().double()
        ratio_dl = AC.worst_ratio(share, ref_dl, dl_bound + ut * dl_full.cpu().double().abs() + floor)
        ref_rg = ref_dl.T @ hidden.double()
        rg_bound = AC.propagated_bound(dl_bound, dl_full.cpu(), dl_out.cpu(), hidden)
        ratio_rg = AC.worst_ratio(rg_full.cpu().double() - rg_out.cpu().double(), ref_rg, rg_bound)
        print("FluteSparseMoeBlock aux_loss %s: error / bound d_logits share %.3f router_weight.grad share %.3f (max |ref| %.3e)"
              % (scoring, ratio_dl, ratio_rg, float(ref_rg.abs().max())))
        assert ratio_dl <= 1.0 and ratio_rg <= 1.0 and float(ref_rg.abs().max()) > 0
