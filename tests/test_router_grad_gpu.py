"""flute_amd.moe_weight_grad and flute_amd.moe_gate_grad (router_grad.hip) on the GPU, and the backward they serve behind
`native_router_grad=True` and `moe_combine(rows=...)`: exact regimes bit for bit, random data inside the derived bound (weight
gradient) or against the default torch backward's own error (gate gradient), the `offsets` contract with hostile values in the rows
no expert serves, non-finite operands, canaries, equal bits over two calls and in a replayed graph, and the wiring up to the block.

The weight gradient takes one workgroup of 256 lanes per row, a lane 8 columns per step of 2048: K = 8 is one lane, 264 is 33
vectors, 2048 exactly one step, 2056 a step and one lane, 4104 two steps and a ragged third; R = 1, 37, 300 rows.  The gate
gradient takes one wave per token and experts l, l + 64, ... per lane: E = 8, 64, 72 (not a multiple of the wave), 256."""
import itertools

import pytest
import torch

from tests import exact_cases as XC
from tests import router_grad_cases as RC
from tests.grouped_cases import (counts_of, exact_layers, experts_case, gate_formula, restated_experts,  # noqa: F401
                                 stack_exact)
from tests.support import bits16, bits32, bits_by_size, env, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu
F16, BF16, F32 = RC.F16, RC.BF16, RC.F32
DTYPES = [F16, BF16]
DTYPE_ID = {F16: 0, BF16: 1, F32: 2}
ROWS, WIDTHS = [1, 37, 300], [8, 264, 2048, 2056, 4104]
INT_MIN = -2 ** 31
PAD = 64                                                           # elements: keeps the 16-byte alignment of either width


def on(env, *ts):
    return tuple(None if t is None else t.to(env.dev) for t in ts)


# ---------------------------------------------------------------------------
# 1. the weight gradient: exact regime and random data
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,K", list(itertools.product(ROWS, WIDTHS)))
def test_weight_grad_exact(env, dtype, R, K):
    """Operands multiples of 1/8: every product is a multiple of 1/64 and sum |products| < 2^18, so every partial sum in any
    order has at most 24 significant bits and the fp64 sum is the only allowed answer."""
    dhp, h = RC.exact_weight_operands(R, K, dtype, 1000 + R + K)
    prod = dhp.double() * h.double()
    total = float(prod.abs().sum(dim=1).max())
    assert total < XC.EXACT_SUM_LIMIT and total < 2.0 ** 18 and torch.equal(prod * 64, (prod * 64).round())
    rw = torch.tensor([0.25, -0.5, 1.0, 2.0])[torch.randint(0, 4, (R,), generator=torch.Generator().manual_seed(R + K))]
    d_rw, dH = env.fa.moe_weight_grad(*on(env, dhp, h, rw))
    assert d_rw.shape == (R,) and d_rw.dtype == torch.float32 and dH.shape == (R, K) and dH.dtype == dtype
    assert torch.equal(d_rw.cpu().double(), prod.sum(dim=1))
    assert torch.equal(dH.cpu().double(), rw.double()[:, None] * dhp.double())        # a power of two times |x| <= 4: exact in T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,K", list(itertools.product(ROWS, WIDTHS)))
def test_weight_grad_random(env, dtype, R, K):
    """dH bit for bit (row_weight[:, None] * dHp.float()).to(T) - +-0, a subnormal and the overflow to +-inf included - and
    d_row_weight inside gamma_(K-1) sum |dHp H| in every row: the products are exact, so the bound holds for any order."""
    dhp, h, rw = RC.draw_weight_operands(R, K, dtype, 7 * R + K)
    big, sub = (65504.0, 2.0 ** -24) if dtype == F16 else (3.3e38, 2.0 ** -133)
    dhp[0, :5] = torch.tensor([0.0, -0.0, sub, big, -big]).to(dtype)
    h[0, :5] = 0.5                                                 # (the products stay finite in fp32; dH = 1.5 * big does not fit T)
    rw[0] = 1.5
    if R > 1:
        rw[1] = -rw[1]                                             # -0 from +0
        dhp[1, 0] = 0.0
    ref, bound = RC.weight_grad_bound(dhp, h)
    d_rw, dH = env.fa.moe_weight_grad(*on(env, dhp, h, rw))
    want = (rw[:, None] * dhp.float()).to(dtype)
    assert torch.isinf(want[0, 3]) and torch.isinf(want[0, 4]) and float(want[0, 2]) != 0 and bits16(want[0, 1:2]).item() != 0
    assert torch.equal(bits16(dH.cpu()), bits16(want))
    err = (d_rw.cpu().double() - ref).abs()
    torch_err = ((dhp.float() * h.float()).sum(dim=1).double() - ref).abs()
    print("moe_weight_grad %s R=%d K=%d: worst error / bound %.2e (torch's fp32 sum on the CPU: %.2e)"
          % (dtype, R, K, float((err / bound).max()), float((torch_err / bound).max())))
    assert float(bound.min()) > 0 and torch.all(err <= bound)


# ---------------------------------------------------------------------------
# 2. offsets, through the C ABI into buffers with canaries; dH = NULL
# ---------------------------------------------------------------------------

def abi_weight_grad(env, dhp, h, rw, off, canary, with_dh=True):
    """flute_moe_weight_grad into the middle of canary-filled buffers; returns (d_row_weight, dH or None, the canary regions)."""
    R, K = dhp.shape
    wbuf = torch.full((PAD + R + PAD,), canary, dtype=torch.float32, device=env.dev)
    hbuf = torch.full((PAD + R * K + PAD,), canary, dtype=dhp.dtype, device=env.dev)
    d_rw, dH = wbuf[PAD:PAD + R], hbuf[PAD:PAD + R * K].view(R, K)
    env.check(env.lib.flute_moe_weight_grad(DTYPE_ID[dhp.dtype], R, K, 0 if off is None else off.shape[0] - 1, dhp.data_ptr(),
                                            h.data_ptr(), rw.data_ptr() if with_dh else None,
                                            None if off is None else off.data_ptr(), d_rw.data_ptr(),
                                            dH.data_ptr() if with_dh else None, env.stream_ptr(env.dev)))
    torch.cuda.synchronize()
    guards = [wbuf[:PAD], wbuf[PAD + R:], hbuf[:PAD], hbuf[PAD + R * K:]] + ([] if with_dh else [dH])
    return d_rw, (dH if with_dh else None), guards


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_grad_offsets(env, dtype):
    R, K = 37, 264
    dhp, h, rw = on(env, *RC.draw_weight_operands(R, K, dtype, 31))
    canary = 123.0
    full_w, full_h, guards = abi_weight_grad(env, dhp, h, rw, None, canary)
    assert all(torch.all(x == canary) for x in guards)
    by_op = env.fa.moe_weight_grad(dhp, h, rw)
    assert torch.equal(bits32(full_w), bits32(by_op[0])) and torch.equal(bits16(full_h), bits16(by_op[1]))
    only_w, none, guards = abi_weight_grad(env, dhp, h, rw, None, canary, with_dh=False)     # dH = NULL: the sums only
    assert none is None and all(torch.all(x == canary) for x in guards) and torch.equal(bits32(only_w), bits32(full_w))
    sums_only = env.fa.moe_weight_grad(dhp, h, None, want_input_grad=False)
    assert sums_only[1] is None and torch.equal(bits32(sums_only[0]), bits32(full_w))
    for last, served in ((0, 0), (1, 1), (R - 1, R - 1), (R, R), (R + 5, R), (2 ** 31 - 1, R), (-3, 0), (INT_MIN, 0)):
        off = torch.tensor([0, min(max(last, 0), R) // 2, -7, last], dtype=torch.int32, device=env.dev)   # (only offsets[E] is read)
        hd, hh, hw = dhp.clone(), h.clone(), rw.clone()
        for t, v in ((hd, float("inf")), (hh, float("nan")), (hw, float("-inf"))):
            t[served:] = v                                         # what the rows no expert serves hold reaches nothing
        d_rw, dH, guards = abi_weight_grad(env, hd, hh, hw, off, canary)
        assert all(torch.all(x == canary) for x in guards), last
        assert torch.equal(bits32(d_rw[:served]), bits32(full_w[:served])), last
        assert torch.equal(bits16(dH[:served]), bits16(full_h[:served])), last
        assert not bits32(d_rw[served:]).any() and not bits16(dH[served:]).any(), last         # +0, bit for bit
        by_op = env.fa.moe_weight_grad(hd, hh, hw, off)
        assert torch.equal(bits32(by_op[0]), bits32(d_rw)) and torch.equal(bits16(by_op[1]), bits16(dH))
        only_w, _, guards = abi_weight_grad(env, hd, hh, hw, off, canary, with_dh=False)
        assert all(torch.all(x == canary) for x in guards) and torch.equal(bits32(only_w), bits32(d_rw)), last


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_grad_nan_stays_in_its_row_and_rows_do_not_know_their_place(env, dtype):
    R, K = 37, 2056
    dhp, h, rw = on(env, *RC.draw_weight_operands(R, K, dtype, 43))
    base_w, base_h = env.fa.moe_weight_grad(dhp, h, rw)
    assert torch.isfinite(base_w).all() and torch.isfinite(base_h).all()
    for which, at in ((0, (5, 2050)), (1, (36, 0)), (2, 17)):
        ops_ = [dhp.clone(), h.clone(), rw.clone()]
        ops_[which][at] = float("nan")
        d_rw, dH = env.fa.moe_weight_grad(*ops_)
        row = at if which == 2 else at[0]
        keep = torch.ones(R, dtype=torch.bool, device=env.dev)
        keep[row] = False
        assert torch.equal(bits32(d_rw)[keep], bits32(base_w)[keep]) and torch.equal(bits16(dH)[keep], bits16(base_h)[keep])
        assert torch.isnan(d_rw[row]) == (which != 2)              # (row_weight does not enter the sum)
        assert torch.isnan(dH[row]).any() == (which != 1)          # (H does not enter dH)
    # a row's two results depend neither on R nor on the row it sits in
    order = torch.randperm(R, generator=torch.Generator().manual_seed(44)).to(env.dev)
    w2, h2 = env.fa.moe_weight_grad(dhp[order], h[order], rw[order])
    assert torch.equal(bits32(w2), bits32(base_w[order])) and torch.equal(bits16(h2), bits16(base_h[order]))
    w1, h1 = env.fa.moe_weight_grad(dhp[11:12], h[11:12], rw[11:12])
    assert torch.equal(bits32(w1), bits32(base_w[11:12])) and torch.equal(bits16(h1), bits16(base_h[11:12]))
    big = torch.cat([dhp] * 9), torch.cat([h] * 9), torch.cat([rw] * 9)
    w9, h9 = env.fa.moe_weight_grad(*big)
    assert torch.equal(bits32(w9[-R:]), bits32(base_w)) and torch.equal(bits16(h9[-R:]), bits16(base_h))


# ---------------------------------------------------------------------------
# 3. the gate gradient
# ---------------------------------------------------------------------------

EXPERTS, TOPK = [8, 64, 72, 256], [1, 2, 8]
FORMS = list(itertools.product(("softmax", "sigmoid"), (False, True), (1.0, 2.5)))


def draw_gate(env, T, E, k, dtype, seed, limited):
    """Random logits, the kernel's own ids for them (moe_gate or moe_gate_limited) and a random incoming gradient."""
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, E, generator=gen) * 2).to(dtype).to(env.dev)
    q = torch.randn(T, k, generator=gen).to(env.dev)
    if limited:
        ids, _ = env.fa.moe_gate_limited(logits, k, *RC.limited_groups(E, k))
    else:
        ids, _ = env.fa.moe_gate(logits, k)
    return logits, ids, q


@pytest.mark.parametrize("limited", [False, True], ids=["moe_gate", "moe_gate_limited"])
@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("E", EXPERTS)
def test_gate_grad_random(env, E, dtype, limited):
    """Against the fp64 restatement of the header's formula, max error relative to max |ref|; the yardstick is the default
    backward - torch's fp32 autograd of the gate formula, rounded to the logits' type - on the same inputs, and the allowance
    four times its error.

    The measure is taken per (k, scoring, renormalize, scale) over the tokens of the T = 1 and the T = 37 launch together, 38
    tokens.  A token's result does not depend on T (asserted bit for bit below), so this is the measure of one batch run as two
    launches; taken on the T = 1 launch alone it compares as few as ONE nonzero number (sigmoid, k = 1), where the yardstick's
    own error is anywhere between 0 and an ulp and four times it bounds nothing - measured on the MI355X: fp32, E = 8, T = 1,
    k = 1, sigmoid, scale 2.5: 7.3e-08 here (1.2 * 2^-24, three roundings) against a yardstick of 1.7e-09.  Every launch's own
    two figures are printed."""
    worst = (0.0, None)
    for k in TOPK:
        draws = [draw_gate(env, T, E, k, dtype, 100 * E + 10 * k + T, limited) for T in (1, 37)]
        for scoring, renorm, scale in FORMS:
            form = (scoring, renorm, scale)
            got = [env.fa.moe_gate_grad(*d, *form) for d in draws]
            assert all(g.shape == (d[0].shape[0], E) and g.dtype == dtype for g, d in zip(got, draws))
            ref = [RC.gate_grad_formula(*d, *form) for d in draws]
            if k == 1 and renorm:                                  # w = s / s = 1: the derivative is zero, and B = q 1 = q makes it so exactly
                assert not any(r.any() for r in ref) and not any((g != 0).any() for g in got), form
                continue
            chain = [RC.gate_torch_chain(*d, *form) for d in draws]
            for g, r, c, d in zip(got, ref, chain, draws):
                print("moe_gate_grad %s E=%d T=%d k=%d %s renormalize=%d scale=%.1f limited=%d: %.3e (torch fp32 backward %.3e)"
                      % (dtype, E, d[0].shape[0], k, *form, limited, max_rel_err(g, r), max_rel_err(c, r)))
            err, yard = max_rel_err(torch.cat(got), torch.cat(ref)), max_rel_err(torch.cat(chain), torch.cat(ref))
            assert yard > 0 and err <= 4 * yard, (k, form, err, yard)
            worst = max(worst, (err / yard, (k,) + form))
    print("moe_gate_grad %s E=%d limited=%d: worst error / yardstick %.2f at %s" % (dtype, E, limited, *worst))


@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("E", [8, 64, 256])
def test_gate_grad_exact_regimes(env, E, dtype):
    """Sigmoid at logits 0: s = 1 / 2 and s (1 - s) = 1 / 4.  Softmax at equal logits, E a power of two: s = 1 / E.  With q powers
    of two (and k a power of two under renormalize) every intermediate is a dyadic number of a few bits: the fp64 formula's value is
    the only allowed answer, bit for bit."""
    T = 37
    gen = torch.Generator().manual_seed(E)
    for k, renorm, scale, level in itertools.product((1, 2, 8), (False, True), (1.0, 2.5), (0.0, 3.0)):
        ids = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)]).int().to(env.dev)
        q = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0, 0.25])[torch.randint(0, 8, (T, k), generator=gen)].to(env.dev)
        zeros = torch.zeros(T, E, dtype=dtype, device=env.dev)
        got = env.fa.moe_gate_grad(zeros, ids, q, "sigmoid", renorm, scale)
        ref = RC.gate_grad_formula(zeros, ids, q, "sigmoid", renorm, scale)
        assert torch.equal(ref.float().double(), ref)              # a few bits, exact in fp32: the premise
        assert torch.equal(got.double(), ref.to(dtype).double()), ("sigmoid", k, renorm, scale)
        equal = torch.full((T, E), level, dtype=dtype, device=env.dev)
        got = env.fa.moe_gate_grad(equal, ids, q, "softmax", renorm, scale)
        ref = RC.gate_grad_formula(equal, ids, q, "softmax", renorm, scale)
        assert torch.equal(ref.float().double(), ref)              # a few bits: the premise
        assert torch.equal(got.double(), ref.to(dtype).double()), ("softmax", k, renorm, scale, level)
        assert float(ref.abs().max()) > 0 or (k == 1 and renorm)   # (one renormalised slot: w = 1, the derivative is zero)


def abi_gate_grad(env, logits, ids, q, drw, pos, scoring, renorm, scale, canary):
    T, E = logits.shape
    buf = torch.full((PAD + T * E + PAD,), canary, dtype=logits.dtype, device=env.dev)
    out = buf[PAD:PAD + T * E].view(T, E)
    ptr = lambda t: None if t is None else t.data_ptr()
    env.check(env.lib.flute_moe_gate_grad(DTYPE_ID[logits.dtype], T, E, ids.shape[1], {"softmax": 0, "sigmoid": 1}[scoring],
                                          int(renorm), float(scale), logits.data_ptr(), ids.data_ptr(), ptr(q), ptr(drw), ptr(pos),
                                          out.data_ptr(), env.stream_ptr(env.dev)))
    torch.cuda.synchronize()
    return out, [buf[:PAD], buf[PAD + T * E:]]


@pytest.mark.parametrize("dtype", [F16, F32])
@pytest.mark.parametrize("E,k", [(8, 2), (72, 8), (256, 8)])
def test_gate_grad_through_pos_and_hostile_slots(env, E, k, dtype):
    T = 37
    P = T * k
    logits, ids, q = draw_gate(env, T, E, k, dtype, 7 * E + k, False)
    gen = torch.Generator().manual_seed(E + k)
    drw = torch.randn(P, generator=gen).to(env.dev)
    pos = torch.randperm(P, generator=gen).int().view(T, k).to(env.dev)
    pos[0, 0], pos[3, k - 1], pos[5, 0], pos[6, 0] = -1, P, 2 ** 31 - 1, INT_MIN          # these add nothing
    canary = 77.0
    for scoring, renorm, scale in FORMS:
        form = (scoring, renorm, scale)
        # d_row_weight through pos equals the pre-folded sum handed as d_weights, bit for bit; alone, and on top of d_weights
        for dw in (None, q):
            folded = RC.fold_pos(dw, drw, pos)
            want = env.fa.moe_gate_grad(logits, ids, folded, *form)
            got = env.fa.moe_gate_grad(logits, ids, dw, *form, grad_row_weight=drw, pos=pos)
            assert torch.equal(bits_by_size(got), bits_by_size(want)), (form, dw is None)
        # every element is written, nothing around it: the C ABI into canaries
        out, guards = abi_gate_grad(env, logits, ids, q, drw, pos, *form, canary)
        assert all(torch.all(x == canary) for x in guards) and torch.equal(bits_by_size(out), bits_by_size(got))
        # an id outside [0, E) is skipped: the result is that of the row without the slot
        base = env.fa.moe_gate_grad(logits, ids, q, *form)
        assert torch.isfinite(base).all()
        if k > 1:
            hostile = ids.clone()
            hostile[2, 0], hostile[4, k - 1], hostile[9, 1] = E, -1, INT_MIN
            got = env.fa.moe_gate_grad(logits, hostile, q, *form)
            keep = torch.ones(T, dtype=torch.bool, device=env.dev)
            keep[[2, 4, 9]] = False
            assert torch.equal(bits_by_size(got)[keep], bits_by_size(base)[keep])
            ref = RC.gate_grad_formula(logits, hostile, q, *form)
            yard = max_rel_err(RC.gate_torch_chain(logits, ids, q, *form), RC.gate_grad_formula(logits, ids, q, *form))
            assert torch.isfinite(got).all() and max_rel_err(got, ref) <= 4 * yard, form
        # a NaN logit stays in its token
        bad = logits.clone()
        bad[7, E - 1] = float("nan")
        got = env.fa.moe_gate_grad(bad, ids, q, *form)
        keep = torch.ones(T, dtype=torch.bool, device=env.dev)
        keep[7] = False
        assert torch.equal(bits_by_size(got)[keep], bits_by_size(base)[keep])
        # a token's result depends neither on T nor on its row
        one = env.fa.moe_gate_grad(logits[11:12], ids[11:12], q[11:12], *form)
        assert torch.equal(bits_by_size(one), bits_by_size(base[11:12]))


# ---------------------------------------------------------------------------
# 4. equal bits over two calls and in a replayed graph
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_bits_over_two_calls_and_in_a_graph(env, dtype):
    R, K, T, E, k = 37, 2056, 37, 72, 8
    dhp, h, rw = on(env, *RC.draw_weight_operands(R, K, dtype, 61))
    dhp2, h2, rw2 = on(env, *RC.draw_weight_operands(R, K, dtype, 62))
    off = torch.tensor([0, 9, 9, R - 5], dtype=torch.int32, device=env.dev)
    off2 = torch.tensor([0, 3, 20, 11], dtype=torch.int32, device=env.dev)
    logits, ids, q = draw_gate(env, T, E, k, dtype, 63, False)
    logits2, ids2, q2 = draw_gate(env, T, E, k, dtype, 64, True)
    drw = torch.randn(T * k, generator=torch.Generator().manual_seed(65)).to(env.dev)
    pos = torch.randperm(T * k, generator=torch.Generator().manual_seed(66)).int().view(T, k).to(env.dev)

    def run():
        return env.fa.moe_weight_grad(dhp, h, rw, off) + (
            env.fa.moe_gate_grad(logits, ids, q, "softmax", True, 2.5, grad_row_weight=drw, pos=pos),
            env.fa.moe_gate_grad(logits, ids, q, "sigmoid", True, 1.0))

    same = lambda xs, ys: all(torch.equal(bits_by_size(a), bits_by_size(b)) for a, b in zip(xs, ys))
    first = [t.clone() for t in run()]
    assert same(run(), first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    graph.replay()
    torch.cuda.synchronize()
    assert same(outs, first)
    for dst, src in ((dhp, dhp2), (h, h2), (rw, rw2), (off, off2), (logits, logits2), (ids, ids2), (q, q2)):
        dst.copy_(src)                                             # other contents in the same buffers
    eager = [t.clone() for t in run()]
    assert not same(eager[:1], first[:1]) and not same(eager[2:3], first[2:3])
    for t in outs:
        t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert same(outs, eager)
    assert not bits32(outs[0][11:]).any() and bits32(outs[0][:11]).any()


# ---------------------------------------------------------------------------
# 5. the wiring: the weighted op, moe_combine, the block
# ---------------------------------------------------------------------------

def test_qgemm_grouped_weighted_native_router_grad(env):
    """Exact 4-bit stacks, integer dY and hidden states: input.grad is bit for bit the default's, row_weight.grad the exact sum,
    and the row no expert serves - whose h is NaN - gets 0 in both."""
    fa, d = env.fa, env.dev
    bits, tile_p, g, dtype, K, N = 4, 32, 64, F16, 320, 3 * 128
    counts = counts_of(fa.ops.GROUPED_INPUT_GRAD_ROW_BLOCK)
    E, T, k = len(counts), 50, 2
    Q, S, t2, tid = stack_exact(env, exact_layers(bits, tile_p, g, dtype, K, N, False, E, 9100))
    args = (bits, g, tid, env.num_sms)
    gen = torch.Generator().manual_seed(17)
    ids = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)]).to(torch.int32)
    ids[3, 1] = E                                                  # a slot no expert serves
    offsets, rows, _, _, _ = fa.moe_route(ids.to(d), None, E)
    R = T * k
    assert int(offsets[-1]) == R - 1
    h = XC.make_x(T, K, 18, dtype, witness=False).to(d).index_select(0, rows.long()).clone()
    h[-1] = float("nan")
    rw = torch.tensor([0.25, -0.5, 1.0, 2.0])[torch.randint(0, 4, (R,), generator=torch.Generator().manual_seed(23))].to(d)
    dY = XC.make_x(R, N, 24, dtype, witness=False).to(d)
    grads, outs = {}, {}
    for native in (False, True):
        hg, rwg = h.clone().requires_grad_(), rw.clone().requires_grad_()
        y = fa.qgemm_grouped_weighted(hg, offsets, Q, S, t2, rwg, *args, native_router_grad=native)
        y.backward(dY)
        grads[native], outs[native] = (hg.grad, rwg.grad), y.detach()
    assert torch.equal(bits16(outs[True]), bits16(outs[False]))
    assert torch.equal(bits16(grads[True][0]), bits16(grads[False][0]))
    dHp = fa.qgemm_grouped_input_grad(dY, offsets, Q, S, t2, *args)
    prod = dHp.double()[:-1] * h.double()[:-1]
    assert float(prod.abs().sum(dim=1).max()) < XC.EXACT_SUM_LIMIT and torch.equal(prod * 8, (prod * 8).round())
    got = grads[True][1]
    assert got.dtype == torch.float32 and torch.equal(got[:-1].double(), prod.sum(dim=1)) and bits32(got[-1:]).item() == 0
    assert torch.equal(bits32(got), bits32(grads[False][1]))       # (exact data: torch's order gives the same sum)
    assert not bits16(grads[True][0][-1]).any()
    # row_weight alone: the sums only, the same bits
    rwg = rw.clone().requires_grad_()
    fa.qgemm_grouped_weighted(h, offsets, Q, S, t2, rwg, *args, native_router_grad=True).backward(dY)
    assert torch.equal(bits32(rwg.grad), bits32(got))


def test_moe_combine_rows_backward(env):
    fa, d = env.fa, env.dev
    T, k, E, N = 37, 3, 5, 264
    gen = torch.Generator().manual_seed(81)
    ids = torch.randint(0, E, (T, k), generator=gen).int()
    ids[0] = torch.tensor([E, -1, E + 5])                          # a token no expert serves
    ids[5, 1] = E
    offsets, rows, _, pos, _ = fa.moe_route(ids.to(d), None, E)
    assert int(offsets[-1]) == T * k - 4
    y = torch.randn(T * k, N, generator=gen).half().to(d)
    dOut = torch.randn(T, N, generator=gen).half().to(d)
    got = {}
    for with_rows in (False, True):
        yg = y.clone().requires_grad_()
        out = fa.moe_combine(yg, pos, offsets, rows if with_rows else None)
        out.backward(dOut)
        got[with_rows] = (out.detach(), yg.grad)
    assert torch.equal(bits16(got[True][0]), bits16(got[False][0]))
    assert torch.equal(bits16(got[True][1]), bits16(got[False][1]))
    assert not bits16(got[True][1][T * k - 4:]).any() and bits16(got[True][1][:T * k - 4]).any()


BLOCK_CASES = [dict(top_k=2, scoring="softmax", renormalize=False, scale=1.0),
               dict(top_k=2, scoring="sigmoid", renormalize=True, scale=2.5, n_group=2, topk_group=1, bias=True)]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=["softmax_top2", "limited_sigmoid"])
def test_sparse_moe_block_native_router_grad(env, experts_case, case, monkeypatch):
    """FluteSparseMoeBlock (E = 4, K = 256, F = 512, 37 tokens) with the router training: hidden.grad and router_weight.grad
    against fp64 autograd of the dense block, each within twice the error of the same module with the keyword off; the forward is
    bit-identical with the keyword on and off, and the backward runs the three launches."""
    c = experts_case
    d, dtype, E, K, T = env.dev, c["dtype"], c["E"], c["K"], c["T"]
    case = dict(case)
    k = case["top_k"]
    gen = torch.Generator().manual_seed(53)
    dOut = torch.randn(T, K, generator=gen).to(dtype).to(d)
    bias = (torch.rand(E, generator=gen) * 0.2).to(d) if case.pop("bias", False) else None
    limited = case.get("n_group", 1) > 1
    scoring, renorm, scale = case["scoring"], case["renormalize"], case["scale"]
    # a router whose keys are well separated: holding the ids fixed is then no assumption
    for attempt in range(20):
        router = (torch.randn(E, K, generator=gen) * 0.08).to(dtype).to(d)
        logits = torch.nn.functional.linear(c["hidden"], router)
        s = torch.softmax(logits.float(), 1) if scoring == "softmax" else torch.sigmoid(logits.float())
        keys = logits.float() if bias is None else s + bias
        if limited:
            gkeys = keys.view(T, case["n_group"], -1).max(dim=2).values.sort(dim=1, descending=True).values
            gap = gkeys[:, case["topk_group"] - 1] - gkeys[:, case["topk_group"]]
        else:
            top = keys.sort(dim=1, descending=True).values
            gap = top[:, k - 1] - top[:, k]
        if float(gap.min()) > 2.0 ** -8:
            break
    assert float(gap.min()) > 2.0 ** -8, float(gap.min())
    with torch.no_grad():
        if limited:
            ids, _ = env.fa.moe_gate_limited(logits, k, case["n_group"], case["topk_group"], scoring, renorm, bias, scale)
        else:
            ids, _ = env.fa.moe_gate(logits, k, scoring, renorm, bias, scale)
    layers = (c["gates"], c["ups"], c["downs"])
    deq = lambda m: env.fa.dequantize(m.weight, m.scales, m.tables2, c["bits"], c["g"], c["tid"]).double()
    dense = [[deq(m[e]) for m in layers] for e in range(E)]
    hd, rd = c["hidden"].double().requires_grad_(), router.double().requires_grad_()
    wd = gate_formula(hd @ rd.T, ids, scoring, renorm, scale)
    restated_experts(c, hd, ids, wd, lambda e, which, x: x @ dense[e][which].T).backward(dOut.double())

    calls = []
    ops = env.fa.ops
    for real in (ops.moe_weight_grad, ops.moe_gate_grad, ops.moe_gather):     # the backward looks them up in flute_amd.ops when it runs
        monkeypatch.setattr(ops, real.__name__, lambda *a, _real=real, **kw: calls.append(_real.__name__) or _real(*a, **kw))
    got = {}
    for native in (False, True):
        experts = env.moe.FluteExperts.from_linears(*layers, fused=True, native_routing=True, native_router_grad=native)
        block = env.moe.FluteSparseMoeBlock(router.clone(), experts, bias=bias, **case)
        with torch.no_grad():
            plain = block(c["hidden"])
        block.router_weight.requires_grad_()
        h = c["hidden"].clone().requires_grad_()
        out = block(h)
        assert torch.equal(bits16(out), bits16(plain))
        del calls[:]
        out.backward(dOut)
        assert calls == (["moe_gather", "moe_weight_grad", "moe_gate_grad"] if native else []), (native, calls)
        got[native] = (plain, h.grad, block.router_weight.grad)
    assert torch.equal(bits16(got[True][0]), bits16(got[False][0]))            # the forward does not know the keyword
    for i, (name, ref) in enumerate((("hidden.grad", hd.grad), ("router_weight.grad", rd.grad)), 1):
        err, yard = max_rel_err(got[True][i], ref), max_rel_err(got[False][i], ref)
        print("FluteSparseMoeBlock native_router_grad %s %s: %.3e (keyword off %.3e)" % (scoring, name, err, yard))
        assert torch.isfinite(got[True][i]).all() and float(got[True][i].abs().max()) > 0
        assert yard > 0 and err <= 2 * yard, (name, err, yard)
