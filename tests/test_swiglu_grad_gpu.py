"""flute_amd.swiglu_grad and flute_amd.moe_gather (swiglu_grad.hip) on the GPU, and the backward they serve behind
`native_glu_grad=True`: exact regimes bit for bit, random data inside the header's error account (its constant read from the
header), the `offsets` contract with hostile values in the rows no expert serves, non-finite operands, the gather, equal bits
over two calls and in a replayed graph, the wiring of `_grouped_glu_backward(native=True)` and the module.

The launch takes one lane per 8 columns and a workgroup of 128 lanes per 1024 columns of one row, and does not stride: F = 8 is one
lane, F = 264 is 33 vectors (neither a multiple of the wave nor of the workgroup), F = 1024 fills a workgroup exactly, F = 2056 is
three column chunks with a ragged last one; R = 1, 37, 300 rows."""
import pytest
import torch

from tests import swiglu_grad_cases as SC
from tests.glu_block_cases import BLOCK_K_CASES
from tests.grouped_cases import dense_project, restated_experts, scale_leaves
from tests.support import bits16, env, first_template, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu
F16, BF16 = SC.F16, SC.BF16
DTYPES = [F16, BF16]
SHAPES = [(1, 8), (37, 264), (300, 1024), (37, 2056), (300, 8), (1, 1024)]
INT_MIN = -2 ** 31


def on(env, *ts):
    return tuple(t.to(env.dev) for t in ts)


# ---------------------------------------------------------------------------
# 1. exact regimes
# ---------------------------------------------------------------------------

def exact_operands(R, F, dtype, seed):
    """dh a power of two with sign, u a small integer: dh u, dh u / 2 and dh g (g an integer up to 64) are exact in either type."""
    gen = torch.Generator().manual_seed(seed)
    dh = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0, -4.0])[torch.randint(0, 8, (R, F), generator=gen)].to(dtype)
    u = torch.randint(-3, 4, (R, F), generator=gen).to(dtype)
    return dh, u, gen


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,F", SHAPES)
def test_exact_regimes(env, dtype, R, F):
    dh, u, gen = exact_operands(R, F, dtype, 100 + R + F)
    prod = dh.double() * u.double()
    # g = 0: d = 2, sig = 1 / 2, ds = 1 / 2, sl = 0
    g = torch.zeros(R, F, dtype=dtype)
    dg, du = env.fa.swiglu_grad(*on(env, g, u, dh))
    assert torch.equal(dg.cpu().double(), prod / 2) and torch.all(du == 0)
    # 18 <= g <= 64: 1 + expf(-g) == 1, so sig = 1, ds = 1, sl = g
    g = torch.randint(18, 65, (R, F), generator=gen).to(dtype)
    dg, du = env.fa.swiglu_grad(*on(env, g, u, dh))
    assert torch.equal(dg.cpu().double(), prod) and torch.equal(du.cpu().double(), dh.double() * g.double())
    assert (dg.cpu().double() == prod).all() and dg.dtype == dtype and dg.shape == (R, F)
    # g <= -104: expf(-g) is infinite, sig = 0, sl = -0, ds = -0: zeros of either sign
    low = [-104.0, -128.0, -1000.0] + ([-65504.0] if dtype == F16 else [-3.0e38])
    g = torch.tensor(low)[torch.randint(0, len(low), (R, F), generator=gen)].to(dtype)
    dg, du = env.fa.swiglu_grad(*on(env, g, u, dh))
    assert torch.all(dg == 0) and torch.all(du == 0)


# ---------------------------------------------------------------------------
# 2. random data against fp64
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,F", SHAPES)
def test_random_within_the_headers_account(env, dtype, R, F):
    c = SC.header_c()
    g, u, dh = SC.draw(R, F, dtype, 7 * R + F)
    rdg, rdu, bdg, bdu, vdg, vdu = SC.bounds(g, u, dh, dtype, c)
    if R * F >= 1000:                                              # (a handful of elements proves no share)
        assert float(vdg.double().mean()) < 0.01 and float(vdu.double().mean()) < 0.01
    dg, du = env.fa.swiglu_grad(*on(env, g, u, dh))
    tdg, tdu = SC.torch_chain(*on(env, g, u, dh))
    worst = lambda x, r, b, v: float(torch.where(v, torch.zeros_like(b), (x.cpu().double() - r).abs() / b).max())
    print("swiglu_grad %s R=%d F=%d: worst error / bound dg %.3f du %.3f (torch chain: dg %.3f du %.3f), vacuous %.4f / %.4f"
          % (dtype, R, F, worst(dg, rdg, bdg, vdg), worst(du, rdu, bdu, vdu), worst(tdg, rdg, bdg, vdg),
             worst(tdu, rdu, bdu, vdu), float(vdg.double().mean()), float(vdu.double().mean())))
    assert torch.all(((dg.cpu().double() - rdg).abs() <= bdg) | vdg)
    assert torch.all(((du.cpu().double() - rdu).abs() <= bdu) | vdu)


# ---------------------------------------------------------------------------
# 3. offsets, through the C ABI into buffers with canaries
# ---------------------------------------------------------------------------

PAD = 64                                                           # elements: 128 bytes, which keeps the 16-byte alignment


def abi_swiglu(env, g, u, dh, off, canary):
    """flute_swiglu_grad into the middle of two canary-filled buffers; returns (dg, du, the four canary regions)."""
    R, F = g.shape
    bufs = [torch.full((PAD + R * F + PAD,), canary, dtype=g.dtype, device=env.dev) for _ in range(2)]
    outs = [b[PAD:PAD + R * F].view(R, F) for b in bufs]
    dtype_id = {F16: 0, BF16: 1}[g.dtype]
    env.check(env.lib.flute_swiglu_grad(dtype_id, R, F, 0 if off is None else off.shape[0] - 1, g.data_ptr(), u.data_ptr(),
                                        dh.data_ptr(), None if off is None else off.data_ptr(), outs[0].data_ptr(),
                                        outs[1].data_ptr(), env.stream_ptr(env.dev)))
    torch.cuda.synchronize()
    return outs[0], outs[1], [b[:PAD] for b in bufs] + [b[PAD + R * F:] for b in bufs]


@pytest.mark.parametrize("dtype", DTYPES)
def test_offsets(env, dtype):
    R, F, E = 37, 264, 3
    g, u, dh = on(env, *SC.draw(R, F, dtype, 31))
    canary = 123.0
    full_dg, full_du, guards = abi_swiglu(env, g, u, dh, None, canary)
    assert all(torch.all(x == canary) for x in guards)
    by_op = env.fa.swiglu_grad(g, u, dh)
    assert torch.equal(bits16(full_dg), bits16(by_op[0])) and torch.equal(bits16(full_du), bits16(by_op[1]))
    # (offsets[E], the rows it serves): in range, past R, negative
    for last, served in ((0, 0), (1, 1), (R - 1, R - 1), (R, R), (R + 5, R), (2 ** 31 - 1, R), (-3, 0), (INT_MIN, 0)):
        off = torch.tensor([0, min(max(last, 0), R) // 2, -7, last], dtype=torch.int32, device=env.dev)   # (only offsets[E] is read)
        hg, hu, hdh = g.clone(), u.clone(), dh.clone()
        for t, v in ((hg, float("nan")), (hu, float("inf")), (hdh, float("-inf"))):
            t[served:] = v                                         # what the rows no expert serves hold reaches nothing
        dg, du, guards = abi_swiglu(env, hg, hu, hdh, off, canary)
        assert all(torch.all(x == canary) for x in guards), last
        assert torch.equal(bits16(dg[:served]), bits16(full_dg[:served])), last
        assert torch.equal(bits16(du[:served]), bits16(full_du[:served])), last
        assert not bits16(dg[served:]).any() and not bits16(du[served:]).any(), last      # +0, bit for bit
        by_op = env.fa.swiglu_grad(hg, hu, hdh, off)
        assert torch.equal(bits16(by_op[0]), bits16(dg)) and torch.equal(bits16(by_op[1]), bits16(du))


# ---------------------------------------------------------------------------
# 4. hostile values
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_range_edges_and_non_finite_operands(env, dtype):
    R, F = 37, 264
    big = 65504.0 if dtype == F16 else 3.39e38
    big = float(torch.tensor(big).to(dtype))
    dh, u, _ = exact_operands(R, F, dtype, 41)
    dh = dh.abs().clamp(max=0.5) * torch.sign(dh)                  # |dh| = 1 / 2: dh g stays finite at the edge
    for sign in (1.0, -1.0):
        g = torch.full((R, F), sign * big).to(dtype)
        dg, du = env.fa.swiglu_grad(*on(env, g, u, dh))
        assert torch.isfinite(dg).all() and torch.isfinite(du).all()
        if sign > 0:                                               # ds = 1, sl = g
            assert torch.equal(dg.cpu().double(), dh.double() * u.double())
            assert torch.equal(du.cpu().double(), dh.double() * g.double())
        else:                                                      # ds = -0, sl = -0
            assert torch.all(dg == 0) and torch.all(du == 0)
    # one non-finite element in one operand changes that element's outputs and no other
    g, u, dh = on(env, *SC.draw(R, F, dtype, 43))
    base = env.fa.swiglu_grad(g, u, dh)
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()
    for which, value, at in ((0, float("nan"), (0, 0)), (0, float("inf"), (5, 8)), (0, float("-inf"), (36, 263)),
                             (1, float("inf"), (36, 256)), (1, float("nan"), (17, 7)), (2, float("-inf"), (3, 131)),
                             (2, float("nan"), (20, 64))):
        ops_ = [g.clone(), u.clone(), dh.clone()]
        ops_[which][at] = value
        dg, du = env.fa.swiglu_grad(*ops_)
        mask = torch.ones(R, F, dtype=torch.bool, device=env.dev)
        mask[at] = False
        for got, ref in ((dg, base[0]), (du, base[1])):
            assert torch.equal(bits16(got)[mask], bits16(ref)[mask]), (which, value)
        if which == 1:                                             # du does not read u
            assert not torch.isfinite(dg[at]) and torch.equal(bits16(du), bits16(base[1]))
        elif value != value or which == 2:
            assert not torch.isfinite(dg[at]) and not torch.isfinite(du[at]), (which, value)
        elif value > 0:                                            # g = +inf: d = 1, sig = 1, sl = inf, ds = 1 * (1 + inf * 0) = NaN
            assert torch.isnan(dg[at]) and torch.isinf(du[at])
        else:                                                      # g = -inf: d = inf, sig = 0, sl = -inf / inf = NaN, ds = 0 * (1 - inf) = NaN
            assert torch.isnan(dg[at]) and torch.isnan(du[at])


# ---------------------------------------------------------------------------
# 5. moe_gather
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 264, 2056])
def test_moe_gather(env, dtype, K):
    Tsrc, R, E = 20, 37, 3
    gen = torch.Generator().manual_seed(50 + K)
    X = torch.randint(-2 ** 15, 2 ** 15, (Tsrc, K), generator=gen).to(torch.int16).view(dtype).to(env.dev)   # every pattern, NaNs included
    rows_buf = torch.full((R + PAD,), 2 ** 31 - 1, dtype=torch.int32)
    rows_buf[:R] = torch.randint(0, Tsrc, (R,), generator=gen).int()
    rows_buf[2], rows_buf[3] = -5, Tsrc + 3                        # clamped to the first and the last source row
    rows_buf = rows_buf.to(env.dev)
    rows = rows_buf[:R]
    want = X.index_select(0, rows.clamp(0, Tsrc - 1).long())
    out = env.fa.moe_gather(X, rows)
    assert out.shape == (R, K) and out.dtype == dtype
    assert torch.equal(bits16(out), bits16(want))
    assert torch.equal(bits16(out[2]), bits16(X[0])) and torch.equal(bits16(out[3]), bits16(X[Tsrc - 1]))
    for last, served in ((R - 4, R - 4), (0, 0), (1, 1), (R + 9, R), (-1, 0)):
        off = torch.tensor([0, 0, 0, last], dtype=torch.int32, device=env.dev)
        hostile = rows.clone()
        hostile[served:] = INT_MIN                                 # never read
        out = env.fa.moe_gather(X, hostile, off)
        assert torch.equal(bits16(out[:served]), bits16(want[:served])), last
        assert not bits16(out[served:]).any(), last
    assert torch.all(rows_buf[R:] == 2 ** 31 - 1)                  # (the op writes nothing there; what follows `rows` stays)


# ---------------------------------------------------------------------------
# 6. equal bits over two calls and in a replayed graph
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_bits_over_two_calls_and_in_a_graph(env, dtype):
    R, F, Tsrc = 37, 264, 20
    g, u, dh = on(env, *SC.draw(R, F, dtype, 61))
    X = torch.randn(Tsrc, F, generator=torch.Generator().manual_seed(62)).to(dtype).to(env.dev)
    rows = torch.randint(0, Tsrc, (R,), generator=torch.Generator().manual_seed(63)).int().to(env.dev)
    off = torch.tensor([0, 9, 9, R - 5], dtype=torch.int32, device=env.dev)
    off2 = torch.tensor([0, 3, 20, 11], dtype=torch.int32, device=env.dev)

    def run(o):
        return env.fa.swiglu_grad(g, u, dh, o) + (env.fa.moe_gather(X, rows, o),)

    first = [t.clone() for t in run(off)]
    assert all(torch.equal(bits16(a), bits16(b)) for a, b in zip(run(off), first))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(off)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits16(a), bits16(b)) for a, b in zip(outs, first))
    eager = [t.clone() for t in run(off2)]
    off.copy_(off2)
    for t in outs:
        t.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits16(a), bits16(b)) for a, b in zip(outs, eager))
    assert not bits16(outs[0][11:]).any() and bits16(outs[0][:11]).any()


# ---------------------------------------------------------------------------
# 7. and 8.: the backward behind native_glu_grad
# ---------------------------------------------------------------------------

def make_experts_case(env, dtype, g):
    """E = 4 experts from FluteLinear.from_codes (4-bit, K = 256, F = 512), 37 tokens at top-2 among experts 0, 1, 3 - expert 2 is
    never chosen - token 0 routed only to ids outside [0, E), token 5 with one such slot; `lut`: every layer's lookups [N, K] in
    fp64.  (The shape and the draw of tests/test_grouped_scale_grad_gpu.py's module case, restated: test modules are not imported
    from.)"""
    d = env.dev
    E, K, F, T, bits, k = 4, 256, 512, 37, 4, 2
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(41)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, k=k, bits=bits, g=g, tid=tid, dtype=dtype)
    c["layers"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)], [linear(F, K) for _ in range(E)])
    lut = lambda m: env.fa.dequantize(m.weight, torch.ones_like(m.scales), m.tables2, bits, g, tid).double()
    c["lut"] = [[lut(m) for m in ms] for ms in c["layers"]]
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["dOut"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    chosen = torch.tensor([0, 1, 3])
    ids = torch.stack([chosen[torch.randperm(3, generator=gen)[:k]] for _ in range(T)])
    ids[0] = torch.tensor([E, -1])
    ids[5, 1] = E
    weights = torch.rand(T, k, generator=gen)
    c["ids"], c["weights"] = ids.to(d), (weights / weights.sum(1, keepdim=True)).to(dtype).to(d)
    return c


@pytest.fixture(scope="module")
def experts_cases(env):
    """g = 64: the module case of the existing backward tests; g = 32: the first of tests/glu_block_cases.py's (K, g) pairs, which
    the block form of the GLU launch serves ((K / g) % 8 == 0)."""
    assert BLOCK_K_CASES[0] == (256, 32)
    return {False: make_experts_case(env, F16, 64), True: make_experts_case(env, F16, BLOCK_K_CASES[0][1])}


def test_grouped_glu_backward_wiring(env, experts_cases):
    c = experts_cases[False]
    fa, ops = env.fa, env.fa.ops
    E, T, k, F, dtype = c["E"], c["T"], c["k"], c["F"], c["dtype"]
    gate, up = (env.moe.GroupedFluteLinear.from_linears(ms) for ms in c["layers"][:2])
    layer = (c["bits"], c["g"], c["tid"], env.num_sms)
    stacks = (gate.weight, gate.scales, gate.tables2, up.weight, up.scales, up.tables2)
    offsets, rows, _, pos, _ = fa.moe_route(c["ids"], None, E)
    R = T * k
    served = int(offsets[-1])
    assert served == R - 3 and int(offsets[3]) == int(offsets[2])  # three slots no expert serves, an expert without rows
    dh = (torch.randn(R, F, generator=torch.Generator().manual_seed(71)) / 4).to(dtype).to(env.dev)
    dh[served:] = float("nan")
    plain = lambda x, w, s, t: fa.qgemm_grouped(x, offsets, w, s, t, *layer)
    pair = lambda dg, du: fa.qgemm_grouped_input_grad(dg, offsets, *stacks[:3], *layer, grad_output2=du, weight2=stacks[3],
                                                      scales2=stacks[4], table22=stacks[5])
    with torch.no_grad():
        dx, x, dg, du = ops._grouped_glu_backward(dh, c["hidden"], rows, pos, offsets, *stacks, layer, True, native=True)
        want_x = fa.moe_gather(c["hidden"], rows, offsets)
        assert torch.equal(bits16(x), bits16(want_x)) and not bits16(x[served:]).any()
        want_dg, want_du = fa.swiglu_grad(plain(want_x, *stacks[:3]), plain(want_x, *stacks[3:]), dh, offsets)
        assert torch.equal(bits16(dg), bits16(want_dg)) and torch.equal(bits16(du), bits16(want_du))
        assert not bits16(dg[served:]).any() and not bits16(du[served:]).any() and bits16(dg[:served]).any()
        assert torch.equal(bits16(dx), bits16(fa.moe_combine(pair(want_dg, want_du), pos, offsets)))
        assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0 and torch.all(dx[0] == 0)
        none, _, dg2, _ = ops._grouped_glu_backward(dh, c["hidden"], rows, pos, offsets, *stacks, layer, False, native=True)
        assert none is None and torch.equal(bits16(dg2), bits16(dg))
        # native=False (the default, and what the keyword's absence means): the torch lines, restated; the rows no expert
        # serves hold what the plain launches left unwritten, so only the served rows of dg and du are defined
        for kw in (dict(native=False), {}):
            dx0, x0, dg0, du0 = ops._grouped_glu_backward(dh, c["hidden"], rows, pos, offsets, *stacks, layer, True, **kw)
            xr = c["hidden"].index_select(0, rows.clamp(0, T - 1).long())
            gr, ur, dhr = plain(xr, *stacks[:3]).float(), plain(xr, *stacks[3:]).float(), dh.float()
            sig = torch.sigmoid(gr)
            dgr = (dhr * ur * sig * (1 + gr * (1 - sig))).to(dtype)
            dur = (dhr * (gr * sig)).to(dtype)
            assert torch.equal(bits16(x0), bits16(xr))
            assert torch.equal(bits16(dg0[:served]), bits16(dgr[:served])) and torch.equal(bits16(du0[:served]), bits16(dur[:served]))
            assert torch.equal(bits16(dx0), bits16(fa.moe_combine(pair(dgr, dur), pos, offsets)))


def reference_and_yardstick(env, c):
    """fp64 autograd of the restated block on dense weights L * S (S an fp64 leaf), and the same loop in T over
    LearnableScalesFluteLinear - the reference and the yardstick of the existing module-level backward tests."""
    if "ref" not in c:
        h64, S64 = c["hidden"].double().requires_grad_(), scale_leaves(c)
        restated_experts(c, h64, c["ids"], c["weights"].double(), dense_project(c, S64)).backward(c["dOut"].double())
        loop = [[env.ln.LearnableScalesFluteLinear(m) for m in ms] for ms in c["layers"]]
        hT = c["hidden"].clone().requires_grad_()
        restated_experts(c, hT, c["ids"], c["weights"], lambda e, which, x: loop[which][e](x)).backward(c["dOut"])
        grads = [torch.stack([m.scales.grad if m.scales.grad is not None else torch.zeros_like(m.scales) for m in ms])
                 for ms in loop]
        c["ref"] = (h64.grad, [s.grad for s in S64], hT.grad, grads)
    return c["ref"]


@pytest.mark.parametrize("glu_blocks", [False, True])
def test_flute_experts_native_glu_grad(env, experts_cases, glu_blocks, monkeypatch):
    """FluteExperts(fused=True, native_routing=True, native_glu_grad=True) with learnable scales: hidden.grad and the scale
    gradients of gate and up against fp64, max-abs error relative to max|ref|, within twice the yardstick's error - the measure and
    the bound of test_flute_experts_backward and test_flute_experts_scale_grads - and a forward whose bits do not know the keyword."""
    c = experts_cases[glu_blocks]
    gh64, gs64, ghT, gsT = reference_and_yardstick(env, c)
    make = lambda v: env.moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True, glu_blocks=glu_blocks,
                                                       native_glu_grad=v)
    off_, on_ = make(False), make(True)
    assert on_.native_glu_grad is True and off_.native_glu_grad is False
    with torch.no_grad():
        frozen = off_(c["hidden"], c["ids"], c["weights"])
        assert torch.equal(bits16(on_(c["hidden"], c["ids"], c["weights"])), bits16(frozen))
    got, calls = {}, []
    ops = env.fa.ops
    for real in (ops.swiglu_grad, ops.moe_gather):                 # the backward looks both up in flute_amd.ops when it runs
        monkeypatch.setattr(ops, real.__name__, lambda *a, _real=real: calls.append(_real.__name__) or _real(*a))
    for name, experts in (("off", off_), ("on", on_)):
        params = env.moe.make_experts_learnable(experts)
        h = c["hidden"].clone().requires_grad_()
        out = experts(h, c["ids"], c["weights"])
        assert torch.equal(bits16(out), bits16(frozen))            # the forward's bits: the same with the keyword on and off
        del calls[:]
        out.backward(c["dOut"])
        assert calls == (["moe_gather", "swiglu_grad"] if name == "on" else []), (name, calls)
        got[name] = (h.grad, [p.grad for p in params])
    gh, gs = got["on"]
    assert torch.isfinite(gh).all() and torch.all(gh[0] == 0)
    err, yard = max_rel_err(gh, gh64), max_rel_err(ghT, gh64)
    print("FluteExperts native_glu_grad glu_blocks=%d: hidden.grad %.3e (keyword off %.3e, yardstick %.3e)"
          % (glu_blocks, err, max_rel_err(got["off"][0], gh64), yard))
    assert yard > 0 and err <= 2 * yard, (err, yard)
    for i, name in enumerate(("gate", "up")):
        assert gs[i] is not None and torch.isfinite(gs[i]).all() and torch.all(gs[i][2] == 0)
        err, yard = max_rel_err(gs[i], gs64[i]), max_rel_err(gsT[i], gs64[i])
        print("FluteExperts native_glu_grad glu_blocks=%d %s scales.grad: %.3e (keyword off %.3e, yardstick %.3e)"
              % (glu_blocks, name, err, max_rel_err(got["off"][1][i], gs64[i]), yard))
        assert yard > 0 and err <= 2 * yard, (name, err, yard)
    # the keyword without the fused launch has nothing to select
    with pytest.raises(ValueError, match="native_glu_grad"):
        env.moe.FluteExperts.from_linears(*c["layers"], fused=False, native_glu_grad=True)
