"""The block form of the grouped input gradient (qgemm_grouped_input_grad_blocks.h: one workgroup per 128-row block of an
expert x 256 k) on the GPU, `form="blocks"` unless said otherwise, at the smallest shapes at which it can still go wrong:
empty experts, both sides of a 128-row block edge, ragged last blocks, one and two k blocks, one chunk pair and a chunk
sequence that wraps the double buffers, a block map that crosses a 64-expert round, malformed tables, graph replay on
another table.

Exact inputs (tests/exact_cases) must come back bit for bit per expert and equal to the slab form; the two forms sum over N
in the same order, so random data must give equal bits too, within the componentwise bound of the documented arithmetic."""
import os
import re

import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import counts_of, exact_layers, exact_matrix, exact_seed, random_stack, stack_exact
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
RB = 128                                         # rows per block
COUNTS = counts_of(RB)                           # 0, 1, 127, 128, 129, 0, 259, 5: three blocks with a ragged last among them


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")


def min_mean_rows(env, E, K):
    """The mean rows per expert from which the automatic rule takes blocks (include/flute_amd.h), restated: the first
    constant where E * (K / 256) workgroups fill the chip, the second where they do not."""
    with open(HEADER) as f:
        text = f.read()
    get = lambda name: int(re.search(r"#define %s (\d+)\b" % name, text).group(1))
    full, partial = (get("FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS"),
                     get("FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS_PARTIAL"))
    return full if E * (K // 256) >= env.num_sms else partial


# ---- the premise and comparison of test_grouped_input_grad_gpu.py's check_exact_grad, restated ----------------------------

def exact_grad(dY, layer):
    """(R, A) = (dY @ W_exact^T, |dY| @ |W_exact|^T) in fp64: [rows, K]."""
    W = layer.w_exact()                                          # [K, N]
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


# ---- exact, per expert ---------------------------------------------------------------------------------------------------

def grad_matrix():
    """The 4- and 2-bit rows of grouped_cases.exact_matrix - TileP 32 / 64 x (g 32 bf16, g 64 fp16 with 3 column blocks,
    g 128 bf16 with a pair codebook, g 256 fp16) - at K = 256 and 512, one and two k blocks.  One column block of the
    layout is a single pair of 64-column chunks at 4 bits and TileP 32; three are at least six, across a buffer wrap."""
    out = []
    for bits, tile_p, g, dtype, _, N, pair in exact_matrix():
        if bits == 3:
            continue
        out.append((bits, tile_p, g, dtype, 512 if g in (64, 256) else 256, N, pair))
    return out


def test_matrix_covers_what_it_claims():
    m = grad_matrix()
    for b in (4, 2):
        for p in (32, 64):
            mine = [c for c in m if c[0] == b and c[1] == p]
            assert {c[2] for c in mine} >= {32, 64, 128} and {c[3] for c in mine} == {F16, BF16}
            assert {c[4] for c in mine} == {256, 512} and any(c[6] for c in mine)
            assert {c[5] // XC.cols_per_block(b, p) for c in mine} == {1, 3}
    assert (4, 32, 32, BF16, 256, 128, False) in m                 # N = 128: one chunk pair


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,pair", grad_matrix())
def test_exact_per_expert_and_equal_to_the_slab_form(env, bits, tile_p, g, dtype, K, N, pair):
    layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, len(COUNTS), exact_seed(bits, tile_p, g) + 500)
    Q, S, t2, tid = stack_exact(env, layers)
    R = sum(COUNTS)
    dY = XC.make_x(R, N, exact_seed(bits, tile_p, g) + 577, dtype, witness=False)
    dYd, off = dY.to(env.dev), offsets_of(COUNTS, env.dev)
    dX = env.fa.qgemm_grouped_input_grad(dYd, off, Q, S, t2, bits, g, tid, form="blocks")
    assert dX.shape == (R, K) and dX.dtype == dtype
    check_exact_grad(layers, COUNTS, dY, dX.cpu())
    slabs = env.fa.qgemm_grouped_input_grad(dYd, off, Q, S, t2, bits, g, tid, form="slabs")
    assert torch.equal(bits16(dX), bits16(slabs))


@pytest.fixture(scope="module")
def small_exact(env):
    """Two exact 4-bit stacks and two integer dY shared by the pair, row-weight, ABI, determinism and graph tests: two k
    blocks, six chunks."""
    bits, tile_p, g, dtype, K, N = 4, 32, 64, F16, 512, 3 * 128
    layers = exact_layers(bits, tile_p, g, dtype, K, N, False, len(COUNTS), 9600)
    layers2 = exact_layers(bits, tile_p, g, dtype, K, N, False, len(COUNTS), 9700)
    Q, S, t2, tid = stack_exact(env, layers)
    Q2, S2, t22, _ = stack_exact(env, layers2)
    R = sum(COUNTS)
    dY = XC.make_x(R, N, 9601, dtype, witness=False)
    dY2 = XC.make_x(R, N, 9701, dtype, witness=False)
    return dict(bits=bits, g=g, dtype=dtype, K=K, N=N, counts=COUNTS, R=R, layers=layers, layers2=layers2, tid=tid,
                stack=(Q, S, t2), stack2=(Q2, S2, t22), dY=dY, dY2=dY2)


def test_pair_form_exact(env, small_exact):
    """Two different stacks and two dY against the fp64 sum of both products; 128 N < 2^21."""
    c = small_exact
    assert 128 * c["N"] < XC.EXACT_SUM_LIMIT
    Q2, S2, t22 = c["stack2"]
    args = (c["dY"].to(env.dev), offsets_of(COUNTS, env.dev), *c["stack"], c["bits"], c["g"], c["tid"])
    second = dict(grad_output2=c["dY2"].to(env.dev), weight2=Q2, scales2=S2, table22=t22)
    dX = env.fa.qgemm_grouped_input_grad(*args, **second, form="blocks")
    check_exact_grad(c["layers"], COUNTS, c["dY"], dX.cpu(), dY2=c["dY2"], layers2=c["layers2"])
    assert torch.equal(bits16(dX), bits16(env.fa.qgemm_grouped_input_grad(*args, **second, form="slabs")))
    single = env.fa.qgemm_grouped_input_grad(*args, form="blocks")
    assert not torch.equal(bits16(dX), bits16(single))


def test_row_weight_exact(env, small_exact):
    c = small_exact
    gen = torch.Generator().manual_seed(3)
    choice = torch.tensor([0.25, -0.25, 1.0, -1.0, 2.0, 0.0])       # powers of two, a zero, signs
    rw = choice[torch.randint(0, len(choice), (c["R"],), generator=gen)]
    assert set(rw.tolist()) == set(choice.tolist())
    args = (c["dY"].to(env.dev), offsets_of(COUNTS, env.dev), *c["stack"], c["bits"], c["g"], c["tid"])
    dX = env.fa.qgemm_grouped_input_grad(*args, row_weight=rw.to(env.dev), form="blocks")
    check_exact_grad(c["layers"], COUNTS, c["dY"], dX.cpu(), row_weight=rw)
    assert torch.equal(bits16(dX), bits16(env.fa.qgemm_grouped_input_grad(*args, row_weight=rw.to(env.dev), form="slabs")))


# ---- the direct ABI ------------------------------------------------------------------------------------------------------

def abi_call(env, c, off, ybuf, xbuf, guard, pair=False, form=2):
    d = env.dev
    Q, S, t2 = c["stack"]
    second = (None,) * 4
    if pair:
        Q2, S2, t22 = c["stack2"]
        second = (c["dY2_buf"][guard:].data_ptr(), Q2.data_ptr(), S2.data_ptr(), t22.data_ptr())
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_input_grad_ex(
            0 if c["dtype"] == F16 else 1, c["bits"], c["g"], len(off) - 1, c["R"], c["N"], c["K"], Q.shape[1], c["tid"],
            ybuf[guard:].data_ptr(), off.data_ptr(), Q.data_ptr(), S.data_ptr(), t2.data_ptr(), None, *second,
            xbuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream, form)
    torch.cuda.synchronize()
    return rc


def test_direct_abi_writes_exactly_what_it_says(env, small_exact):
    """dX and dY in the middle of buffers with more guard rows than a block has, dX pre-filled with NaN bits.  offsets[E] in
    {R, 2R/3, 0}: the rows below are the products, the rows from offsets[E] on are zeros, the guards are intact.  Malformed
    tables - entries below 0 and above R, a decreasing pair, overlapping ranges that claim more blocks than the grid holds -
    are memory-safe by the clamping: guards intact.  No input here is meant to fault."""
    c = dict(small_exact)
    d, dtype, K, N, R, E = env.dev, c["dtype"], c["K"], c["N"], c["R"], len(COUNTS)
    guard = 160
    canary = XC.NAN_BITS[dtype]

    def padded(rows):
        buf = torch.full((guard + R + guard, N), 3.0, dtype=dtype, device=d)
        buf[guard:guard + R] = rows.to(d)
        return buf

    ybuf, c["dY2_buf"] = padded(c["dY"]), padded(c["dY2"])
    xbuf = torch.empty((guard + R + guard, K), dtype=torch.int16, device=d)
    full = offsets_of(COUNTS)

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
    # offsets[E] < R behind clamped entries: rows only one expert names hold its product, the tail is zeros
    neg = full.clone()
    neg[:3] = torch.tensor([-5, -1, -70])                          # experts 0 and 1 clamp to no rows, expert 2 to [0, 128)
    dX = run(neg)
    assert XC.exact_equal(dX[128:256], exact_grad(c["dY"][128:256], c["layers"][3])[0], dtype)
    above = full.clone()
    above[-3:] = torch.tensor([R + 1, R + 1000, 2 ** 31 - 1])
    decreasing = full.clone()
    decreasing[3], decreasing[4] = full[4], full[3]
    short = torch.tensor([-5, 100, 50, 400, 400, 400, 400, 400, 500], dtype=torch.int32)      # offsets[E] = 500 < R
    dX = run(short)
    assert torch.all(bits16(dX[500:]) == 0)
    assert XC.exact_equal(dX[100:400], exact_grad(c["dY"][100:400], c["layers"][2])[0], dtype)
    assert XC.exact_equal(dX[400:500], exact_grad(c["dY"][400:500], c["layers"][7])[0], dtype)
    # experts 1, 3, 5 and 7 each claim every row: 24 blocks, the grid holds floor((R + 127 E) / 128) = 13; the surplus is dropped
    assert 4 * -(-R // RB) > (R + (RB - 1) * E) // RB
    greedy = torch.tensor([R, 0, R, 0, R, 0, R, 0, R], dtype=torch.int32)
    for off in (above, decreasing, greedy):
        run(off)
        run(off, pair=True)
    # no expert has a row: zeros everywhere
    assert torch.all(bits16(run(torch.zeros(E + 1, dtype=torch.int32))) == 0)


# ---- the block map -------------------------------------------------------------------------------------------------------

def test_block_map_across_three_rounds_of_the_scan(env):
    """E = 130, rows in experts 0 and 129 only (129 each: two blocks, the second with one row): the scan over the table
    takes three rounds of 64 experts and the second expert's blocks are found in the last."""
    E, bits, tile_p, g, dtype, K, N = 130, 4, 32, 64, F16, 256, 128
    two = exact_layers(bits, tile_p, g, dtype, K, N, False, 2, 9800)
    Q2, S2, t22, tid = stack_exact(env, two)
    Q = torch.zeros((E,) + Q2.shape[1:], dtype=Q2.dtype, device=env.dev)
    S = torch.zeros((E,) + S2.shape[1:], dtype=S2.dtype, device=env.dev)
    t2 = torch.zeros((E,) + t22.shape[1:], dtype=t22.dtype, device=env.dev)
    for i, e in enumerate((0, 129)):
        Q[e], S[e], t2[e] = Q2[i], S2[i], t22[i]
    counts = [0] * E
    counts[0] = counts[129] = 129
    dY = XC.make_x(258, N, 9801, dtype, witness=False)
    dX = env.fa.qgemm_grouped_input_grad(dY.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, bits, g, tid, form="blocks")
    check_exact_grad(two, [129, 129], dY, dX.cpu())


# ---- random data ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,tile_p,g,dtype", [(4, 32, 64, F16), (2, 64, 64, BF16), (4, 64, 128, BF16)])
def test_random_componentwise(env, bits, tile_p, g, dtype):
    """Random codes, scales and tables against the fp64 product with the exact lut * s weight: the gamma bound of an fp32
    sum of N terms over weights rounded once to T, plus the one rounding of the output (XC.assert_componentwise with
    contraction length N) - the slab form's test, at N = 3 column blocks.  And the slab form's bits: the n order is shared."""
    counts = [7, 0, RB + 12]
    K, N = 512, 3 * XC.cols_per_block(bits, tile_p)
    Q, S, t2, Ws = random_stack(env, bits, tile_p, g, dtype, K, N, len(counts), seed=bits * 100 + 41)
    gen = torch.Generator().manual_seed(6)
    dY = torch.randn(sum(counts), N, generator=gen).to(dtype)
    off = offsets_of(counts)
    args = (dY.to(env.dev), off.to(env.dev), Q, S, t2, bits, g, first_template(bits, tile_p))
    dXd = env.fa.qgemm_grouped_input_grad(*args, form="blocks")
    dX = dXd.cpu()
    for e, W in enumerate(Ws):                                    # W [K, N]
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            XC.assert_componentwise(dX[r0:r1], dY[r0:r1], W.T, N, dtype, what=(bits, tile_p, g, dtype, e))
    assert torch.equal(bits16(dXd), bits16(env.fa.qgemm_grouped_input_grad(*args, form="slabs")))


# ---- determinism, graphs -------------------------------------------------------------------------------------------------

def test_equal_bits_over_two_calls_and_in_a_graph(env, small_exact):
    """The grid follows from (E, R, K) alone and the host reads nothing: a captured launch replayed after `offsets` and dY
    were overwritten in place serves the new contents, bit for bit what an eager call on them returns.  One stream."""
    c = small_exact
    R, E = c["R"], len(COUNTS)
    counts2 = [130, 255, 0, 0, 1, 0, R - 130 - 255 - 1 - 3, 3]
    assert sum(counts2) == R and len(counts2) == E and min(counts2) >= 0
    dY2 = XC.make_x(R, c["N"], 9602, c["dtype"], witness=False).to(env.dev)
    off2 = offsets_of(counts2, env.dev)
    dy = c["dY"].to(env.dev).clone()
    off = offsets_of(COUNTS, env.dev)
    run = lambda a, o: env.fa.qgemm_grouped_input_grad(a, o, *c["stack"], c["bits"], c["g"], c["tid"], env.num_sms,
                                                       form="blocks")
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


# ---- the automatic form and the module -------------------------------------------------------------------------------------

def test_automatic_form_takes_blocks_above_the_threshold(env, small_exact):
    c = small_exact
    E = 2
    t = min_mean_rows(env, E, c["K"])
    counts = [t + 70, t - 40] if t > 40 else [t + 30, t]
    R = sum(counts)
    assert R >= t * E
    form = env.dev_mod.grouped_input_grad_form(E, R, c["N"], c["K"], c["bits"], c["g"], c["tid"], env.num_sms, c["dtype"])
    assert form == "blocks"
    assert env.dev_mod.grouped_input_grad_form(E, t * E - 1, c["N"], c["K"], c["bits"], c["g"], c["tid"], env.num_sms,
                                               c["dtype"]) == "slabs"
    Q, S, t2 = (s[:E] for s in c["stack"])
    dY = XC.make_x(R, c["N"], 9603, c["dtype"], witness=False)
    args = (dY.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, c["bits"], c["g"], c["tid"], env.num_sms)
    auto = env.fa.qgemm_grouped_input_grad(*args)
    check_exact_grad(c["layers"][:E], counts, dY, auto.cpu())
    assert torch.equal(bits16(auto), bits16(env.fa.qgemm_grouped_input_grad(*args, form="blocks")))


def test_flute_experts_backward_is_the_composition_on_the_block_form(env):
    """One backward of FluteExperts(fused=True, native_routing=True) at top-1 with a mean row count per expert above the
    threshold: both input-gradient launches - the down projection's with the routing weight in its epilogue, the pair
    form over gate and up - take the block form by themselves, and hidden.grad is, bit for bit, the composition the
    modules' docstrings name with those two launches forced to form="blocks"."""
    fa, d, dtype = env.fa, env.dev, F16
    E, K, F, bits, g = 2, 256, 256, 4, 64
    T = max(300, 2 * E * max(min_mean_rows(env, E, K), min_mean_rows(env, E, F)))
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(61)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    gates, ups, downs = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)], [linear(F, K) for _ in range(E)])
    experts = env.moe.FluteExperts.from_linears(gates, ups, downs, fused=True, native_routing=True)
    hidden = torch.randn(T, K, generator=gen).to(dtype).to(d)
    dOut = torch.randn(T, K, generator=gen).to(dtype).to(d)
    ids = torch.randint(0, E, (T, 1), generator=gen).to(d)
    weights = (torch.rand(T, 1, generator=gen) * 0.5 + 0.5).to(dtype).to(d)
    for N_, K_ in ((K, F), (F, K)):                                # the down projection's launch, the pair launch
        assert env.dev_mod.grouped_input_grad_form(E, T, N_, K_, bits, g, tid, env.num_sms, dtype) == "blocks"

    h = hidden.clone().requires_grad_()
    experts(h, ids, weights).backward(dOut)

    with torch.no_grad():
        offsets, rows, rw, pos, _ = fa.moe_route(ids, weights, E)
    args = (bits, g, tid, env.num_sms)
    gate, up, down = experts.gate, experts.up, experts.down
    y0 = torch.zeros(T, K, dtype=dtype, device=d, requires_grad=True)
    fa.moe_combine(y0, pos, offsets).backward(dOut)                # moe_combine's own gradient: a gather
    with torch.no_grad():
        dh = fa.qgemm_grouped_input_grad(y0.grad, offsets, down.weight, down.scales, down.tables2, *args, row_weight=rw,
                                         form="blocks")
        x = hidden.index_select(0, rows.long())
        gg = fa.qgemm_grouped(x, offsets, gate.weight, gate.scales, gate.tables2, *args).float()
        uu = fa.qgemm_grouped(x, offsets, up.weight, up.scales, up.tables2, *args).float()
        sig = torch.sigmoid(gg)
        dg = (dh.float() * uu * sig * (1 + gg * (1 - sig))).to(dtype)
        du = (dh.float() * (gg * sig)).to(dtype)
        dx = fa.qgemm_grouped_input_grad(dg, offsets, gate.weight, gate.scales, gate.tables2, *args, grad_output2=du,
                                         weight2=up.weight, scales2=up.scales, table22=up.tables2, form="blocks")
        by_hand = fa.moe_combine(dx, pos, offsets)
    assert torch.isfinite(h.grad).all() and float(h.grad.abs().max()) > 0
    assert torch.equal(bits16(h.grad), bits16(by_hand))
