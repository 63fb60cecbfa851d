"""The block form of the grouped input gradient for stacks of 3-bit experts (qgemm_grouped_input_grad_w3_blocks.h: one workgroup per
128-row block of an expert x 256 k, a three-plane decoder and a two-request dY stager of its own) on the GPU, through
`qgemm_grouped_input_grad_w3_blocks`, at the smallest shapes at which it can still go wrong: empty experts, both sides of a 128-row
block edge, ragged last blocks, one and two k blocks, 8 chunks (one 512-column block of the layout) and 24 (which wrap the double
buffers), malformed tables, graph replay on another table.

Exact inputs (tests/exact_cases) must come back bit for bit per expert; the launch sums over N in the slab form's order, so on
every input - exact or random - its bits must equal `qgemm_grouped_input_grad(..., form="slabs")`."""
import os
import re

import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import counts_of, exact_layers, exact_matrix, exact_seed, random_stack, stack_exact
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
BITS, TILE_P, RB = 3, 32, 128
COUNTS = counts_of(RB)                           # 0, 1, 127, 128, 129, 0, 259, 5: three blocks with a ragged last among them
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")


def exact_grad(dY, layer):
    """(R, A) = (dY @ W_exact^T, |dY| @ |W_exact|^T) in fp64: [rows, K]."""
    W = layer.w_exact()                                          # [K, N]
    d = dY.double()
    return d @ W.T, d.abs() @ W.abs().T


def check_exact_grad(layers, counts, dY, dX, dY2=None, layers2=None, row_weight=None):
    """Per expert: the premise (integer dY in [-4, 4], exact weights <= 16, sum |dY| |w| < 2^21 - then every partial sum in any
    order is exact in fp32 and round_T(R) is the only allowed answer) and dX[r0:r1] == round_T(w_r R) by value."""
    off = offsets_of(counts).tolist()
    dtype = layers[0].dtype
    for e in range(len(layers)):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        R = A = 0
        for rows, lay in ((dY[r0:r1], layers[e]),) + (((dY2[r0:r1], layers2[e]),) if dY2 is not None else ()):
            w = lay.w_exact(0, 256)
            assert torch.equal(w.to(dtype).double(), w) and torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16
            assert torch.equal(rows.double(), rows.double().round()) and rows.double().abs().max() <= 4
            Re, Ae = exact_grad(rows, lay)
            R, A = R + Re, A + Ae
        assert float(A.max()) < XC.EXACT_SUM_LIMIT, ("sum |dY w| reaches 2^21", float(A.max()))
        if row_weight is not None:
            R = R * row_weight[r0:r1].double()[:, None]          # a power of two (or zero) times an exact fp32 sum: exact
        assert torch.isfinite(R.to(dtype)).all()
        assert XC.exact_equal(dX[r0:r1], R, dtype), (e, layers[e])


def grad_matrix():
    """The four 3-bit rows of grouped_cases.exact_matrix - g 32 bf16, g 64 fp16 with N = 3 x 512, g 128 bf16 with a pair codebook,
    g 256 fp16 - at K = 256 and 512: one and two k blocks; N = 512 is 8 chunks, N = 1536 is 24."""
    return [(g, dtype, 512 if g in (64, 256) else 256, N, pair) for bits, _, g, dtype, _, N, pair in exact_matrix() if bits == BITS]


@pytest.mark.parametrize("g,dtype,K,N,pair", grad_matrix())
def test_exact_per_expert_and_equal_to_the_slab_form(env, g, dtype, K, N, pair):
    assert N in (512, 1536) and 4 * 16 * N < XC.EXACT_SUM_LIMIT
    layers = exact_layers(BITS, TILE_P, g, dtype, K, N, pair, len(COUNTS), exact_seed(BITS, TILE_P, g) + 700)
    Q, S, t2, tid = stack_exact(env, layers)
    R = sum(COUNTS)
    dY = XC.make_x(R, N, exact_seed(BITS, TILE_P, g) + 777, dtype, witness=False)
    args = (dY.to(env.dev), offsets_of(COUNTS, env.dev), Q, S, t2, BITS, g, tid)
    dX = env.fa.qgemm_grouped_input_grad_w3_blocks(*args)
    assert dX.shape == (R, K) and dX.dtype == dtype
    check_exact_grad(layers, COUNTS, dY, dX.cpu())
    assert torch.equal(bits16(dX), bits16(env.fa.qgemm_grouped_input_grad(*args, form="slabs")))


@pytest.fixture(scope="module")
def small_exact(env):
    """Two exact stacks and two integer dY shared by the pair, row-weight, ABI and graph tests: two k blocks, 8 chunks."""
    g, dtype, K, N = 64, F16, 512, 512
    layers = exact_layers(BITS, TILE_P, g, dtype, K, N, False, len(COUNTS), 39600)
    layers2 = exact_layers(BITS, TILE_P, g, dtype, K, N, False, len(COUNTS), 39700)
    Q, S, t2, tid = stack_exact(env, layers)
    Q2, S2, t22, _ = stack_exact(env, layers2)
    R = sum(COUNTS)
    return dict(g=g, dtype=dtype, K=K, N=N, R=R, layers=layers, layers2=layers2, tid=tid, stack=(Q, S, t2), stack2=(Q2, S2, t22),
                dY=XC.make_x(R, N, 39601, dtype, witness=False), dY2=XC.make_x(R, N, 39701, dtype, witness=False))


def test_pair_form_and_row_weight_exact(env, small_exact):
    """Two different stacks and two dY against the fp64 sum of both products (128 N < 2^21); power-of-two row weights with a zero
    and signs.  Both exact, both with the slab form's bits."""
    c = small_exact
    assert 128 * c["N"] < XC.EXACT_SUM_LIMIT
    Q2, S2, t22 = c["stack2"]
    args = (c["dY"].to(env.dev), offsets_of(COUNTS, env.dev), *c["stack"], BITS, c["g"], c["tid"])
    second = dict(grad_output2=c["dY2"].to(env.dev), weight2=Q2, scales2=S2, table22=t22)
    dX = env.fa.qgemm_grouped_input_grad_w3_blocks(*args, **second)
    check_exact_grad(c["layers"], COUNTS, c["dY"], dX.cpu(), dY2=c["dY2"], layers2=c["layers2"])
    assert torch.equal(bits16(dX), bits16(env.fa.qgemm_grouped_input_grad(*args, **second, form="slabs")))
    assert not torch.equal(bits16(dX), bits16(env.fa.qgemm_grouped_input_grad_w3_blocks(*args)))
    choice = torch.tensor([0.25, -0.25, 1.0, -1.0, 2.0, 0.0])
    rw = choice[torch.randint(0, len(choice), (c["R"],), generator=torch.Generator().manual_seed(3))]
    assert set(rw.tolist()) == set(choice.tolist())
    dX = env.fa.qgemm_grouped_input_grad_w3_blocks(*args, row_weight=rw.to(env.dev))
    check_exact_grad(c["layers"], COUNTS, c["dY"], dX.cpu(), row_weight=rw)
    assert torch.equal(bits16(dX), bits16(env.fa.qgemm_grouped_input_grad(*args, row_weight=rw.to(env.dev), form="slabs")))


@pytest.mark.parametrize("g,dtype", [(64, F16), (128, BF16)])
def test_random_componentwise(env, g, dtype):
    """Random codes, scales and tables against the fp64 product with the exact lut * s weight: the gamma bound of an fp32 sum of N
    terms over weights rounded once to T, plus the one rounding of the output (XC.assert_componentwise with contraction length N)."""
    counts = [7, 0, RB + 12]
    K, N = 512, 1536
    Q, S, t2, Ws = random_stack(env, BITS, TILE_P, g, dtype, K, N, len(counts), seed=341 + g)
    dY = torch.randn(sum(counts), N, generator=torch.Generator().manual_seed(6)).to(dtype)
    off = offsets_of(counts)
    args = (dY.to(env.dev), off.to(env.dev), Q, S, t2, BITS, g, first_template(BITS, TILE_P))
    dXd = env.fa.qgemm_grouped_input_grad_w3_blocks(*args)
    dX = dXd.cpu()
    for e, W in enumerate(Ws):                                    # W [K, N]
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            XC.assert_componentwise(dX[r0:r1], dY[r0:r1], W.T, N, dtype, what=(g, dtype, e))
    assert torch.equal(bits16(dXd), bits16(env.fa.qgemm_grouped_input_grad(*args, form="slabs")))


def test_direct_abi_writes_exactly_what_it_says(env, small_exact):
    """dX and dY in the middle of buffers with more guard rows than a block has, dX pre-filled with NaN bits.  offsets[E] in
    {R, 2R/3, 0}: the rows below are the products, the rows from offsets[E] on are zeros, the guards are intact.  Malformed
    tables - entries below 0 and above R, a decreasing pair, ranges that claim more blocks than the grid holds - are memory-safe
    by the clamping contract of grouped_rows.h: guards intact.  No input here is meant to fault."""
    c = small_exact
    d, dtype, K, N, R, E = env.dev, c["dtype"], c["K"], c["N"], c["R"], len(COUNTS)
    guard = 160
    canary = XC.NAN_BITS[dtype]
    (Q, S, t2), (Q2, S2, t22) = c["stack"], c["stack2"]

    def padded(rows):
        buf = torch.full((guard + R + guard, N), 3.0, dtype=dtype, device=d)
        buf[guard:guard + R] = rows.to(d)
        return buf

    ybuf, ybuf2 = padded(c["dY"]), padded(c["dY2"])
    xbuf = torch.empty((guard + R + guard, K), dtype=torch.int16, device=d)
    full = offsets_of(COUNTS)

    def run(off, pair=False):
        off = off.to(d)
        second = (ybuf2[guard:].data_ptr(), Q2.data_ptr(), S2.data_ptr(), t22.data_ptr()) if pair else (None,) * 4
        xbuf.fill_(canary)
        with torch.cuda.device(d):
            rc = env.lib.flute_qgemm_grouped_input_grad_w3_blocks(
                0, BITS, c["g"], E, R, N, K, Q.shape[1], c["tid"], ybuf[guard:].data_ptr(), off.data_ptr(), Q.data_ptr(),
                S.data_ptr(), t2.data_ptr(), None, *second, xbuf[guard:].data_ptr(), env.num_sms,
                torch.cuda.current_stream(d).cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.all(xbuf[:guard] == canary) and torch.all(xbuf[guard + R:] == canary)
        return xbuf[guard:guard + R].view(dtype).cpu()

    for zb in (R, 2 * R // 3, 0):
        off = full.clamp(max=zb)                                   # a proper table whose last entry is zb
        dX = run(off)
        check_exact_grad(c["layers"], (off[1:] - off[:-1]).tolist(), c["dY"], dX)
        assert torch.all(bits16(dX[zb:]) == 0), zb                 # every row is written: zeros where no expert serves
        assert not torch.any(bits16(dX) == canary)
    dX = run(full.clamp(max=2 * R // 3), pair=True)
    assert torch.all(bits16(dX[2 * R // 3:]) == 0) and not torch.any(bits16(dX) == canary)
    neg = full.clone()
    neg[:3] = torch.tensor([-5, -1, -70])                          # experts 0 and 1 clamp to no rows, expert 2 to [0, 128)
    dX = run(neg)
    assert XC.exact_equal(dX[128:256], exact_grad(c["dY"][128:256], c["layers"][3])[0], dtype)
    above = full.clone()
    above[-3:] = torch.tensor([R + 1, R + 1000, 2 ** 31 - 1])
    decreasing = full.clone()
    decreasing[3], decreasing[4] = full[4], full[3]
    # experts 1, 3, 5 and 7 each claim every row: 24 blocks, the grid holds floor((R + 127 E) / 128) = 13; the surplus is dropped
    assert 4 * -(-R // RB) > (R + (RB - 1) * E) // RB
    greedy = torch.tensor([R, 0, R, 0, R, 0, R, 0, R], dtype=torch.int32)
    for off in (above, decreasing, greedy):
        run(off)
        run(off, pair=True)
    assert torch.all(bits16(run(torch.zeros(E + 1, dtype=torch.int32))) == 0)      # no expert has a row: zeros everywhere


def test_graph_replay_serves_the_new_table(env, small_exact):
    """The grid follows from (E, R, K) alone and the host reads nothing: a captured launch replayed after `offsets` and dY were
    overwritten in place serves the new contents, bit for bit what an eager call on them returns.  One stream."""
    c = small_exact
    R, E = c["R"], len(COUNTS)
    counts2 = [130, 255, 0, 0, 1, 0, R - 130 - 255 - 1 - 3, 3]
    assert sum(counts2) == R and len(counts2) == E and min(counts2) >= 0
    dY2 = XC.make_x(R, c["N"], 39602, c["dtype"], witness=False).to(env.dev)
    off2 = offsets_of(counts2, env.dev)
    dy, off = c["dY"].to(env.dev).clone(), offsets_of(COUNTS, env.dev)
    run = lambda a, o: env.fa.qgemm_grouped_input_grad_w3_blocks(a, o, *c["stack"], BITS, c["g"], c["tid"], env.num_sms)
    first = run(dy, off).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dx = run(dy, off)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(dx), bits16(first))
    off.copy_(off2)
    dy.copy_(dY2)
    for _ in range(2):                                            # more than one replay against the eager result
        dx.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(dY2, off2)
        assert torch.equal(bits16(dx), bits16(eager))
    check_exact_grad(c["layers"], counts2, dY2.cpu(), dx.cpu())
    assert not torch.equal(bits16(eager), bits16(first))


def test_flute_experts_backward_keeps_its_bits(env):
    """One backward of a 3-bit FluteExperts(fused=True, native_routing=True) at top-1 with a mean row count per expert above both
    thresholds of the header: with `w3_grad_blocks=True` (and with "auto", which then takes the same launches) hidden.grad is, bit
    for bit, the default's."""
    with open(HEADER) as f:
        thr = max(int(v) for v in re.findall(r"#define FLUTE_GROUPED_INPUT_GRAD_W3_BLOCKS_MIN_MEAN_ROWS\w* (\d+)\b", f.read()))
    E, K, F, g, dtype, d = 2, 512, 512, 64, F16, env.dev
    T = max(300, E * thr + 1)
    tid, gen = first_template(BITS, TILE_P), torch.Generator().manual_seed(39900)
    table = torch.randn(8, generator=gen).sort().values.to(dtype).to(d)

    def linear(kk, nn):
        codes = torch.randint(0, 8, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, table, BITS, g, tid)

    layers = [[linear(kk, nn) for _ in range(E)] for kk, nn in ((K, F), (K, F), (F, K))]
    hidden = torch.randn(T, K, generator=gen).to(dtype).to(d)
    dOut = torch.randn(T, K, generator=gen).to(dtype).to(d)
    ids = torch.randint(0, E, (T, 1), generator=gen).to(d)
    weights = (torch.rand(T, 1, generator=gen) * 0.5 + 0.5).to(dtype).to(d)
    for N_, K_ in ((K, F), (F, K)):
        assert env.dev_mod.grouped_input_grad_w3_blocks_form(E, T, N_, K_, g, tid, env.num_sms, dtype) == "blocks"
    grads = {}
    for value in (False, True, "auto"):
        experts = env.moe.FluteExperts.from_linears(*layers, fused=True, native_routing=True, w3_grad_blocks=value)
        h = hidden.clone().requires_grad_()
        experts(h, ids, weights).backward(dOut)
        grads[value] = h.grad
    assert torch.isfinite(grads[False]).all() and float(grads[False].abs().max()) > 0
    assert torch.equal(bits16(grads[True]), bits16(grads[False])) and torch.equal(bits16(grads["auto"]), bits16(grads[False]))
