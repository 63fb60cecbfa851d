"""flute_amd.qgemm_grouped_glu / qgemm_grouped_weighted (qgemm_grouped.h) and FluteExperts(fused=True) on the GPU.

GLU.  Gate and up are exact stacks (tests/exact_cases) with different seeds and X = make_x(...) * 2^-p, still exact in T, so
g = x @ Wgate^T and u = x @ Wup^T are exact in fp32 whatever the summation order.  With E = g / (1 + e^-g) * u in fp64 the
documented arithmetic (include/flute_amd.h) allows

    |H - E| <= (u_T + eps_s (1 + u_T)) |E| + eta_T,      eps_s = 2^-21 (the header's derivation), eta_T = 2^-24 / 2^-126,

element by element: under 1.13 u_T, so a wrong slab pairing or a wrong row (off by O(1)) cannot hide.  p is chosen on the CPU
so that a quarter of the elements have 0.25 <= |g| <= 8, where silu is neither the identity nor zero; the premises are asserted.

Weighted.  row_weight from {0.25, 0.5, 0.75, 1, 1.5} on exact layers: w * R is exact in fp32 while |R| < 2^19, so
Y = round_T(w R) bit for bit; the rows from offsets[E] on are zeros, everything outside [0, T) keeps its canary.

Module.  FluteExperts(fused=True) against the fp64 result within twice the per-expert loop's own error, in a graph, and
the default path bit for bit what it was."""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import (COUNTS, K_CHUNK_CASES, assert_glu, draw_row_weights, exact_layers, exact_matrix,  # noqa: F401
                                 exact_seed, experts_case, random_stack, stack_exact, weighted_expected)
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
TSRC = 40


def draw_rows(R, tsrc, seed):
    """R source rows with repeats; the last one is the accumulator witness (the last row of make_x)."""
    rows = torch.randint(0, tsrc, (R,), generator=torch.Generator().manual_seed(seed))
    rows[-1] = tsrc - 1
    return rows


def exact_in_fp32(x, lay, A, witness):
    """exact_cases.premise without its demand that the product fits T: g and u stay in fp32 here and are never rounded to T."""
    xd = x.double()
    assert torch.equal(xd, xd.round()) and xd.abs().max() <= 4, "activations: integers in [-4, 4]"
    w = lay.w_exact(0, min(lay.N, 256))
    assert torch.equal(w.to(lay.dtype).double(), w) and torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16
    assert float(A.max()) < XC.EXACT_SUM_LIMIT, ("sum |x w| reaches 2^21", float(A.max()))
    if witness:
        XC.assert_witness(xd[-1], w, lay.dtype)


def glu_reference(gate, up, counts, Xi, rows):
    """For integer activations Xi [Tsrc, K] read through `rows` [R]: the power p, X = Xi 2^-p in T and E [R, F] fp64, with
    every premise of the bound asserted."""
    dtype = gate[0].dtype
    off = offsets_of(counts).tolist()
    R = off[-1]
    assert rows.shape == (R,) and int(rows[-1]) == Xi.shape[0] - 1
    G = torch.zeros(R, gate[0].N, dtype=torch.float64)
    U = torch.zeros_like(G)
    for e in range(len(counts)):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        x = Xi[rows[r0:r1]]
        for lay, out in ((gate[e], G), (up[e], U)):
            P, A = XC.exact_product(x, lay, abs_too=True)
            exact_in_fp32(x, lay, A, witness=(r1 == R))
            out[r0:r1] = P
    share = lambda p: float(((G.abs() * 2.0 ** -p >= 0.25) & (G.abs() * 2.0 ** -p <= 8)).double().mean())
    p = max((p for p in range(0, 20) if float(G.abs().max()) * 2.0 ** -p <= 88), key=share)     # silu32's eps_s holds for |g| <= 88
    X = (Xi.double() * 2.0 ** -p).to(dtype)
    assert torch.equal(X.double(), Xi.double() * 2.0 ** -p), "X 2^-p is exact in T"
    g, u = G * 2.0 ** -p, U * 2.0 ** -p
    E = g / (1 + torch.exp(-g)) * u
    assert share(p) >= 0.25, ("a quarter of the elements with 0.25 <= |g| <= 8", p, share(p))
    assert float(g.abs().max()) <= 88, float(g.abs().max())
    if dtype == F16:
        assert float(E.abs().max()) < XC.FP16_MAX / 2, float(E.abs().max())
    return dict(p=p, X=X, E=E, share=share(p))


class GluCase:
    """Two exact stacks on the device and, per (counts, rows, Xi), the reference."""

    def __init__(self, env, bits, tile_p, g, dtype, K, N, pair, E, seed):
        self.bits, self.g, self.dtype, self.K, self.N, self.E = bits, g, dtype, K, N, E
        self.gate = exact_layers(bits, tile_p, g, dtype, K, N, pair, E, seed)
        self.up = exact_layers(bits, tile_p, g, dtype, K, N, pair, E, seed + 500)
        self.Qg, self.Sg, self.Tg, self.tid = stack_exact(env, self.gate)
        self.Qu, self.Su, self.Tu, _ = stack_exact(env, self.up)
        self.env = env

    def ops(self):
        return (self.Qg, self.Sg, self.Tg, self.Qu, self.Su, self.Tu)

    def run(self, X, off, rows):
        return self.env.fa.qgemm_grouped_glu(X, off, *self.ops(), self.bits, self.g, self.tid, self.env.num_sms, rows=rows)

    def check(self, counts, Xi, rows, what, use_rows=True):
        d = self.env.dev
        ref = glu_reference(self.gate, self.up, counts, Xi, rows)
        H = self.run(ref["X"].to(d), offsets_of(counts, d), rows.int().to(d) if use_rows else None)
        assert H.shape == (sum(counts), self.N) and H.dtype == self.dtype
        assert_glu(H, ref["E"], self.dtype, (what, "p = %d" % ref["p"], "share %.2f" % ref["share"]))
        return ref, H


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,pair", exact_matrix())
def test_glu_main_matrix(env, bits, tile_p, g, dtype, K, N, pair):
    seed = exact_seed(bits, tile_p, g) + 31
    c = GluCase(env, bits, tile_p, g, dtype, K, N, pair, len(COUNTS), seed)
    Xi = XC.make_x(TSRC, K, seed + 77, dtype)
    c.check(COUNTS, Xi, draw_rows(sum(COUNTS), TSRC, seed + 78), (bits, tile_p, g, dtype, K, N, pair))


def test_glu_several_row_passes(env):
    """300 rows of one expert: more than two passes of the kernel's 32 rows, and a short last expert."""
    counts = [300, 0, 0, 5]
    c = GluCase(env, 4, 32, 64, F16, 1088, 3 * 128, False, 4, 5242)
    c.check(counts, XC.make_x(TSRC, 1088, 5243, F16), draw_rows(sum(counts), TSRC, 5244), "row passes")


@pytest.mark.parametrize("bits,tile_p,K", [k for k in K_CHUNK_CASES if k[1] == 32])
def test_glu_across_k_chunks(env, bits, tile_p, K):
    """One case per bit width: the scale panel is staged a second time for each of the two stacks."""
    counts = [0, 17, 3]
    N = XC.cols_per_block(bits, tile_p)
    c = GluCase(env, bits, tile_p, 32, BF16, K, N, False, len(counts), 8000 + bits)
    c.check(counts, XC.make_x(TSRC, K, 8001, BF16), draw_rows(sum(counts), TSRC, 8002), ("k chunks", bits, K))


@pytest.fixture(scope="module")
def glu_small(env):
    """One exact 4-bit pair of stacks shared by the index-free, determinism, graph and direct-ABI tests."""
    return GluCase(env, 4, 32, 64, F16, 1088, 3 * 128, False, len(COUNTS), 9100)


def test_glu_without_an_index(env, glu_small):
    R = sum(COUNTS)
    glu_small.check(COUNTS, XC.make_x(R, glu_small.K, 9101, F16), torch.arange(R), "rows = None", use_rows=False)


def test_glu_two_calls_equal_bits(env, glu_small):
    c, d = glu_small, env.dev
    rows = draw_rows(sum(COUNTS), TSRC, 9102).int().to(d)
    X = (XC.make_x(TSRC, c.K, 9103, F16) / 64).to(d)
    off = offsets_of(COUNTS, d)
    a, b = c.run(X, off, rows), c.run(X, off, rows)
    assert torch.equal(bits16(a), bits16(b))
    assert not torch.equal(bits16(a), bits16(c.run(X, off, rows.flip(0).contiguous())))


def test_glu_graph_replay_honours_new_offsets_rows_and_x(env, glu_small):
    """The host reads nothing: a captured launch replayed after offsets, rows and X were overwritten in place serves the new
    data, bit for bit what an eager call on it returns."""
    c, d = glu_small, env.dev
    R = sum(COUNTS)
    counts2 = [40, 0, 3, 0, 60, 16, 1, 32]
    assert sum(counts2) == R
    rows1, rows2 = draw_rows(R, TSRC, 9104), draw_rows(R, TSRC, 9105)
    ref1 = glu_reference(c.gate, c.up, COUNTS, XC.make_x(TSRC, c.K, 9106, F16), rows1)
    ref2 = glu_reference(c.gate, c.up, counts2, XC.make_x(TSRC, c.K, 9107, F16), rows2)
    x, off, rows = ref1["X"].to(d).clone(), offsets_of(COUNTS, d), rows1.int().to(d)
    first = c.run(x, off, rows).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h = c.run(x, off, rows)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(h), bits16(first))
    off.copy_(offsets_of(counts2, d))
    rows.copy_(rows2.int().to(d))
    x.copy_(ref2["X"].to(d))
    h.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = c.run(ref2["X"].to(d), offsets_of(counts2, d), rows2.int().to(d))
    assert torch.equal(bits16(h), bits16(eager))
    assert_glu(h, ref2["E"], F16, "graph replay")
    assert not torch.equal(bits16(eager), bits16(first))


def test_glu_direct_abi_clamps_and_writes_exactly_its_rows(env, glu_small):
    """H and Xsrc in the middle of larger buffers, offsets[E] = R + 4, one index -1 and one >= Tsrc: the rows < R are within
    the bound of the clamped source rows' result, a clamped row has the bits of the row that names the clamped index, and
    the guard rows and the rows >= R keep the canary."""
    c, d, dtype = glu_small, env.dev, F16
    R, E, guard = sum(COUNTS), len(COUNTS), 16
    off_host = offsets_of(COUNTS)
    r0 = int(off_host[E - 1])                                  # the last expert has 70 rows
    rows = draw_rows(R, TSRC, 9108)
    rows[r0:r0 + 4] = torch.tensor([-1, 0, TSRC + 5, TSRC - 1])
    ref = glu_reference(c.gate, c.up, COUNTS, XC.make_x(TSRC, c.K, 9109, dtype), rows.clamp(0, TSRC - 1))
    canary = XC.NAN_BITS[dtype]
    hbuf = torch.full((guard + R + guard, c.N), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + TSRC + guard, c.K), 3.0, dtype=dtype, device=d)
    xbuf[guard:guard + TSRC] = ref["X"].to(d)
    off_host[E] = R + 4
    off, rows_d = off_host.to(d), rows.int().to(d)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_glu(
            0, c.bits, c.g, E, R, TSRC, c.N, c.K, c.Qg.shape[1], c.tid, xbuf[guard:].data_ptr(), rows_d.data_ptr(),
            off.data_ptr(), *[t.data_ptr() for t in c.ops()], hbuf[guard:].data_ptr(), env.num_sms,
            torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(hbuf[:guard] == canary) and torch.all(hbuf[guard + R:] == canary)
    H = hbuf[guard:guard + R].view(dtype)
    assert_glu(H, ref["E"], dtype, "direct ABI")
    assert torch.equal(bits16(H[r0]), bits16(H[r0 + 1])) and torch.equal(bits16(H[r0 + 2]), bits16(H[r0 + 3]))
    assert not torch.equal(bits16(H[r0]), bits16(H[r0 + 2]))


# ---- the weighted down projection ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,tile_p,g,dtype,K,nblk,pair", [(4, 32, 64, F16, 1088, 3, False), (4, 64, 256, F16, 4352, 1, False),
                                                             (2, 64, 128, BF16, 2048, 1, True), (2, 32, 32, BF16, 64, 1, False),
                                                             (3, 32, 64, F16, 1088, 3, False)])
def test_weighted_exact_products(env, bits, tile_p, g, dtype, K, nblk, pair):
    N = nblk * XC.cols_per_block(bits, tile_p)
    layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, len(COUNTS), 6000 + bits + tile_p)
    Q, S, t2, tid = stack_exact(env, layers)
    T = sum(COUNTS)
    X, w = XC.make_x(T, K, 6001, dtype), draw_row_weights(T, 6002)
    want = weighted_expected(layers, COUNTS, X, w)
    Y = env.fa.qgemm_grouped_weighted(X.to(env.dev), offsets_of(COUNTS, env.dev), Q, S, t2, w.to(env.dev), bits, g, tid,
                                      env.num_sms)
    assert Y.shape == (T, N) and Y.dtype == dtype
    assert XC.exact_equal(Y, want, dtype)


@pytest.fixture(scope="module")
def weighted_small(env):
    bits, tile_p, g, dtype, K, N = 4, 32, 64, F16, 1088, 3 * 128
    layers = exact_layers(bits, tile_p, g, dtype, K, N, False, len(COUNTS), 9200)
    Q, S, t2, tid = stack_exact(env, layers)
    T = sum(COUNTS)
    X, w = XC.make_x(T, K, 9201, dtype), draw_row_weights(T, 9202)
    return dict(bits=bits, g=g, dtype=dtype, K=K, N=N, layers=layers, Q=Q, S=S, t2=t2, tid=tid, X=X, w=w,
                want=weighted_expected(layers, COUNTS, X, w))


def weighted_abi(env, c, off):
    """The direct call with X and Y in the middle of larger buffers: (front guard, rows [0, T), rows >= T) of Y as int16."""
    d, dtype, K, N = env.dev, c["dtype"], c["K"], c["N"]
    T, guard, E = sum(COUNTS), 16, len(COUNTS)
    canary = XC.NAN_BITS[dtype]
    ybuf = torch.full((guard + T + guard, N), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + T + guard, K), 3.0, dtype=dtype, device=d)
    xbuf[guard:guard + T] = c["X"].to(d)
    off, w = off.to(d), c["w"].to(d)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_weighted(
            0 if dtype == F16 else 1, c["bits"], c["g"], E, T, N, K, c["Q"].shape[1], c["tid"], xbuf[guard:].data_ptr(),
            off.data_ptr(), c["Q"].data_ptr(), c["S"].data_ptr(), c["t2"].data_ptr(), w.data_ptr(), ybuf[guard:].data_ptr(),
            env.num_sms, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(ybuf[:guard] == canary), "front guard"
    assert torch.all(ybuf[guard + T:] == canary), "rows >= T"
    return ybuf[guard:guard + T].cpu()


def test_weighted_zero_fill_reduced_last_offset(env, weighted_small):
    """offsets[E] reduced so that the last expert's rows belong to nobody: those rows are exactly zero."""
    c, E = weighted_small, len(COUNTS)
    off = offsets_of(COUNTS)
    off[E] = off[E - 1]
    covered = int(off[E])
    Y = weighted_abi(env, c, off)
    assert covered < sum(COUNTS) and torch.all(Y[covered:] == 0)
    assert XC.exact_equal(Y[:covered].view(c["dtype"]), c["want"][:covered], c["dtype"])
    # past the end instead: clamped to T, every row served, nothing zeroed
    off = offsets_of(COUNTS)
    off[E] += 4
    assert XC.exact_equal(weighted_abi(env, c, off).view(c["dtype"]), c["want"], c["dtype"])


def test_weighted_zero_fill_all_offsets_zero(env, weighted_small):
    """No expert has a row: the launch still writes every row of [0, T) as zeros and nothing else."""
    Y = weighted_abi(env, weighted_small, torch.zeros(len(COUNTS) + 1, dtype=torch.int32))
    assert torch.all(Y == 0)


@pytest.mark.parametrize("bits,tile_p,g,dtype", [(4, 32, 64, F16), (2, 64, 64, BF16), (3, 32, 32, BF16)])
def test_weighted_by_one_is_the_plain_form(env, bits, tile_p, g, dtype):
    """row_weight = 1 and offsets[E] = T: the fp32 product by 1.0 is exact, so the weighted form is the plain form bit for bit on
    every row (one kernel template, qgemm_grouped.h).  K = 1088: each of the eight waves gets a block and the last block is
    short; N: the smallest the template takes, two slabs or more.  Then offsets[E] lowered by 17: equal below it, zeros from it on."""
    K, N, E, T = 1088, XC.cols_per_block(bits, tile_p), len(COUNTS), sum(COUNTS)
    Q, S, t2, _ = random_stack(env, bits, tile_p, g, dtype, K, N, E, seed=8800 + bits)
    X = torch.randn(T, K, generator=torch.Generator().manual_seed(8801)).to(dtype).to(env.dev)
    off, ones = offsets_of(COUNTS, env.dev), torch.ones(T, device=env.dev)
    tid = first_template(bits, tile_p)
    plain = bits16(env.fa.qgemm_grouped(X, off, Q, S, t2, bits, g, tid, env.num_sms))
    assert torch.equal(bits16(env.fa.qgemm_grouped_weighted(X, off, Q, S, t2, ones, bits, g, tid, env.num_sms)), plain)
    cut = T - 17
    off[E] = cut
    short = bits16(env.fa.qgemm_grouped_weighted(X, off, Q, S, t2, ones, bits, g, tid, env.num_sms))
    assert torch.equal(short[:cut], plain[:cut]) and torch.all(short[cut:] == 0)


# ---- the module --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fused_experts(env, experts_case):
    c = experts_case
    return env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=True)


def test_fused_experts_against_loop_and_fp64(env, experts_case, fused_experts):
    """R, Y_loop as tests/test_grouped_gpu.py::test_flute_experts_against_loop_and_fp64 computes them:
    max|Y_fused - R| <= 2 max|Y_loop - R|."""
    c = experts_case
    d, dtype, E, K, T, bits, g, tid = env.dev, c["dtype"], c["E"], c["K"], c["T"], c["bits"], c["g"], c["tid"]
    gates, ups, downs, hidden, ids, weights = c["gates"], c["ups"], c["downs"], c["hidden"], c["ids"], c["weights"]
    assert fused_experts.fused is True
    Y = fused_experts(hidden, ids, weights)
    assert Y.shape == (T, K) and Y.dtype == dtype

    deq = lambda m: env.fa.dequantize(m.weight, m.scales, m.tables2, bits, g, tid)
    silu = torch.nn.functional.silu
    R = torch.zeros(T, K, dtype=torch.float64, device=d)
    Y_loop = torch.zeros(T, K, dtype=dtype, device=d)
    for e in range(E):
        tok, slot = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        x = hidden[tok]
        wgt = weights[tok, slot]
        xd = x.double()
        h = silu(xd @ deq(gates[e]).double().T) * (xd @ deq(ups[e]).double().T)
        R.index_add_(0, tok, (h @ deq(downs[e]).double().T) * wgt.double()[:, None])
        hl = silu(gates[e](x)) * ups[e](x)
        Y_loop.index_add_(0, tok, downs[e](hl) * wgt[:, None])
    err = float((Y.double() - R).abs().max())
    err_loop = float((Y_loop.double() - R).abs().max())
    print("FluteExperts(fused=True): max|Y_fused - R| = %.3e, loop max|Y_loop - R| = %.3e, max|R| = %.3e"
          % (err, err_loop, float(R.abs().max())))
    assert err_loop > 0
    assert err <= 2 * err_loop, (err, err_loop)


def test_fused_experts_forward_in_a_graph(env, experts_case, fused_experts):
    """sort_by_expert, the two fused launches and index_add_ captured once; after topk_ids, the routing weights and the
    hidden states were overwritten in place a replay returns the bits of an eager call on the new routing."""
    c, experts = experts_case, fused_experts
    hidden, ids, weights = c["hidden"].clone(), c["ids"].clone(), c["weights"].clone()
    first = experts(hidden, ids, weights).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = experts(hidden, ids, weights)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(first))
    ids2 = c["ids2"]
    hidden2, weights2 = c["hidden"].flip(0).contiguous(), c["weights"].flip(1).contiguous()
    ids.copy_(ids2)
    hidden.copy_(hidden2)
    weights.copy_(weights2)
    graph.replay()
    torch.cuda.synchronize()
    eager = experts(hidden2, ids2, weights2)
    assert torch.equal(bits16(y), bits16(eager))
    assert not torch.equal(bits16(eager), bits16(first))
    # ids outside [0, E) are served by no expert and contribute nothing: a token routed only there comes back zero
    ids3 = ids2.clone()
    ids3[0] = torch.tensor([c["E"], -1], device=ids3.device)
    out = experts(hidden2, ids3, weights2)
    assert torch.all(out[0] == 0) and torch.isfinite(out).all()
    assert torch.equal(bits16(out[1:]), bits16(eager[1:]))


def test_default_path_keeps_its_bits(env, experts_case):
    """fused=False is the forward FluteExperts had before the argument existed."""
    c = experts_case
    off = env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=False)
    assert off.fused is False and c["experts"].fused is False
    a = off(c["hidden"], c["ids"], c["weights"])
    b = c["experts"](c["hidden"], c["ids"], c["weights"])
    assert torch.equal(bits16(a), bits16(b))
