"""flute_amd.qgemm_grouped / flute_qgemm_grouped and integrations.moe on the GPU: all experts of a mixture-of-experts
projection in one launch, from row offsets the host never reads.

Exact inputs (tests/exact_cases) must come back bit for bit per expert, random data within the module's derived
componentwise bound, two calls and a graph replay on other offsets with equal bits, a direct ABI call must write
exactly its rows, the expert bases must survive 32-bit limits, and `FluteExperts` must be as close to the fp64 result
as the per-expert loop over `flute_amd.qgemm` is."""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import (COUNTS, K_CHUNK_CASES, check_exact, exact_layers, exact_matrix, exact_seed, experts_case,  # noqa: F401
                                 random_stack, stack_exact)
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,pair", exact_matrix())
def test_exact_per_expert(env, bits, tile_p, g, dtype, K, N, pair):
    layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, len(COUNTS), exact_seed(bits, tile_p, g))
    Q, S, t2, tid = stack_exact(env, layers)
    T = sum(COUNTS)
    X = XC.make_x(T, K, exact_seed(bits, tile_p, g) + 77, dtype)
    Y = env.fa.qgemm_grouped(X.to(env.dev), offsets_of(COUNTS, env.dev), Q, S, t2, bits, g, tid)
    assert Y.shape == (T, N) and Y.dtype == dtype
    check_exact(env, layers, COUNTS, X, Y.cpu())


def test_exact_several_row_passes(env):
    """300 rows of one expert: more than two passes of the kernel's 32 rows (4 bits), and a short last expert."""
    counts = [300, 0, 0, 5]
    bits, tile_p, g, dtype, K, N = 4, 32, 64, F16, 1088, 3 * 128
    layers = exact_layers(bits, tile_p, g, dtype, K, N, False, 4, 4242)
    Q, S, t2, tid = stack_exact(env, layers)
    X = XC.make_x(sum(counts), K, 4243, dtype)
    Y = env.fa.qgemm_grouped(X.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, bits, g, tid)
    check_exact(env, layers, counts, X, Y.cpu())


@pytest.mark.parametrize("bits,tile_p,K", K_CHUNK_CASES)
def test_exact_across_k_chunks(env, bits, tile_p, K):
    counts = [0, 17, 3]
    g, dtype, N = 32, BF16, XC.cols_per_block(bits, tile_p)
    layers = exact_layers(bits, tile_p, g, dtype, K, N, False, len(counts), 7000 + bits + tile_p)
    Q, S, t2, tid = stack_exact(env, layers)
    X = XC.make_x(sum(counts), K, 7001, dtype)
    Y = env.fa.qgemm_grouped(X.to(env.dev), offsets_of(counts, env.dev), Q, S, t2, bits, g, tid)
    check_exact(env, layers, counts, X, Y.cpu())


@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("bits,tile_p,g,dtype", [(4, 32, 64, F16), (3, 32, 32, BF16), (2, 64, 64, BF16)])
def test_random_componentwise(env, bits, tile_p, g, dtype, nblk):
    counts = [7, 0, 40]
    K, N = 2048 + 64, nblk * XC.cols_per_block(bits, tile_p)
    Q, S, t2, Ws = random_stack(env, bits, tile_p, g, dtype, K, N, len(counts), seed=bits * 100 + nblk)
    gen = torch.Generator().manual_seed(5)
    X = torch.randn(sum(counts), K, generator=gen).to(dtype)
    off = offsets_of(counts)
    Y = env.fa.qgemm_grouped(X.to(env.dev), off.to(env.dev), Q, S, t2, bits, g, first_template(bits, tile_p)).cpu()
    for e, W in enumerate(Ws):
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            XC.assert_componentwise(Y[r0:r1], X[r0:r1], W, K, dtype, what=(bits, tile_p, g, dtype, nblk, e))


@pytest.fixture(scope="module")
def small_exact(env):
    """One exact 4-bit stack shared by the determinism, graph and direct-ABI tests."""
    bits, tile_p, g, dtype, K, N = 4, 32, 64, F16, 1088, 3 * 128
    layers = exact_layers(bits, tile_p, g, dtype, K, N, False, len(COUNTS), 9000)
    Q, S, t2, tid = stack_exact(env, layers)
    X = XC.make_x(sum(COUNTS), K, 9001, dtype)
    return dict(bits=bits, g=g, dtype=dtype, K=K, N=N, layers=layers, Q=Q, S=S, t2=t2, tid=tid, X=X)


def test_two_calls_equal_bits(env, small_exact):
    c = small_exact
    Xd, off = c["X"].to(env.dev), offsets_of(COUNTS, env.dev)
    a = env.fa.qgemm_grouped(Xd, off, c["Q"], c["S"], c["t2"], c["bits"], c["g"], c["tid"])
    b = env.fa.qgemm_grouped(Xd, off, c["Q"], c["S"], c["t2"], c["bits"], c["g"], c["tid"])
    assert torch.equal(bits16(a), bits16(b))


def test_graph_replay_honours_new_offsets(env, small_exact):
    """The host reads nothing: a captured launch replayed after `offsets` and X were overwritten in place serves the new
    distribution, bit for bit what an eager call on it returns."""
    c = small_exact
    T = sum(COUNTS)
    counts2 = [40, 0, 3, 0, 60, 16, 1, 32]
    assert sum(counts2) == T
    X2 = XC.make_x(T, c["K"], 9002, c["dtype"]).to(env.dev)
    off2 = offsets_of(counts2, env.dev)
    x = c["X"].to(env.dev).clone()
    off = offsets_of(COUNTS, env.dev)
    run = lambda: env.fa.qgemm_grouped(x, off, c["Q"], c["S"], c["t2"], c["bits"], c["g"], c["tid"], env.num_sms)
    first = run().clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(first))
    off.copy_(off2)
    x.copy_(X2)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    eager = env.fa.qgemm_grouped(X2, off2, c["Q"], c["S"], c["t2"], c["bits"], c["g"], c["tid"], env.num_sms)
    assert torch.equal(bits16(y), bits16(eager))
    check_exact(env, c["layers"], counts2, X2.cpu(), y.cpu())
    assert not torch.equal(bits16(eager), bits16(first))


def test_direct_abi_writes_exactly_its_rows(env, small_exact):
    """X and Y in the middle of larger buffers, offsets[E] = T + 4: every row index is clamped to T, so the guard rows
    and the rows >= T keep the canary, and the rows < T are the exact product."""
    c = small_exact
    d, dtype, K, N = env.dev, c["dtype"], c["K"], c["N"]
    T, guard, E = sum(COUNTS), 16, len(COUNTS)
    canary = XC.NAN_BITS[dtype]
    ybuf = torch.full((guard + T + guard, N), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + T + guard, K), 3.0, dtype=dtype, device=d)
    xbuf[guard:guard + T] = c["X"].to(d)
    off = offsets_of(COUNTS)
    off[E] = T + 4
    off = off.to(d)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped(
            0 if dtype == F16 else 1, c["bits"], c["g"], E, T, N, K, c["Q"].shape[1], c["tid"],
            xbuf[guard:].data_ptr(), off.data_ptr(), c["Q"].data_ptr(), c["S"].data_ptr(), c["t2"].data_ptr(),
            ybuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(ybuf[:guard] == canary) and torch.all(ybuf[guard + T:] == canary)
    Y = ybuf[guard:guard + T].view(dtype).cpu()
    check_exact(env, c["layers"], COUNTS, c["X"], Y)
    # rows no expert covers are left unwritten: the same call with the last expert's rows given to nobody
    ybuf.fill_(canary)
    off2 = offsets_of(COUNTS)
    off2[E] = off2[E - 1]
    off2 = off2.to(d)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped(
            0 if dtype == F16 else 1, c["bits"], c["g"], E, T, N, K, c["Q"].shape[1], c["tid"],
            xbuf[guard:].data_ptr(), off2.data_ptr(), c["Q"].data_ptr(), c["S"].data_ptr(), c["t2"].data_ptr(),
            ybuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    covered = int(off2[E])
    assert torch.all(ybuf[guard + covered:] == canary) and torch.all(ybuf[:guard] == canary)
    assert torch.equal(ybuf[guard:guard + covered].view(dtype).cpu(), Y[:covered])


def test_past_32_bit_limits(env):
    """136 stacked 8192 x 8192 4-bit experts: Q is 4.25 GiB, so the bases of experts 64 and 135 lie past 2^31 and 2^32
    bytes.  Rows go to experts 0, 64 and 135 only; each is checked against the dense product with its own weights."""
    d = env.dev
    free = torch.cuda.mem_get_info(d)[0]
    if free < 16 * 2 ** 30:
        pytest.skip("needs 16 GiB of free device memory, %.1f GiB free" % (free / 2 ** 30))
    bits, g, dtype, N, K, E = 4, 64, F16, 8192, 8192, 136
    tid = first_template(bits, 32)
    gen = torch.Generator(device=d).manual_seed(11)
    Q = torch.randint(-32768, 32767, (E, bits * N // 16, K), dtype=torch.int16, device=d, generator=gen)
    S = (torch.rand(E, N, K // g, device=d, generator=gen) * 0.02 + 0.005).to(dtype)
    tables = (torch.randn(E, 2 ** bits, device=d, generator=gen)).sort(dim=1).values.to(dtype)
    t2 = torch.stack([env.utils.make_qmap2_from_qmap(t) for t in tables])
    counts = [0] * E
    counts[0], counts[64], counts[135] = 3, 5, 2
    off = offsets_of(counts)
    X = torch.randn(sum(counts), K, device=d, generator=gen).to(dtype)
    Y = env.fa.qgemm_grouped(X, off.to(d), Q, S, t2, bits, g, tid)
    for e in (0, 64, 135):
        r0, r1 = int(off[e]), int(off[e + 1])
        W = env.fa.dequantize(Q[e], S[e], t2[e], bits, g, tid).double().T            # [K, N]
        XC.assert_componentwise(Y[r0:r1], X[r0:r1], W, K, dtype, what=e)
        del W
    del Q, S, Y
    torch.cuda.empty_cache()


def test_flute_experts_against_loop_and_fp64(env, experts_case):
    """FluteExperts against R, the fp64 result from the dequantized weights, and against the per-expert loop over
    flute_amd.qgemm on rows selected on the host (both round at the same places): max|Y - R| <= 2 max|Y_loop - R|."""
    c = experts_case
    d, dtype, E, K, T, bits, g, tid = env.dev, c["dtype"], c["E"], c["K"], c["T"], c["bits"], c["g"], c["tid"]
    gates, ups, downs, hidden, ids, weights = c["gates"], c["ups"], c["downs"], c["hidden"], c["ids"], c["weights"]

    Y = c["experts"](hidden, ids, weights)
    assert Y.shape == (T, K) and Y.dtype == dtype

    # the grouping against the host's
    perm, offsets = env.moe.sort_by_expert(ids, E)
    flat = ids.reshape(-1).cpu().tolist()
    ref_perm = [i for e in range(E) for i, v in enumerate(flat) if v == e]
    assert perm.cpu().tolist() == ref_perm
    assert offsets.cpu().tolist() == [sum(v < e for v in flat) for e in range(E + 1)]
    assert offsets[2] == offsets[3]

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
    print("FluteExperts: max|Y - R| = %.3e, loop max|Y_loop - R| = %.3e, max|R| = %.3e" % (err, err_loop, float(R.abs().max())))
    assert err_loop > 0
    assert err <= 2 * err_loop, (err, err_loop)


def test_flute_experts_forward_in_a_graph(env, experts_case):
    """The whole forward - sort_by_expert, the gathers, three grouped launches, index_add_ - is captured once; after
    topk_ids, the routing weights and the hidden states were overwritten in place, a replay returns what an eager
    call on the new routing returns.  Nothing in it may read the routing on the host (capture would raise)."""
    c = experts_case
    experts, T = c["experts"], c["T"]
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
    assert not torch.equal(ids2, c["ids"])
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
