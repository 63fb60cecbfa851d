"""flute_amd.moe_route / moe_combine (moe_route.hip, moe_combine.hip) and FluteExperts(native_routing=True) on the GPU.

Route.  Integers only: every output equals a naive Python loop on the host, value for value, and `perm` / `offsets` also
equal integrations.moe.sort_by_expert's on the same ids; both id widths, the three weight dtypes and no weights; every
output inside a canary-padded buffer.

Combine.  Bit for bit a torch restatement of the contract (include/flute_amd.h, flute_moe_combine): fp32 additions in
slot order from +0, skipped slots adding +0, one rounding.  At k = 8 also element by element against the fp64 sum S,

    |out - S| <= u_T |S| + (k - 1) 2^-24 sum_j |y_j| + eta_T,

the bound of k - 1 fp32 additions (each partial sum is at most sum |y_j| in magnitude, each addition within 2^-24
relative) and one rounding to T (eta_T: T's smallest subnormal step, as in tests/grouped_cases.py).

Module.  FluteExperts(native_routing=True) bit for bit what the same launches give when sort_by_expert drives them and
the torch restatement combines them; top-3 against fp64 within twice the per-expert loop's own error; in a graph; ids
outside [0, E); and the default path bit for bit what it was."""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import experts_case  # noqa: F401
from tests.moe_cases import CANARY, GUARD, canary_padded, host_route, intact, native, top3_case  # noqa: F401
from tests.support import bits16, env  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
I32, I64 = torch.int32, torch.int64
ETA = {F16: 2.0 ** -24, BF16: 2.0 ** -126}
ID_CODE = {I32: 0, I64: 1}
WEIGHT_CODE = {F16: 0, BF16: 1, F32: 2}


# ---- route ---------------------------------------------------------------------------------------------------------------

def route_abi(env, ids, weights, E):
    """The direct call with every output in the middle of a larger buffer: (offsets, rows, row_weight, pos, perm)."""
    d = env.dev
    T, k = ids.shape
    P = T * k
    sizes = dict(offsets=E + 1, perm=P, rows=P, row_weight=P, pos=P)
    bufs = {n: canary_padded(s, F32 if n == "row_weight" else I32, d) for n, s in sizes.items()}
    ptr = lambda n: bufs[n][1].data_ptr() if sizes[n] else None
    with torch.cuda.device(d):
        rc = env.lib.flute_moe_route(
            ID_CODE[ids.dtype], 0 if weights is None else WEIGHT_CODE[weights.dtype], T, k, E, ids.data_ptr() or None,
            None if weights is None else weights.data_ptr(), bufs["offsets"][1].data_ptr(), ptr("perm"), ptr("rows"),
            None if weights is None else ptr("row_weight"), ptr("pos"), torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for n, s in sizes.items():
        assert intact(bufs[n][0], s), "canary around " + n
    if weights is None:
        assert bool(torch.all(bufs["row_weight"][0] == CANARY)), "row_weight written without weights"
    out = {n: bufs[n][1] for n in sizes}
    return out["offsets"], out["rows"], None if weights is None else out["row_weight"], out["pos"].view(T, k), out["perm"]


def check_route(env, ids_host, E, widths=(I32, I64), weight_dtypes=(F16, BF16, F32, None)):
    """ids_host [T, k] int64 on the host.  Every output of the direct call and of flute_amd.moe_route against the host loop
    and sort_by_expert."""
    d = env.dev
    T, k = ids_host.shape
    P = T * k
    want_off, want_perm, want_rows, want_pos = host_route(ids_host.reshape(-1).tolist(), k, E)
    w_host = torch.randn(T, k, generator=torch.Generator().manual_seed(P + E))
    for width in widths:
        if width == I32 and (int(ids_host.abs().max()) if P else 0) >= 2 ** 31:
            continue
        ids = ids_host.to(width).to(d)
        if P and E:
            sperm, soff = env.moe.sort_by_expert(ids, E)
            assert soff.tolist() == want_off and sperm.tolist() == want_perm, "the host loop is sort_by_expert's grouping"
        for wd in weight_dtypes:
            weights = None if wd is None else w_host.to(wd).to(d)
            for got in (route_abi(env, ids, weights, E), env.fa.moe_route(ids, weights, E)):
                offsets, rows, row_weight, pos, perm = got
                what = (T, k, E, width, wd)
                assert [t.dtype for t in (offsets, rows, pos, perm)] == [I32] * 4
                assert offsets.shape == (E + 1,) and rows.shape == (P,) and perm.shape == (P,) and pos.shape == (T, k)
                assert offsets.tolist() == want_off, what
                assert perm.tolist() == want_perm, what
                assert rows.tolist() == want_rows, what
                assert pos.reshape(-1).tolist() == want_pos, what
                assert torch.equal(rows, perm // k) if k else True
                assert torch.equal(pos.reshape(-1)[perm.long()], torch.arange(P, device=d, dtype=I32))
                if wd is None:
                    assert row_weight is None
                else:
                    assert row_weight.dtype == F32 and row_weight.shape == (P,)
                    expect = weights.flatten()[perm.long()].float()
                    assert torch.equal(row_weight.view(I32), expect.view(I32)), what


def draw_ids(T, k, E, seed, choices=None):
    gen = torch.Generator().manual_seed(seed)
    if choices is None:
        return torch.randint(0, E, (T, k), generator=gen)
    return torch.tensor(choices)[torch.randint(0, len(choices), (T, k), generator=gen)]


ROUTE_CASES = [
    (1, 1, 1, None),                 # the smallest case
    (1, 2, 8, None),                 # one token, two slots
    (37, 2, 4, [0, 1, 3]),           # expert 2 is never chosen
    (5, 8, 64, None),                # P < 64
    (33, 3, 3, None),                # P not a multiple of 64, E not a power of two
    (261, 8, 256, None),             # P = 2088 > 2 * 1024: every wave walks its range more than once
    (40, 4, 1024, None),             # the cap on E
]


@pytest.mark.parametrize("T,k,E,choices", ROUTE_CASES)
def test_route_against_host_loop(env, T, k, E, choices):
    ids = draw_ids(T, k, E, 1000 + T + E, choices)
    if E == 1024:
        ids[0, 0], ids[-1, -1] = E - 1, 0
    if choices is not None:
        assert 2 not in ids
    check_route(env, ids, E)


def test_route_all_pairs_to_the_last_expert(env):
    check_route(env, torch.full((70, 3), 6), 7, weight_dtypes=(F16, None))
    check_route(env, torch.full((261, 8), 255), 256, weight_dtypes=(None,))


def test_route_ids_outside_sort_last_in_order(env):
    E = 5
    ids = draw_ids(45, 4, E, 77)
    ids[0, 1], ids[3, 0], ids[3, 3], ids[17, 2], ids[44, 3], ids[44, 0] = -1, E, -1, E + 100, E, -7
    check_route(env, ids, E, weight_dtypes=(BF16, None))
    wide = ids.clone()
    wide[1, 1], wide[9, 0], wide[30, 2], wide[30, 3] = 2 ** 32 + 1, -2 ** 32, 2 ** 32, 2 ** 40 + 3
    off, _, _, _, perm = route_abi(env, wide.to(env.dev), None, E)
    tail = perm[int(off[E]):].tolist()
    assert tail == sorted(tail) and {1 * 4 + 1, 9 * 4, 30 * 4 + 2, 30 * 4 + 3} <= set(tail)      # 2^32 + 1 is outside, not expert 1
    check_route(env, wide, E, widths=(I64,), weight_dtypes=(F32,))
    # nobody served: every pair is outside
    check_route(env, torch.full((9, 2), -1), 4, weight_dtypes=(None,))


def test_route_no_pairs_still_writes_offsets(env):
    for T, k in ((0, 2), (3, 0)):
        check_route(env, torch.zeros(T, k, dtype=I64), 6, weight_dtypes=(F16, None))
    check_route(env, draw_ids(4, 2, 1, 5), 0, weight_dtypes=(None,))            # no expert at all: everything is outside


# ---- combine -------------------------------------------------------------------------------------------------------------

def combine_reference(Y, pos, offsets):
    """The contract restated in torch ops: fp32, slot order, a skipped slot adds +0, one rounding."""
    P, N = Y.shape
    T, k = pos.shape
    served = int(offsets[-1].clamp(0, P))
    acc = torch.zeros(T, N, dtype=F32, device=Y.device)
    zero = torch.zeros((), dtype=F32, device=Y.device)
    for j in range(k):
        p = pos[:, j].long()
        valid = (p >= 0) & (p < served)
        y = Y[p.clamp(0, max(P - 1, 0))].float() if P else acc
        acc = acc + torch.where(valid[:, None], y, zero)
    return acc.to(Y.dtype)


def combine_abi(env, Y, pos, offsets):
    """The direct call with `out` in the middle of a larger buffer."""
    d = env.dev
    T, k = pos.shape
    N = Y.shape[1]
    canary = XC.NAN_BITS[Y.dtype]
    buf = torch.full((GUARD + T * N + GUARD,), canary, dtype=torch.int16, device=d)
    with torch.cuda.device(d):
        rc = env.lib.flute_moe_combine(
            0 if Y.dtype == F16 else 1, T, k, offsets.shape[0] - 1, N, Y.data_ptr() or None, pos.data_ptr() or None,
            offsets.data_ptr(), buf[GUARD:].data_ptr(), torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.all(buf[:GUARD] == canary)) and bool(torch.all(buf[GUARD + T * N:] == canary)), "canary around out"
    return buf[GUARD:GUARD + T * N].view(T, N)


def combine_case(dev, dtype, T, k, N, seed, E=6):
    """Y [T k, N] of mixed magnitudes and signs, pos a permutation as moe_route writes it, offsets with offsets[E] = P."""
    gen = torch.Generator().manual_seed(seed)
    P = T * k
    Y = (torch.randn(P, N, generator=gen) * 2.0 ** torch.randint(-6, 7, (P, N), generator=gen)).to(dtype)
    pos = torch.randperm(P, generator=gen).to(I32).reshape(T, k)
    offsets = torch.zeros(E + 1, dtype=I32)
    offsets[E] = P
    return Y.to(dev), pos.to(dev), offsets.to(dev)


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_combine_bit_for_bit(env, dtype, k):
    for T in (1, 37):
        for N in (8, 256, 4096 + 8):
            Y, pos, offsets = combine_case(env.dev, dtype, T, k, N, 31 * T + N + k)
            P = T * k
            nan = torch.full((N,), float("nan"), dtype=dtype, device=env.dev)
            for served in sorted({P, P - (P + 2) // 3, 0, P + 5, -3}):
                offsets[-1] = served
                Yn = Y.clone()
                Yn[max(0, min(served, P)):] = nan                   # rows no expert served: whatever they hold must not reach out
                want = combine_reference(Yn, pos, offsets)
                assert bool(torch.isfinite(want).all())
                for out in (combine_abi(env, Yn, pos, offsets), bits16(env.fa.moe_combine(Yn, pos, offsets))):
                    assert torch.equal(out, bits16(want)), (dtype, k, T, N, served)
                if min(served, P) <= 0:
                    assert bool(torch.all(want == 0))
            if T > 1:
                # positions outside [0, P) are skipped, whatever offsets[E] says
                offsets[-1] = P
                bad = pos.clone()
                bad[0, 0], bad[5, k - 1], bad[T - 1, 0] = -1, P, 2 ** 31 - 1
                bad[7] = -5
                want = combine_reference(Y, bad, offsets)
                assert torch.equal(combine_abi(env, Y, bad, offsets), bits16(want)), (dtype, k, T, N, "positions")
                assert bool(torch.all(want[7] == 0))


def test_combine_without_slots_is_zero(env):
    d = env.dev
    out = env.fa.moe_combine(torch.empty(0, 64, dtype=F16, device=d), torch.empty(5, 0, dtype=I32, device=d),
                             torch.zeros(3, dtype=I32, device=d))
    assert out.shape == (5, 64) and bool(torch.all(bits16(out) == 0))
    empty = env.fa.moe_combine(torch.empty(0, 64, dtype=BF16, device=d), torch.empty(0, 2, dtype=I32, device=d),
                               torch.zeros(3, dtype=I32, device=d))
    assert empty.shape == (0, 64)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_combine_accuracy_top8(env, dtype):
    T, k, N = 37, 8, 256
    Y, pos, offsets = combine_case(env.dev, dtype, T, k, N, 4242)
    terms = Y.cpu().double()[pos.cpu().long()]                      # [T, k, N]
    S, A = terms.sum(1), terms.abs().sum(1)
    share = float((S.abs() >= A / 4).double().mean())
    assert share >= 0.5, ("half the sums at least a quarter of sum |y_j|: the bound is not vacuous", share)
    out = env.fa.moe_combine(Y, pos, offsets).cpu().double()
    err = (out - S).abs()
    bound = XC.U_T[dtype] * S.abs() + (k - 1) * 2.0 ** -24 * A + ETA[dtype]
    worst = float((err / bound).max())
    print("combine %s top-8: max |out - S| / bound = %.4f, share = %.2f" % (dtype, worst, share))
    assert bool(torch.isfinite(out).all()) and bool((err <= bound).all()), worst


# ---- the module ----------------------------------------------------------------------------------------------------------

def reference_forward(env, c, experts, hidden, ids, weights, fused):
    """The same launches driven by sort_by_expert's own perm / offsets, combined by the torch restatement."""
    E, k = c["E"], ids.shape[1]
    gate, up, down = experts.gate, experts.up, experts.down
    perm, offsets = env.moe.sort_by_expert(ids, E)
    token = perm // k
    if fused:
        a = (c["bits"], c["g"], c["tid"], env.num_sms)
        h = env.fa.qgemm_grouped_glu(hidden, offsets, gate.weight, gate.scales, gate.tables2, up.weight, up.scales,
                                     up.tables2, *a, rows=token.to(I32))
        y = env.fa.qgemm_grouped_weighted(h, offsets, down.weight, down.scales, down.tables2,
                                          weights.reshape(-1)[perm].float(), *a)
    else:
        x = hidden[token]
        h = torch.nn.functional.silu(gate(x, offsets)) * up(x, offsets)
        y = down(h, offsets) * weights.reshape(-1)[perm].to(hidden.dtype)[:, None]
    pos = torch.empty(perm.shape[0], dtype=I32, device=perm.device)
    pos[perm] = torch.arange(perm.shape[0], dtype=I32, device=perm.device)
    return combine_reference(y, pos.reshape(ids.shape), offsets)


@pytest.fixture(scope="module")
def native_fused(env, experts_case):
    return native(env, experts_case, True)


@pytest.mark.parametrize("fused", [True, False])
def test_native_top2_equals_the_launches_on_sort_by_expert(env, experts_case, native_fused, fused):
    c = experts_case
    experts = native_fused if fused else native(env, c, False)
    assert experts.native_routing is True and experts.fused is fused
    for ids in (c["ids"], c["ids2"], c["ids"].to(I32)):
        Y = experts(c["hidden"], ids, c["weights"])
        assert Y.shape == (c["T"], c["K"]) and Y.dtype == c["dtype"]
        want = reference_forward(env, c, experts, c["hidden"], ids, c["weights"], fused)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        assert torch.equal(bits16(Y), bits16(want)), fused


@pytest.mark.parametrize("fused", [True, False])
def test_native_top3_against_loop_and_fp64(env, top3_case, fused):
    """R and Y_loop as tests/test_grouped_gpu.py::test_flute_experts_against_loop_and_fp64 computes them (the loop's sum
    over a token's experts taken on the host side in expert order): max|Y - R| <= 2 max|Y_loop - R|; two calls, equal bits."""
    c = top3_case
    d, dtype, E, K, T, bits, g, tid = env.dev, c["dtype"], c["E"], c["K"], c["T"], c["bits"], c["g"], c["tid"]
    gates, ups, downs, hidden, ids, weights = c["gates"], c["ups"], c["downs"], c["hidden"], c["ids"], c["weights"]
    assert ids.shape == (T, 3) and all(len(set(r)) == 3 for r in ids.tolist())
    experts = native(env, c, fused)
    Y = experts(hidden, ids, weights)
    assert Y.shape == (T, K) and Y.dtype == dtype
    assert torch.equal(bits16(Y), bits16(experts(hidden, ids, weights)))
    assert torch.equal(bits16(Y), bits16(reference_forward(env, c, experts, hidden, ids, weights, fused)))

    deq = lambda m: env.fa.dequantize(m.weight, m.scales, m.tables2, bits, g, tid)
    silu = torch.nn.functional.silu
    R = torch.zeros(T, K, dtype=torch.float64, device=d)
    Y_loop = torch.zeros(T, K, dtype=dtype, device=d)
    for e in range(E):
        tok, slot = (ids == e).nonzero(as_tuple=True)
        x = hidden[tok]
        wgt = weights[tok, slot]
        xd = x.double()
        h = silu(xd @ deq(gates[e]).double().T) * (xd @ deq(ups[e]).double().T)
        R.index_add_(0, tok, (h @ deq(downs[e]).double().T) * wgt.double()[:, None])
        hl = silu(gates[e](x)) * ups[e](x)
        Y_loop.index_add_(0, tok, downs[e](hl) * wgt[:, None])        # a token appears once per expert: no race
    err = float((Y.double() - R).abs().max())
    err_loop = float((Y_loop.double() - R).abs().max())
    print("FluteExperts(native_routing=True, fused=%s) top-3: max|Y - R| = %.3e, loop max|Y_loop - R| = %.3e, max|R| = %.3e"
          % (fused, err, err_loop, float(R.abs().max())))
    assert err_loop > 0
    assert err <= 2 * err_loop, (err, err_loop)


def test_native_forward_in_a_graph(env, experts_case, native_fused):
    """moe_route, the two fused launches and moe_combine captured once (capture raises if anything reads the routing on
    the host); after topk_ids, the routing weights and the hidden states were overwritten in place a replay returns the
    bits of an eager call on the new routing."""
    c, experts = experts_case, native_fused
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


@pytest.mark.parametrize("fused", [True, False])
def test_native_ids_outside_contribute_nothing(env, experts_case, native_fused, fused):
    c = experts_case
    experts = native_fused if fused else native(env, c, False)
    hidden, ids, weights = c["hidden"], c["ids2"], c["weights"]
    base = experts(hidden, ids, weights)
    ids3 = ids.clone()
    ids3[0] = torch.tensor([c["E"], -1], device=ids3.device)
    out = experts(hidden, ids3, weights)
    assert bool(torch.all(out[0] == 0)) and bool(torch.isfinite(out).all())
    assert torch.equal(bits16(out[1:]), bits16(base[1:]))
    assert float(base[0].abs().max()) > 0


@pytest.mark.parametrize("fused", [True, False])
def test_default_path_keeps_its_bits(env, experts_case, fused):
    """native_routing=False is the forward FluteExperts had before the argument existed."""
    c = experts_case
    plain = env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused)
    off = env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused, native_routing=False)
    assert plain.native_routing is False and off.native_routing is False
    a = off(c["hidden"], c["ids"], c["weights"])
    b = plain(c["hidden"], c["ids"], c["weights"])
    assert torch.equal(bits16(a), bits16(b))
