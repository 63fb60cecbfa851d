"""flute_amd.qgemm_grouped_table_grad / flute_qgemm_grouped_table_grad on the GPU, and the training of the experts'
lookup tables built on it: dT2[e] = the dense table gradient of expert e over the rows a device-side table gives it, one
main launch and one reduce launch.

Kernel level, on the gradient tests' case matrix (grouped_cases.matrix): every non-empty expert's slice is bit for bit
`qgemm_table_grad` on its rows (the dense launch never splits M at these counts), empty experts are zeros, NaN rows past
offsets[E] stay out, the fused scale gradient is `qgemm_grouped_scale_grad`'s; the row weight is bit for bit a
pre-multiplied dY; random data stays within the componentwise bound of the documented chain depth; exact layers equal
the fp64 sums; a direct ABI call writes exactly dT2 and dS, also on malformed tables; calls and graph replays give equal
bits; a NaN stays in the bins of its expert that the formula names.  On top: the three codebook entry points return the
public ops' bits and the stated compositions, `FluteExperts` / `FluteSparseMoeBlock` give the codebooks the gradient of
fp64 autograd as closely as a per-expert loop of dense learnable layers does, and a dozen Adam steps on scales and
codebooks learn a teacher."""
import pytest
import torch

from tests import exact_cases as XC
from tests import scale_grad_ref as SR
from tests import table_grad_ref as TR
from tests.grouped_cases import (BF16, F16, GRAD_COUNTS, HALF_SUB, MIN_NORMAL, PAD, exact_inputs, exact_layers,  # noqa: F401
                                 exact_premise, exact_scales, exact_seed, gate_formula, matrix, nan_padded, restated_experts,
                                 stack_exact, tiny)
from tests.support import bits16, bits32, env, first_template, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu


def random_case_of(env, bits, tile_p, g, dtype, pair, K, N):
    """A random stack (codes, random scales as the random_layer of test_table_grad_gpu.py draws them, an NF-style table
    or a pair codebook per expert), random dY and X with NaN rows past offsets[E], a row weight, and the launches every
    test of the case reads - computed once."""
    key = ("table_grad", bits, tile_p, g, dtype, pair, K, N)
    if key not in env.cache:
        d, E, Rs, n = env.dev, len(GRAD_COUNTS), sum(GRAD_COUNTS), 2 ** bits
        assert max(GRAD_COUNTS) <= 224                                    # the dense launch splits M from 8 steps of 32 rows on
        tid = first_template(bits, tile_p)
        gen = torch.Generator().manual_seed(exact_seed(bits, tile_p, g) + 11)
        W = torch.randint(0, n, (E, K, N), generator=gen, dtype=torch.uint8).to(d)
        S = (torch.randn(E, N, K // g, generator=gen) / 8).to(dtype).to(d)
        if pair:
            t2 = torch.randn(E, n, n, 2, generator=gen).to(dtype).contiguous().view(torch.float32)
        else:
            t2 = torch.stack([env.O.make_qmap2_from_qmap(torch.randn(n, generator=gen).sort().values.to(dtype))
                              for _ in range(E)])
        Q = torch.stack([env.utils.pack(W[e], bits, [tid], env.num_sms) for e in range(E)])
        dY = nan_padded(torch.randn(Rs, N, generator=gen).to(dtype)).to(d)
        X = nan_padded(torch.randn(Rs, K, generator=gen).to(dtype)).to(d)
        rw = torch.cat([torch.rand(Rs, generator=gen) * 1.5 + 0.25, torch.full((PAD,), float("nan"))]).to(d)
        c = dict(W=W, Q=Q, S=S, t2=t2.to(d), dY=dY, X=X, rw=rw, off=offsets_of(GRAD_COUNTS, d), tid=tid, R=Rs + PAD,
                 bits=bits, g=g, dtype=dtype, K=K, N=N)
        f = env.fa.qgemm_grouped_table_grad
        c["dT"] = f(dY, X, c["off"], Q, S, bits, g, tid)
        c["dTw"] = f(dY, X, c["off"], Q, S, bits, g, tid, row_weight=rw)
        c["both"] = f(dY, X, c["off"], Q, S, bits, g, tid, table2=c["t2"], with_scale_grad=True)
        c["bothw"] = f(dY, X, c["off"], Q, S, bits, g, tid, table2=c["t2"], with_scale_grad=True, row_weight=rw)
        env.cache[key] = c
    return env.cache[key]


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_bit_equal_with_dense_op(env, bits, tile_p, g, dtype, pair, K, N):
    c = random_case_of(env, bits, tile_p, g, dtype, pair, K, N)
    n, E = 2 ** bits, len(GRAD_COUNTS)
    dT = c["dT"]
    assert dT.shape == (E, n, n, 2) and dT.dtype == torch.float32
    assert torch.isfinite(dT).all()                                  # the NaN rows past offsets[E] were not read
    off = offsets_of(GRAD_COUNTS).tolist()
    for e, m in enumerate(GRAD_COUNTS):
        if m == 0:
            assert torch.all(bits32(dT[e]) == 0), e
            continue
        r0, r1 = off[e], off[e + 1]
        dense = env.fa.qgemm_table_grad(c["dY"][r0:r1], c["X"][r0:r1], c["Q"][e], c["S"][e], bits, g, c["tid"])
        assert torch.equal(bits32(dT[e]), bits32(dense)), (e, m)
        assert float(dense.abs().max()) > 0
    # the fused launch: the same dT2, and dS bit for bit the grouped scale gradient's, with and without a row weight
    for (t, s), alone, kw in ((c["both"], dT, {}), (c["bothw"], c["dTw"], dict(row_weight=c["rw"]))):
        assert torch.equal(bits32(t), bits32(alone))
        want = env.fa.qgemm_grouped_scale_grad(c["dY"], c["X"], c["off"], c["Q"], c["t2"], bits, g, c["tid"], **kw)
        assert s.shape == (E, N, K // g) and s.dtype == dtype and torch.isfinite(s).all()
        assert torch.equal(bits16(s), bits16(want))


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_row_weight_is_a_premultiplied_grad_output(env, bits, tile_p, g, dtype, pair, K, N):
    """round_T(row_weight[r] * dY[r, n]) with the product in fp32, formed by the kernel, against the same rounding by torch."""
    c = random_case_of(env, bits, tile_p, g, dtype, pair, K, N)
    pre = (c["dY"].float() * c["rw"][:, None]).to(dtype)
    ref = env.fa.qgemm_grouped_table_grad(pre, c["X"], c["off"], c["Q"], c["S"], bits, g, c["tid"])
    assert torch.isfinite(c["dTw"]).all()
    assert torch.equal(bits32(c["dTw"]), bits32(ref))
    assert not torch.equal(bits32(c["dTw"]), bits32(c["dT"]))


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_random_within_componentwise_bound(env, bits, tile_p, g, dtype, pair, K, N):
    """Per expert and bin |dT2 - R| <= gamma(d) A, d = table_grad_ref.chain_depth(M_e) with M_e the expert's rows (the new
    file's header restates the derivation), A the same sum over absolute values.  With a row weight the operand dYw is
    itself rounded once to T before the chain: (u + gamma) A (1 + u), A and R taken with the unrounded fp64 product
    row_weight dY.  That models the rounding as x (1 + d), |d| <= u, which holds down to T's smallest normal only; below
    it the error is absolute, at most HALF_SUB, so exactly there the underflow term is written out:
    + (1 + gamma) HALF_SUB B, B = the bin's sum of |X| |S| over those (r, n) only whose |row_weight[r] dY[r, n]| is below
    MIN_NORMAL (in bf16 there are none).  The result is fp32 and of order one: it has no rounding or underflow term."""
    c = random_case_of(env, bits, tile_p, g, dtype, pair, K, N)
    u, sub, tiny_ = XC.U_T[dtype], HALF_SUB[dtype], MIN_NORMAL[dtype]
    off = offsets_of(GRAD_COUNTS).tolist()
    worst = 0.0
    for e, m in enumerate(GRAD_COUNTS):
        if m == 0:
            continue
        r0, r1 = off[e], off[e + 1]
        dY, X, W, S = c["dY"][r0:r1], c["X"][r0:r1], c["W"][e], c["S"][e]
        gam = XC.gamma(TR.chain_depth(m))
        R, A = TR.table_grad(dY, X, W, S, bits, g), TR.table_grad(dY, X, W, S, bits, g, absolute=True)
        err = (c["dT"][e].double().reshape(-1, 2) - R).abs()
        bound = gam * A
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert torch.all(err <= bound), (e, float((err - bound).max()))
        dYw = dY.double() * c["rw"][r0:r1].double()[:, None]
        R, A = TR.table_grad(dYw, X, W, S, bits, g), TR.table_grad(dYw, X, W, S, bits, g, absolute=True)
        B = TR.table_grad((dYw.abs() < tiny_).double(), X, W, S, bits, g, absolute=True)
        bound = (u + gam) * A * (1 + u) + (1 + gam) * sub * B
        err = (c["dTw"][e].double().reshape(-1, 2) - R).abs()
        assert torch.all(err <= bound), ("weighted", e, float((err - bound).max()))
    print("grouped table grad", (bits, tile_p, g), "max err / bound", worst)


@pytest.mark.parametrize("bits,tile_p,g,dtype,pair,K,N", matrix())
def test_exact_layers(env, bits, tile_p, g, dtype, pair, K, N):
    """X and dY multiples of 1/4, scales +-2^e, exact tables: every term is a multiple of 2^-5 and every bin's sum of |terms|
    stays below 2^24 quanta (grouped_cases.exact_premise asserts it), so every partial sum in any order is exact in
    fp32 and the fp64 sum is the only allowed answer - for dT2 by value, for the fused dS after its one rounding."""
    d, E = env.dev, len(GRAD_COUNTS)
    layers = exact_layers(bits, tile_p, g, dtype, K, N, pair, E, exact_seed(bits, tile_p, g) + 700)
    Q, _, t2, tid = stack_exact(env, layers)
    S = torch.stack([exact_scales(N, K // g, dtype, seed=701 + g + e) for e in range(E)]).to(d)
    parts = [exact_inputs(m, K, N, dtype, seed=702 + g + e) for e, m in enumerate(GRAD_COUNTS)]
    X, dY = (nan_padded(torch.cat([p[i] for p in parts])).to(d) for i in range(2))
    dT, dS = env.fa.qgemm_grouped_table_grad(dY, X, offsets_of(GRAD_COUNTS, d), Q, S, bits, g, tid, table2=t2,
                                             with_scale_grad=True)
    off = offsets_of(GRAD_COUNTS).tolist()
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            assert torch.all(bits32(dT[e]) == 0) and torch.all(bits16(dS[e]) == 0), e
            continue
        codes = lay.W.to(d)
        L = SR.lut_of_codes(codes, lay.pairs, bits)
        R, Rs = exact_premise(X[r0:r1], dY[r0:r1], S[e], codes, L, bits, g, dtype)
        got = dT[e].double().reshape(-1, 2)
        assert torch.equal(got, R), (e, float((got - R).abs().max()))
        assert XC.exact_equal(dS[e], Rs, dtype), e
        assert float(R.abs().max()) > 0


@pytest.fixture(scope="module")
def small(env):
    """One random 4-bit case shared by the ABI and NaN tests."""
    return random_case_of(env, 4, 32, 64, F16, False, 320, 256)


def test_direct_abi_writes_exactly_dT2_and_dS(env, small):
    """dT2 and dS each in the middle of a canary-filled buffer, the scratch prefilled with NaN bits: exactly dT2 and dS
    are written, finite, the wrapper's bits.  Malformed tables (negative entries, entries above R, a decreasing pair) give
    the clamped table's result with the guards intact."""
    c = small
    d, dtype, K, N, g, bits, E = env.dev, c["dtype"], c["K"], c["N"], c["g"], c["bits"], len(GRAD_COUNTS)
    G, nb = K // g, 2 * 4 ** bits
    guard, n_t, n_s = 4096, E * nb, E * N * G
    nan32, nan16 = 0x7FC00000, XC.NAN_BITS[dtype]
    nbytes = env.lib.flute_qgemm_grouped_table_grad_scratch_bytes(bits, g, E, N, K)
    assert nbytes == E * (N // 128) * -(-K // 256) * nb * 4
    tbuf = torch.empty(guard + n_t + guard, dtype=torch.int32, device=d)
    sbuf = torch.empty(guard + n_s + guard, dtype=torch.int16, device=d)
    scratch = torch.empty(nbytes // 4 + guard, dtype=torch.int32, device=d)
    full = offsets_of(GRAD_COUNTS)

    def run(off, with_ds=True, row_weight=None, R=None, E_=None, scratch_bytes=nbytes):
        tbuf.fill_(nan32), sbuf.fill_(nan16), scratch.fill_(nan32)
        off = off.to(d)
        with torch.cuda.device(d):
            rc = env.lib.flute_qgemm_grouped_table_grad(
                0 if dtype == F16 else 1, bits, g, E if E_ is None else E_, c["R"] if R is None else R, N, K,
                c["Q"].shape[1], c["tid"], c["dY"].data_ptr(), c["X"].data_ptr(), off.data_ptr(), c["Q"].data_ptr(),
                c["S"].data_ptr(), c["t2"].data_ptr() if with_ds else None,
                None if row_weight is None else row_weight.data_ptr(), tbuf[guard:].data_ptr(),
                sbuf[guard:].data_ptr() if with_ds else None, scratch.data_ptr(), scratch_bytes, env.num_sms,
                torch.cuda.current_stream(d).cuda_stream)
        torch.cuda.synchronize()
        assert torch.all(tbuf[:guard] == nan32) and torch.all(tbuf[guard + n_t:] == nan32)
        assert torch.all(sbuf[:guard] == nan16) and torch.all(sbuf[guard + n_s:] == nan16)
        assert torch.all(scratch[nbytes // 4:] == nan32)            # the scratch is used up to the queried size at most
        return rc, tbuf[guard:guard + n_t].clone().view(torch.float32).view(E, -1), \
            sbuf[guard:guard + n_s].clone().view(dtype).view(E, N, G)

    def check(off, **kw):
        """The result for `off` - with R the ABI's row count, the case's by default - against the wrapper's on the clamped,
        well-formed table of the same ranges: per expert its rows [clamp(off[e]), clamp(off[e + 1])) alone, or zeros."""
        rc, t, s = run(off, **kw)
        assert rc == 0 and torch.isfinite(t).all() and torch.isfinite(s).all()
        R = c["R"] if kw.get("R") is None else kw["R"]
        lo, hi = off[:-1].clamp(0, R), off[1:].clamp(0, R)
        args = (c["Q"], c["S"], bits, g, c["tid"])
        for e in range(E):
            r0, r1 = int(lo[e]), int(hi[e])
            if r1 <= r0:
                assert torch.all(bits32(t[e]) == 0), (off.tolist(), e)
                if kw.get("with_ds", True):
                    assert torch.all(bits16(s[e]) == 0), (off.tolist(), e)
                continue
            one = offsets_of([0] * e + [r1 - r0] + [0] * (E - 1 - e), d)      # expert e alone over its clamped rows
            wt, ws = env.fa.qgemm_grouped_table_grad(c["dY"][r0:r1], c["X"][r0:r1], one, *args, table2=c["t2"],
                                                     with_scale_grad=True)
            assert torch.equal(bits32(t[e]), bits32(wt[e].reshape(-1))), (off.tolist(), e)
            if kw.get("with_ds", True):
                assert torch.equal(bits16(s[e]), bits16(ws[e])), (off.tolist(), e)
        return t, s

    t, s = check(full)
    assert torch.equal(bits32(t), bits32(c["both"][0].view(E, -1))) and torch.equal(bits16(s), bits16(c["both"][1]))
    rc, t, s = run(full, row_weight=c["rw"])
    assert rc == 0
    assert torch.equal(bits32(t), bits32(c["bothw"][0].view(E, -1))) and torch.equal(bits16(s), bits16(c["bothw"][1]))
    rc, t, s = run(full, with_ds=False)                             # table only: dS stays untouched
    assert rc == 0 and torch.equal(bits32(t), bits32(c["dT"].view(E, -1))) and torch.all(bits16(s) == nan16)
    Rs = sum(GRAD_COUNTS)
    check(full.clamp(max=2 * Rs // 3))                              # a proper table that ends early
    neg = full.clone()
    neg[:3] = torch.tensor([-5, -1, -70])
    above = full.clone()
    above[-3:] = torch.tensor([c["R"] + 1, c["R"] + 1000, 2 ** 31 - 1])
    decreasing = full.clone()
    decreasing[3], decreasing[4] = full[4], full[3]
    for off in (neg, decreasing):
        check(off)
    # entries past R: with R = Rs - 10 every row below R is finite, so the clamp alone decides what experts 5 .. 7 return.
    # `full` itself is then a table that runs past R (expert 6 loses its last 5 rows, expert 7 all of them: zeros), and in
    # `past` expert 5's end is R + 1 (it gets the rows [97, R) expert 6 had) and experts 6 and 7 start at or past R: zeros
    Rc = Rs - 10
    assert full[6] < Rc < full[7] and GRAD_COUNTS[5] == 0
    past = full.clone()
    past[-3:] = torch.tensor([Rc + 1, Rc + 1000, 2 ** 31 - 1])
    for off in (full, past):
        t, s = check(off, R=Rc)
        assert torch.all(bits32(t[7]) == 0) and torch.all(bits16(s[7]) == 0)
    assert torch.all(bits32(t[6]) == 0) and torch.all(bits16(s[6]) == 0) and float(t[5].abs().max()) > 0
    neg_past = past.clone()
    neg_past[:3] = neg[:3]
    check(neg_past, R=Rc)
    # (at the case's own R such entries reach into its NaN rows past offsets[E]: memory-safe, and the experts below keep their bits)
    rc, t, s = run(above)
    good = c["both"]
    assert rc == 0
    for e in (0, 1, 2, 3, 4):
        assert torch.equal(bits32(t[e]), bits32(good[0][e].reshape(-1))) and torch.equal(bits16(s[e]), bits16(good[1][e]))
    # R == 0 writes zeros; E == 0 writes nothing; one byte too few is refused and writes nothing
    rc, t, s = run(full, R=0)
    assert rc == 0 and torch.all(bits32(t) == 0) and torch.all(bits16(s) == 0)
    rc, t, s = run(full, E_=0)
    assert rc == 0 and torch.all(bits32(t) == nan32) and torch.all(bits16(s) == nan16)
    rc, t, s = run(full, scratch_bytes=nbytes - 1)
    assert rc == -5 and torch.all(bits32(t) == nan32) and torch.all(bits16(s) == nan16)


def test_equal_bits_over_calls_and_graph_replays(env):
    """A 2-bit case - 16 pair indices: most lanes of a wave meet on a bin - twice eagerly and 20 times from a captured
    graph: the same bits every time.  The host reads nothing: a replay after `offsets`, dY and X were overwritten in
    place serves the new contents, bit for bit what an eager call on them returns."""
    c = random_case_of(env, 2, 32, 64, F16, False, 320, 256)
    d, E = env.dev, len(GRAD_COUNTS)
    counts2 = [40, 0, 3, 0, 60, 33, 1, sum(GRAD_COUNTS) - 137]
    assert sum(counts2) == sum(GRAD_COUNTS) and len(counts2) == E and min(counts2) >= 0
    gen = torch.Generator().manual_seed(78)
    dY2 = nan_padded(torch.randn(sum(GRAD_COUNTS), c["N"], generator=gen).to(c["dtype"])).to(d)
    X2 = nan_padded(torch.randn(sum(GRAD_COUNTS), c["K"], generator=gen).to(c["dtype"])).to(d)
    off2 = offsets_of(counts2, d)
    dy, x, off = c["dY"].clone(), c["X"].clone(), c["off"].clone()
    run = lambda a, b, o: env.fa.qgemm_grouped_table_grad(a, b, o, c["Q"], c["S"], c["bits"], c["g"], c["tid"], env.num_sms,
                                                          table2=c["t2"], with_scale_grad=True, row_weight=c["rw"])
    same = lambda a, b: torch.equal(bits32(a[0]), bits32(b[0])) and torch.equal(bits16(a[1]), bits16(b[1]))
    first = run(dy, x, off)
    assert same(first, c["bothw"]) and same(run(dy, x, off), first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(dy, x, off)
    for _ in range(20):
        out[0].fill_(7.0), out[1].fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, first)
    off.copy_(off2), dy.copy_(dY2), x.copy_(X2)
    out[0].fill_(7.0), out[1].fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(dY2, X2, off2)
    assert same(out, eager)
    assert torch.isfinite(eager[0]).all() and not torch.equal(bits32(eager[0]), bits32(first[0]))
    assert torch.all(bits32(eager[0][1]) == 0) and torch.all(bits32(eager[0][3]) == 0)


def test_nan_stays_in_the_bins_the_formula_names(env, small):
    """A NaN in one X element of expert 6 (row 40 of its 97, column k = 261: the second, partial k block, the odd half
    of pair row 130): dT2[6] is NaN in exactly the bins (c, 1) whose pair index c occurs at pair row 130 of expert 6's
    codes, and every other bin of every expert - and every other expert's dS - keeps the clean run's bits."""
    c = small
    bits, g, E = c["bits"], c["g"], len(GRAD_COUNTS)
    e, k = 6, 261
    off = offsets_of(GRAD_COUNTS).tolist()
    X = c["X"].clone()
    X[off[e] + 40, k] = float("nan")
    dT, dS = env.fa.qgemm_grouped_table_grad(c["dY"], X, c["off"], c["Q"], c["S"], bits, g, c["tid"], table2=c["t2"],
                                             with_scale_grad=True)
    clean_t, clean_s = c["both"]
    named = torch.zeros(4 ** bits, 2, dtype=torch.bool, device=env.dev)
    named[TR.pair_index(c["W"][e], bits)[k >> 1].unique(), k & 1] = True
    assert 0 < int(named.sum()) < named.numel() // 2
    got = dT[e].reshape(-1, 2)
    assert torch.isnan(got[named]).all()
    assert torch.equal(bits32(got[~named]), bits32(clean_t[e].reshape(-1, 2)[~named]))
    others = [i for i in range(E) if i != e]
    assert torch.equal(bits32(dT[others]), bits32(clean_t[others]))
    assert torch.equal(bits16(dS[others]), bits16(clean_s[others]))
    hit = torch.zeros_like(dS[e], dtype=torch.bool)
    hit[:, k // g] = True                                            # dS: the group of k, every column
    assert torch.isnan(dS[e][hit]).all() and torch.equal(bits16(dS[e][~hit]), bits16(clean_s[e][~hit]))


# ---------------------------------------------------------------------------
# autograd, op level
# ---------------------------------------------------------------------------

def codebooks_of(env, form, E, bits, seed):
    """fp32 masters that need their rounding: [E, 2^b] or [E, 2^b, 2^b, 2]."""
    n = 2 ** bits
    gen = torch.Generator().manual_seed(seed)
    shape = (E, n) if form == "scalar" else (E, n, n, 2)
    return (torch.randn(shape, generator=gen) / 2 + 1e-3).to(env.dev)


def through_entry(env, c, form, table_form, scales_grad, codebook_grad):
    """One forward and backward through a codebook entry point on the `tiny` stacks: (out, dX, d row_weight or None,
    [dS_gate, dS_up], [dC_gate, dC_up], the built table2s)."""
    (Qg, Sg, _), (Qu, Su, _) = c["gate"], c["up"]
    bits = c["args"][0]
    cg, cu = codebooks_of(env, table_form, 3, bits, 61), codebooks_of(env, table_form, 3, bits, 62)
    built = [env.fa.ops._grouped_codebook_table2(t, bits, Sg.dtype) for t in (cg, cu)]
    if scales_grad:
        Sg, Su = torch.nn.Parameter(Sg.clone()), torch.nn.Parameter(Su.clone())
    if codebook_grad:
        cg, cu = torch.nn.Parameter(cg), torch.nn.Parameter(cu)
    rw = None
    if form == "plain":
        x = c["x_sorted"].clone().requires_grad_()
        y = env.ln.qgemm_grouped_learnable(x, c["off"], Qg, Sg, cg, *c["args"])
    elif form == "weighted":
        x, rw = c["x_sorted"].clone().requires_grad_(), c["rw"].clone().requires_grad_()
        y = env.ln.qgemm_grouped_weighted_learnable(x, c["off"], Qg, Sg, cg, rw, *c["args"])
    else:
        rows, pos = c["rows"] if "rows" in form else None, c["pos"] if "pos" in form else None
        x = (c["x_sorted"] if rows is None else c["tokens"]).clone().requires_grad_()
        y = env.ln.qgemm_grouped_glu_learnable(x, c["off"], Qg, Sg, cg, Qu, Su, cu, *c["args"], rows=rows, pos=pos)
    y.backward(c["dY"])
    return y.detach(), x.grad, None if rw is None else rw.grad, [Sg.grad, Su.grad], [cg.grad, cu.grad], built


@pytest.mark.parametrize("table_form", ["scalar", "pair"])
@pytest.mark.parametrize("form", ["plain", "weighted", "glu", "glu_rows", "glu_rows_pos"])
def test_codebook_entry_points(env, tiny, form, table_form):
    """The forward is the public op on the built table2; codebook.grad is the direct qgemm_grouped_table_grad call on the
    tensors the backward forms (folded per expert for the scalar form); scales.grad is ..._learnable_scales' when both
    train, and the codebook's gradient does not depend on whether the scales train."""
    c, fa, ln = tiny, env.fa, env.ln
    (Qg, Sg, _), (Qu, Su, _) = c["gate"], c["up"]
    args, off = c["args"], c["off"]
    y, dx, drw, dS, dC, (tg, tu) = through_entry(env, c, form, table_form, True, True)
    x, dY = c["x_sorted"], c["dY"]
    fold = fa.grouped_pair_grad_to_table_grad if table_form == "scalar" else (lambda t: t)
    # the public op and the scales-only entry point on the built tables
    Sg1, Su1 = torch.nn.Parameter(Sg.clone()), torch.nn.Parameter(Su.clone())
    if form == "plain":
        x0 = x.clone().requires_grad_()
        y0 = fa.qgemm_grouped(x0, off, Qg, Sg, tg, *args)
        ln.qgemm_grouped_learnable_scales(x, off, Qg, Sg1, tg, *args).backward(dY)
        want = [fa.qgemm_grouped_table_grad(dY, x, off, Qg, Sg, *args), None]
    elif form == "weighted":
        x0, rw0 = x.clone().requires_grad_(), c["rw"].clone().requires_grad_()      # (the op's backward path with d row_weight)
        y0 = fa.qgemm_grouped_weighted(x0, off, Qg, Sg, tg, rw0, *args)
        ln.qgemm_grouped_weighted_learnable_scales(x, off, Qg, Sg1, tg, c["rw"], *args).backward(dY)
        want = [fa.qgemm_grouped_table_grad(dY, x, off, Qg, Sg, *args, row_weight=c["rw"]), None]
    else:
        kw = dict(rows=c["rows"] if "rows" in form else None, pos=c["pos"] if "pos" in form else None)
        x0 = (x if kw["rows"] is None else c["tokens"]).clone().requires_grad_()
        y0 = fa.qgemm_grouped_glu(x0, off, Qg, Sg, tg, Qu, Su, tu, *args, **kw)
        ln.qgemm_grouped_glu_learnable_scales(x0.detach(), off, Qg, Sg1, tg, Qu, Su1, tu, *args, **kw).backward(dY)
        gt = fa.qgemm_grouped(x, off, Qg, Sg, tg, *args).float()
        ut = fa.qgemm_grouped(x, off, Qu, Su, tu, *args).float()
        sig = torch.sigmoid(gt)
        dg = (dY.float() * ut * sig * (1 + gt * (1 - sig))).to(x.dtype)
        du = (dY.float() * (gt * sig)).to(x.dtype)
        want = [fa.qgemm_grouped_table_grad(dg, x, off, Qg, Sg, *args), fa.qgemm_grouped_table_grad(du, x, off, Qu, Su, *args)]
    y0.backward(dY)
    assert torch.equal(bits16(y), bits16(y0.detach())) and torch.equal(bits16(dx), bits16(x0.grad))
    assert float(y.abs().max()) > 0 and (drw is not None) == (form == "weighted")
    if form == "weighted":
        assert torch.equal(bits32(drw), bits32(rw0.grad)) and float(drw.abs().max()) > 0
    for got, w, s_got, s_want in zip(dC, want, dS, (Sg1.grad, Su1.grad)):
        if w is None:
            assert got is None and s_got is None                     # (the up stack plays no part in this form)
            continue
        w = fold(w)
        assert got.dtype == torch.float32 and got.shape == w.shape and torch.equal(bits32(got), bits32(w))
        assert torch.isfinite(w).all() and float(w[0].abs().max()) > 0 and float(w[2].abs().max()) > 0
        assert not w[1].any()                                        # the empty expert: zeros
        assert torch.equal(bits16(s_got), bits16(s_want)) and float(s_want.abs().max()) > 0
    # the codebooks alone: the same gradient; nothing to train and grad mode off: the public op
    _, _, _, dS2, dC2, _ = through_entry(env, c, form, table_form, False, True)
    assert dS2 == [None, None]
    assert all((a is None and b is None) or torch.equal(bits32(a), bits32(b)) for a, b in zip(dC2, dC))
    with torch.no_grad():
        cg = codebooks_of(env, table_form, 3, args[0], 61).requires_grad_()
        y1 = ln.qgemm_grouped_learnable(x, off, Qg, Sg, cg, *args)
        served = int(off[-1])
        assert not y1.requires_grad
        assert torch.equal(bits16(y1[:served]), bits16(fa.qgemm_grouped(x, off, Qg, Sg, tg, *args)[:served]))


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------

NAMES = ("gate", "up", "down")


def make_experts_case(env, dtype):
    """The make_experts_case of test_grouped_scale_grad_gpu.py with the codes kept: E = 4 experts from
    FluteLinear.from_codes (4-bit, g = 64, K = 256, F = 512) with a table of their own each, 37 tokens; expert 2 is never
    chosen, token 0 is routed only to ids outside [0, E), token 5 has one such slot."""
    d = env.dev
    E, K, F, T, bits, g = 4, 256, 512, 37, 4, 64
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(43)
    nf4 = torch.tensor(env.O.NF4_VALUES)
    c = dict(E=E, K=K, F=F, T=T, bits=bits, g=g, tid=tid, dtype=dtype, codes=[[], [], []], layers=([], [], []))
    for which, (kk, nn) in enumerate(((K, F), (K, F), (F, K))):
        for e in range(E):
            codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
            scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
            table = (nf4 * (1 + torch.randn(16, generator=gen) / 16)).to(dtype).to(d)
            c["codes"][which].append(codes)
            c["layers"][which].append(env.FluteLinear.from_codes(codes, scales, table, bits, g, tid))
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["dOut"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["routing"] = {}
    for k in (2, 3):
        chosen = torch.tensor([0, 1, 3])
        ids = torch.stack([chosen[torch.randperm(3, generator=gen)[:k]] for _ in range(T)])
        ids[0] = torch.tensor([E, -1, E + 5][:k])
        ids[5, 1] = E
        weights = torch.rand(T, k, generator=gen)
        c["routing"][k] = (ids.to(d), (weights / weights.sum(1, keepdim=True)).to(dtype).to(d))
    c["refs"] = {}
    return c


@pytest.fixture(scope="module")
def experts_case(env):
    return make_experts_case(env, F16)


def codebook_leaves(c, table):
    """The three stacks' codebooks as fp64 leaves: [E, 16] from `tables`, or [E, 16, 16, 2] from `tables2`."""
    dtype = c["dtype"]
    if table == "scalar":
        return [torch.stack([m.tables for m in ms]).double().requires_grad_() for ms in c["layers"]]
    return [torch.stack([m.tables2.view(dtype).view(16, 16, 2) for m in ms]).double().requires_grad_() for ms in c["layers"]]


def dense_project(c, C64, table):
    """project(e, which, x) = x @ (pairs[idx] * S)^T in fp64, pairs from the codebook leaf of the stack `which`."""
    bits, g = c["bits"], c["g"]

    def project(e, which, x):
        leaf = C64[which][e]
        pairs = leaf.reshape(256, 2) if table == "pair" else \
            torch.stack([leaf[:, None].expand(16, 16), leaf[None, :].expand(16, 16)], -1).reshape(256, 2)
        codes = c["codes"][which][e]
        Lk = pairs[TR.pair_index(codes, bits)].permute(0, 2, 1).reshape(codes.shape)       # [K, N]
        S = c["layers"][which][e].scales.double()
        return x @ (Lk * S.repeat_interleave(g, dim=1).T)
    return project


def learnable_loop(env, c, table):
    """The yardstick's layers: every expert's FluteLinear as a dense LearnableFluteLinear in T."""
    return [[env.ln.LearnableFluteLinear(m, scales=True, table=table) for m in ms] for ms in c["layers"]]


def loop_grads(loop):
    return [torch.stack([m.codebook.grad if m.codebook.grad is not None else torch.zeros_like(m.codebook) for m in ms])
            for ms in loop]


def reference_codebook_grads(env, c, k, table):
    """(fp64 gradients, the yardstick's gradients) of the three stacks' codebooks for dOut, computed once per (k, form)."""
    if (k, table) not in c["refs"]:
        ids, weights = c["routing"][k]
        C64 = codebook_leaves(c, table)
        restated_experts(c, c["hidden"].double(), ids, weights.double(), dense_project(c, C64, table)) \
            .backward(c["dOut"].double())
        loop = learnable_loop(env, c, table)
        restated_experts(c, c["hidden"], ids, weights, lambda e, which, x: loop[which][e](x)).backward(c["dOut"])
        c["refs"][(k, table)] = ([t.grad for t in C64], loop_grads(loop))
    return c["refs"][(k, table)]


@pytest.mark.parametrize("table", ["scalar", "pair"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("fused,native", [(False, False), (True, False), (False, True), (True, True)])
def test_flute_experts_codebook_grads(env, experts_case, fused, native, k, table):
    """The three codebook.grad of a learnable FluteExperts in every configuration against fp64 autograd of the restated
    block on dense weights pairs[idx] * S with the codebook an fp64 leaf, max-abs error relative to max|ref|; the
    yardstick is the per-expert loop over dense LearnableFluteLinear in T and the bound twice its error (the operation
    orders differ, not the precision).  The figures are printed (-s) and tabulated in DESIGN.md 3.3k."""
    c = experts_case
    ids, weights = c["routing"][k]
    ref, yard = reference_codebook_grads(env, c, k, table)
    experts = env.moe.FluteExperts.from_linears(*c["layers"], fused=fused, native_routing=native)
    with torch.no_grad():
        frozen_out = experts(c["hidden"], ids, weights)
    params = env.moe.make_experts_learnable(experts, scales=True, table=table)
    assert len(params) == 6
    h, w = c["hidden"].clone().requires_grad_(), weights.clone().requires_grad_()
    out = experts(h, ids, w)
    if native or k == 2:                                           # (index_add_ at top-3: the order of a token's addends is free)
        assert torch.equal(bits16(out), bits16(frozen_out))        # the built tables are the stacks' own: the same forward
    out.backward(c["dOut"])
    assert h.grad is not None and w.grad is not None
    for name, p, s, r, y in zip(NAMES, params[1::2], params[0::2], ref, yard):
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32
        assert torch.isfinite(p.grad).all() and s.grad is not None
        err, yerr = max_rel_err(p.grad, r), max_rel_err(y, r)
        print("FluteExperts codebook.grad %s fused=%d native=%d k=%d %s: %.3e (yardstick %.3e)"
              % (table, fused, native, k, name, err, yerr))
        assert yerr > 0
        assert err <= 2 * yerr, (name, err, yerr)
        assert torch.all(p.grad[2] == 0) and torch.all(r[2] == 0)  # an expert no token chose


@pytest.mark.parametrize("table", ["scalar", "pair"])
def test_sparse_moe_block_codebook_grads(env, experts_case, table):
    """The same through FluteSparseMoeBlock with a group-limited sigmoid router (n_group = 2, topk_group = 1, renormalised,
    a bias, scale 2.5) on the fused, natively routed experts, the kernel's ids held fixed (the group keys are separated
    by more than 2^-8, asserted); the bound twice the error of the whole block restated in T over LearnableFluteLinear."""
    c = experts_case
    d, dtype, E, K, T = env.dev, c["dtype"], c["E"], c["K"], c["T"]
    k, n_group, topk_group, scoring, renorm, scale = 2, 2, 1, "sigmoid", True, 2.5
    gen = torch.Generator().manual_seed(53)
    bias = (torch.rand(E, generator=gen) * 0.2).to(d)
    for attempt in range(20):
        router = (torch.randn(E, K, generator=gen) * 0.08).to(dtype).to(d)
        logits = torch.nn.functional.linear(c["hidden"], router)
        keys = torch.sigmoid(logits.float()) + bias
        gkeys = keys.view(T, n_group, -1).max(dim=2).values.sort(dim=1, descending=True).values
        gap = gkeys[:, topk_group - 1] - gkeys[:, topk_group]
        if float(gap.min()) > 2.0 ** -8:
            break
    assert float(gap.min()) > 2.0 ** -8, float(gap.min())
    experts = env.moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
    block = env.moe.FluteSparseMoeBlock(router.clone(), experts, top_k=k, scoring=scoring, renormalize=renorm, bias=bias,
                                        scale=scale, n_group=n_group, topk_group=topk_group)
    with torch.no_grad():
        frozen_out = block(c["hidden"])
        ids, _ = env.fa.moe_gate_limited(logits, k, n_group, topk_group, scoring, renorm, bias, scale)
    params = env.moe.make_experts_learnable(block, scales=True, table=table)
    assert len(params) == 6
    out = block(c["hidden"])
    assert out.requires_grad and torch.equal(bits16(out), bits16(frozen_out))
    out.backward(c["dOut"])
    C64 = codebook_leaves(c, table)
    hd, rd = c["hidden"].double(), router.double()
    restated_experts(c, hd, ids, gate_formula(hd @ rd.T, ids, scoring, renorm, scale), dense_project(c, C64, table)) \
        .backward(c["dOut"].double())
    loop = learnable_loop(env, c, table)
    wT = gate_formula(torch.nn.functional.linear(c["hidden"], router).float(), ids, scoring, renorm, scale).to(dtype)
    restated_experts(c, c["hidden"], ids, wT, lambda e, which, x: loop[which][e](x)).backward(c["dOut"])
    for name, p, leaf, y in zip(NAMES, params[1::2], C64, loop_grads(loop)):
        err, yerr = max_rel_err(p.grad, leaf.grad), max_rel_err(y, leaf.grad)
        print("FluteSparseMoeBlock codebook.grad %s %s: %.3e (yardstick %.3e)" % (table, name, err, yerr))
        assert yerr > 0
        assert err <= 2 * yerr, (name, err, yerr)


def test_train_experts_scales_and_codebooks(env):
    """A dozen Adam steps on the scales and scalar codebooks of the tiny bf16 block toward a teacher with perturbed tables
    and scales: the loss falls below 0.8 of its start, the packed codes keep their bits, the codebooks moved, and the
    frozen block is plain GroupedFluteLinear stacks with the unchanged state-dict keys, whose tables / tables2 are the
    rounded codebooks and whose forward has the bits of the learnable forward under no_grad."""
    c = make_experts_case(env, BF16)
    dtype, moe = c["dtype"], env.moe
    torch.manual_seed(0)
    ids, weights = c["routing"][2]
    student = moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
    teacher = moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True)
    with torch.no_grad():
        for m in (teacher.gate, teacher.up, teacher.down):
            m.scales.copy_((m.scales.float() * (1 + torch.randn_like(m.scales.float()) / 8)).to(dtype))
            tables = (m.tables.float() * (1 + torch.randn_like(m.tables.float()) / 8)).to(dtype)
            m.tables.copy_(tables)
            m.tables2.copy_(torch.stack([env.utils.make_qmap2_from_qmap(t) for t in tables]))
        target = teacher(c["hidden"], ids, weights).float()
    keys = list(student.state_dict())
    weights0 = [m.weight.clone() for m in (student.gate, student.up, student.down)]
    tables0 = [m.tables.clone() for m in (student.gate, student.up, student.down)]
    params = moe.make_experts_learnable(student, scales=True, table="scalar")
    assert len(params) == 6 and [p.dtype for p in params] == [dtype, torch.float32] * 3
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = []
    for _ in range(12):
        loss = (student(c["hidden"], ids, weights).float() - target).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("expert scales + codebooks training: loss %.4e -> %.4e" % (losses[0], losses[-1]))
    assert losses[-1] < 0.8 * losses[0], losses
    stacks = (student.gate, student.up, student.down)
    assert all(torch.equal(m.weight, w) for m, w in zip(stacks, weights0))
    assert all(not torch.equal(m.codebook.detach().to(dtype), t) for m, t in zip(stacks, tables0))   # the codebooks moved
    learned = [(m.scales.detach().clone(), m.codebook.detach().clone()) for m in stacks]
    with torch.no_grad():
        learnable_out = student(c["hidden"], ids, weights)
    moe.freeze_experts(student)
    stacks = (student.gate, student.up, student.down)
    assert all(type(m) is moe.GroupedFluteLinear for m in stacks)
    assert list(student.state_dict()) == keys and not list(student.parameters())
    for m, (s, cb) in zip(stacks, learned):
        assert torch.equal(m.scales, s)
        assert torch.equal(m.tables, cb.to(dtype))
        assert torch.equal(m.tables2, torch.stack([env.utils.make_qmap2_from_qmap(t) for t in cb.to(dtype)]))
    out = student(c["hidden"], ids, weights)
    assert not out.requires_grad and torch.equal(bits16(out), bits16(learnable_out))
