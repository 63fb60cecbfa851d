"""flute_amd.qgemm_grouped_glu_blocks (qgemm_block2.h, GM = 3) and FluteExperts(glu_blocks=...) on the GPU, at the smallest
shapes at which a 128-row block kernel can still go wrong: empty experts, both sides of a block edge, ragged last blocks, every
exit of the K ring, one to three scale blocks, a block map that crosses a 64-expert chunk, malformed tables and indices,
non-finite source rows, graph replay on another table.

Exact stacks (tests/glu_block_cases): g and u are exact in fp32 whatever the summation order, so H must be within

    |H - E| <= (u_T + eps_s (1 + u_T)) |E| + eta_T,      eps_s = 2^-21 (include/flute_amd.h), eta_T = 2^-24 / 2^-126,

of E = g / (1 + e^-g) * u in fp64, element by element (grouped_cases.assert_glu; the premises are asserted by the reference),
and must equal the row form's bits: silu32 is one function.  Random stacks: within twice the error of the restated
two-launch computation against fp64 on the dequantized weights."""
import pytest
import torch

from tests import exact_cases as XC
from tests.glu_block_cases import (BLOCK_COUNTS, BLOCK_TSRC, GluBlockCase, glu_block_reference, glu_block_rows, glu_blocks_matrix,
                                   glu_blocks_seed0, premised_case, segments_of)
from tests.grouped_cases import assert_glu, dense_project, random_stack, restated_experts, scale_leaves
from tests.support import bits16, env, first_template, max_rel_err, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
COUNTS, TSRC = BLOCK_COUNTS, BLOCK_TSRC
R_ALL = sum(COUNTS)


def test_matrix_covers_what_it_claims():
    m = glu_blocks_matrix()
    assert len(m) == 32
    assert {(b, p, d) for b, p, d, *_ in m} == {(b, p, d) for b in (4, 2) for p in (32, 64) for d in (F16, BF16)}
    for b in (4, 2):
        assert {c[5] for c in m if c[0] == b} == {256, 512} and any(c[6] for c in m if c[0] == b)
        assert {(c[3], c[4]) for c in m if c[0] == b} == {(256, 32), (512, 32), (768, 32), (1024, 64)}
    assert sum(c[6] for c in m) == 6


@pytest.mark.parametrize("bits,tile_p,dtype,K,g,F,pair", glu_blocks_matrix())
def test_exact_matrix_and_equal_to_the_row_form(env, bits, tile_p, dtype, K, g, F, pair):
    lay, Xi, rows, ref, tries = premised_case(bits, tile_p, g, dtype, K, F, pair, COUNTS, TSRC, glu_blocks_seed0(bits, tile_p, K))
    c = GluBlockCase(env, lay)
    H = c.check(COUNTS, ref, rows, (bits, tile_p, dtype, K, g, F, pair, "seed try %d" % tries))
    d = env.dev
    row_form = c.run(ref["X"].to(d), offsets_of(COUNTS, d), rows.int().to(d), blocks=False)
    assert torch.equal(bits16(H), bits16(row_form))


@pytest.mark.parametrize("bits,tile_p,dtype", [(4, 32, F16), (2, 64, BF16)])
def test_random_componentwise(env, bits, tile_p, dtype):
    """K = 2304 (36 steps, nine scale blocks at group size 32), F = 512, rows drawn with repeats from 64 source rows.  R: fp64 on
    the dequantized weights; yardstick: the unfused sequence - gather, two plain grouped launches, silu and the product in T."""
    counts, K, F, g, tsrc = [7, 0, 140, 260], 2304, 512, 32, 64
    d, tid = env.dev, first_template(bits, tile_p)
    Qg, Sg, Tg, Wg = random_stack(env, bits, tile_p, g, dtype, K, F, len(counts), seed=bits * 100 + 11)
    Qu, Su, Tu, Wu = random_stack(env, bits, tile_p, g, dtype, K, F, len(counts), seed=bits * 100 + 51)
    R = sum(counts)
    X = (torch.randn(tsrc, K, generator=torch.Generator().manual_seed(6)) / 8).to(dtype)
    rows = torch.randint(0, tsrc, (R,), generator=torch.Generator().manual_seed(7))
    off = offsets_of(counts)
    Xd, offd, rowsd = X.to(d), off.to(d), rows.int().to(d)
    H = env.fa.qgemm_grouped_glu_blocks(Xd, offd, Qg, Sg, Tg, Qu, Su, Tu, bits, g, tid, env.num_sms, rows=rowsd)
    xs = Xd[rowsd.long()]
    two = torch.nn.functional.silu(env.fa.qgemm_grouped(xs, offd, Qg, Sg, Tg, bits, g, tid, env.num_sms)) * \
        env.fa.qgemm_grouped(xs, offd, Qu, Su, Tu, bits, g, tid, env.num_sms)
    ref = torch.zeros(R, F, dtype=torch.float64)
    for e in range(len(counts)):
        r0, r1 = int(off[e]), int(off[e + 1])
        x = X[rows[r0:r1]].double()
        ref[r0:r1] = torch.nn.functional.silu(x @ Wg[e]) * (x @ Wu[e])
    err, err_two = float((H.double().cpu() - ref).abs().max()), float((two.double().cpu() - ref).abs().max())
    print("glu blocks random %s: max|H - R| = %.3e, two launches %.3e, max|R| = %.3e" % ((bits, tile_p, dtype), err, err_two,
                                                                                       float(ref.abs().max())))
    assert err_two > 0
    assert err <= 2 * err_two, (err, err_two)


@pytest.fixture(scope="module")
def small(env):
    """One exact 4-bit bf16 pair of stacks (TileP 64, K = 512, F = 512) shared by the tests below."""
    lay, Xi, rows, ref, _ = premised_case(4, 64, 32, BF16, 512, 512, False, COUNTS, TSRC, 209500)
    return dict(lay=lay, case=GluBlockCase(env, lay), Xi=Xi, rows=rows, ref=ref)


def test_without_an_index(env, small):
    c, lay = small["case"], small["lay"]
    Xi = XC.make_x(R_ALL, lay.K, 209601, lay.dtype)
    ref = lay.reference(COUNTS, Xi, torch.arange(R_ALL))
    c.check(COUNTS, ref, torch.arange(R_ALL), "rows = None", use_rows=False)


@pytest.mark.parametrize("T", [1, 130])
def test_one_expert(env, T):
    lay, Xi, rows, ref, _ = premised_case(2, 32, 32, BF16, 256, 256, False, [T], 16, 209700 + T)
    GluBlockCase(env, lay).check([T], ref, rows, ("one expert", T))


def test_two_calls_equal_bits(env, small):
    c, d = small["case"], env.dev
    X, off, rows = small["ref"]["X"].to(d), offsets_of(COUNTS, d), small["rows"].int().to(d)
    a, b = c.run(X, off, rows), c.run(X, off, rows)
    assert torch.equal(bits16(a), bits16(b))
    assert not torch.equal(bits16(a), bits16(c.run(X, off, rows.flip(0).contiguous())))


def test_block_map_across_a_64_expert_chunk(env):
    """E = 130, rows in experts 0 and 129 only (129 each: two blocks, the second with one row): the scan over the table takes three
    rounds of 64 experts and the second expert's blocks are found in the last."""
    E = 130
    two, Xi, rows, ref, _ = premised_case(4, 32, 32, F16, 256, 256, False, [129, 129], 64, 209800)
    c2 = GluBlockCase(env, two)
    wide = lambda t: torch.zeros((E,) + t.shape[1:], dtype=t.dtype, device=env.dev)
    ops = [wide(t) for t in c2.ops()]
    for i, e in enumerate((0, 129)):
        for dst, src in zip(ops, c2.ops()):
            dst[e] = src[i]
    counts = [0] * E
    counts[0] = counts[129] = 129
    d = env.dev
    H = env.fa.qgemm_grouped_glu_blocks(ref["X"].to(d), offsets_of(counts, d), *ops, 4, 32, c2.tid, env.num_sms,
                                        rows=rows.int().to(d))
    assert_glu(H, ref["E"], F16, "E = 130")


def abi_call(env, c, X, rows, off, tsrc, guard=160, xfill=float("inf")):
    """The direct call with Xsrc and H in the middle of larger buffers: rows [0, R) of H as int16, after asserting that the guard
    rows in front of H and the rows >= R kept the canary.  The guard rows around Xsrc hold `xfill`."""
    d, lay = env.dev, c.lay
    R = rows.shape[0]
    canary = XC.NAN_BITS[lay.dtype]
    hbuf = torch.full((guard + R + guard, lay.F), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + tsrc + guard, lay.K), xfill, dtype=lay.dtype, device=d)
    xbuf[guard:guard + tsrc] = X.to(d)
    off_d, rows_d = off.to(d), rows.int().to(d)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_glu_blocks(
            0 if lay.dtype == F16 else 1, lay.bits, lay.g, off.shape[0] - 1, R, tsrc, lay.F, lay.K, c.Qg.shape[1], c.tid,
            xbuf[guard:].data_ptr(), rows_d.data_ptr(), off_d.data_ptr(), *[t.data_ptr() for t in c.ops()],
            hbuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(hbuf[:guard] == canary), "front guard"
    assert torch.all(hbuf[guard + R:] == canary), "rows >= R"
    return hbuf[guard:guard + R].cpu()


def test_direct_abi_hostile_tables_and_indices(env, small):
    """Xsrc and H inside larger buffers (the guard rows of Xsrc are Inf: a read outside Xsrc would reach a result).  A last offset
    past R, a decreasing table, overlapping ranges that own more blocks than the grid holds, all-zero offsets, and `rows` entries
    that are negative or >= Tsrc: nothing outside H's R rows is written, every row exactly one expert names is within the bound
    of that expert's result on the clamped source row, and nothing is non-finite."""
    c, lay, E = small["case"], small["lay"], len(COUNTS)
    dtype, canary = lay.dtype, XC.NAN_BITS[lay.dtype]
    rows = small["rows"].clone()
    r3 = int(offsets_of(COUNTS)[3])
    rows[r3:r3 + 4] = torch.tensor([-1, 0, TSRC + 5, TSRC - 1])            # clamped to 0 and Tsrc - 1
    clamped = rows.clamp(0, TSRC - 1)

    def check(off, segments, what):
        ref = glu_block_reference(lay.gate, lay.up, segments, R_ALL, small["Xi"], clamped)
        H = abi_call(env, c, ref["X"], rows, off, TSRC)
        cov = ref["covered"]
        assert_glu(H.view(dtype)[cov], ref["E"][cov], dtype, what)
        return H

    off = offsets_of(COUNTS)
    off[E] = R_ALL + 200
    H = check(off, segments_of(COUNTS), "last offset past R")
    assert torch.equal(H[r3], H[r3 + 1]) and torch.equal(H[r3 + 2], H[r3 + 3]) and not torch.equal(H[r3], H[r3 + 2])
    # a decreasing entry: expert 1 = [100, 50) has no rows, expert 2 = [50, 400) overlaps expert 0 = [0, 100) in rows [50, 100)
    # (unspecified contents there); a negative first entry and a last one far past R are clamped
    dec = torch.tensor([-5, 100, 50, 400, 400, 400, 400, R_ALL + 10 ** 6], dtype=torch.int32)
    H = check(dec, [(0, 0, 50), (2, 100, 400), (6, 400, R_ALL)], "decreasing table")
    assert torch.isfinite(H.view(dtype)[50:100]).all()
    # overlapping ranges that own more blocks than the grid holds: experts 1, 3 and 5 each claim every row (18 blocks, the grid
    # has 12 row blocks), the others [R, 0) - none: whatever was written is some expert's finite result
    H = abi_call(env, c, small["ref"]["X"], rows, torch.tensor([R_ALL, 0, R_ALL, 0, R_ALL, 0, R_ALL, 0], dtype=torch.int32), TSRC)
    written = (H != canary).any(dim=1)
    assert written.any() and torch.isfinite(H.view(dtype)[written]).all()
    # no expert has a row: nothing at all is written
    H = abi_call(env, c, small["ref"]["X"], rows, torch.zeros(E + 1, dtype=torch.int32), TSRC)
    assert torch.all(H == canary)


def test_non_finite_rows_stay_in_their_rows(env, small):
    """A NaN and an Inf source row, each read by several sorted rows in different experts, one of them the last row before an
    expert's end (the rows after it in that block read no index and no activation): exactly the sorted rows that read them are
    non-finite, every other row keeps the bits of the clean launch."""
    c, lay = small["case"], small["lay"]
    off = offsets_of(COUNTS)
    rows = small["rows"].clone()
    nan_row, inf_row = 5, 9
    rows[(rows == nan_row) | (rows == inf_row)] = 0                         # only the rows named below read them
    readers = {int(off[2]) + 3: nan_row, int(off[4]) - 1: nan_row, int(off[5]) - 1: inf_row, int(off[7]) - 300 + 127: inf_row,
               int(off[7]) - 2: nan_row, int(off[3]) + 64: inf_row}
    for r, s in readers.items():
        rows[r] = s
    X = small["ref"]["X"]
    clean = abi_call(env, c, X, rows, off, TSRC)
    assert torch.isfinite(clean.view(lay.dtype)).all()
    Xbad = X.clone()
    Xbad[nan_row, 17], Xbad[inf_row, 33] = float("nan"), float("inf")
    H = abi_call(env, c, Xbad, rows, off, TSRC)
    finite = torch.isfinite(H.view(lay.dtype)).all(dim=1)
    assert sorted((~finite).nonzero().flatten().tolist()) == sorted(readers)
    assert not torch.isfinite(H.view(lay.dtype)[sorted(readers)]).all(dim=1).any()
    assert torch.equal(H[finite], clean[finite])


def test_graph_replay_honours_new_offsets_rows_and_x(env, small):
    """The host reads nothing and the grid follows from (E, R, F) alone: a captured launch (one stream, no parallel branches) replayed
    after offsets, rows and Xsrc were overwritten in place with another table of the same R returns the bits of an eager call."""
    c, lay, d = small["case"], small["lay"], env.dev
    counts2 = [130, 255, 0, 0, 1, 299, 0]
    assert sum(counts2) == R_ALL and len(counts2) == len(COUNTS)
    rows2 = glu_block_rows(R_ALL, TSRC, 209901)
    ref2 = lay.reference(counts2, XC.make_x(TSRC, lay.K, 209902, lay.dtype), rows2, need_witness=False)
    x, off, rows = small["ref"]["X"].to(d).clone(), offsets_of(COUNTS, d), small["rows"].int().to(d)
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
    assert_glu(h, ref2["E"], lay.dtype, "graph replay")
    assert not torch.equal(bits16(eager), bits16(first))


# ---- the module --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def glu_module_case(env):
    """E = 2 experts (4-bit, g = 32, K = 256, N_ff = 256, fp16), top-1, 300 tokens - a mean of 150 rows per expert, above the
    query's threshold; 60 tokens are below it.  `lut`: every layer's lookups [N, K] in fp64."""
    d, dtype = env.dev, F16
    E, K, F, T, bits, g = 2, 256, 256, 300, 4, 32
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(52)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, bits=bits, g=g, tid=tid, dtype=dtype, few=60)
    c["layers"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)], [linear(F, K) for _ in range(E)])
    lut = lambda m: env.fa.dequantize(m.weight, torch.ones_like(m.scales), m.tables2, bits, g, tid).double()
    c["lut"] = [[lut(m) for m in ms] for ms in c["layers"]]
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["dOut"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["ids"] = torch.randint(0, E, (T, 1), generator=gen).to(d)
    c["weights"] = (torch.rand(T, 1, generator=gen) * 0.5 + 0.5).to(dtype).to(d)
    return c


def test_flute_experts_forward_on_the_block_glu(env, glu_module_case):
    """max|Y - R| <= 2 max|Y_loop - R|: R the fp64 result on the dequantized weights, Y_loop the per-expert loop over FluteLinear.
    "auto" takes the block launch at 300 tokens and the row form at 60 (asserted through the query), with the bits of True / False."""
    from flute_amd import dev
    c = glu_module_case
    hidden, ids, weights = c["hidden"], c["ids"], c["weights"]
    make = lambda v: env.moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True, glu_blocks=v)
    Y = make(True)(hidden, ids, weights)
    deq = lambda m: env.fa.dequantize(m.weight, m.scales, m.tables2, c["bits"], c["g"], c["tid"]).double()
    R = restated_experts(c, hidden.double(), ids, weights.double(), lambda e, which, x: x @ deq(c["layers"][which][e]).T)
    Y_loop = restated_experts(c, hidden, ids, weights, lambda e, which, x: c["layers"][which][e](x))
    err, err_loop = float((Y.double() - R).abs().max()), float((Y_loop.double() - R).abs().max())
    print("FluteExperts(glu_blocks=True): max|Y - R| = %.3e, loop %.3e, max|R| = %.3e" % (err, err_loop, float(R.abs().max())))
    assert err_loop > 0
    assert err <= 2 * err_loop, (err, err_loop)
    form = lambda T: dev.grouped_glu_blocks_form(c["E"], T, T, c["F"], c["K"], c["bits"], c["g"], c["tid"], env.num_sms, c["dtype"])
    assert form(c["T"]) == "blocks" and form(c["few"]) == "rows"
    auto, rows_form = make("auto"), make(False)
    assert torch.equal(bits16(auto(hidden, ids, weights)), bits16(Y))
    few = slice(0, c["few"])
    assert torch.equal(bits16(auto(hidden[few], ids[few], weights[few])), bits16(rows_form(hidden[few], ids[few], weights[few])))
    # the other routing path and the block on top of it
    plain = env.moe.FluteExperts.from_linears(*c["layers"], fused=True, glu_blocks=True)
    assert max_rel_err(plain(hidden, ids, weights), R) <= 2 * max_rel_err(Y_loop, R)


def test_flute_experts_backward_with_the_block_glu(env, glu_module_case):
    """One backward with learnable scales against the same step with glu_blocks=False.  The backward recomputes g and u and the
    down projection's input gradient does not read H: hidden.grad and the gate / up scale gradients are bit-equal.  The down
    scale gradient reads H: within twice the glu_blocks=False step's error against fp64 autograd of the restated block."""
    c = glu_module_case
    hidden, ids, weights, dOut = c["hidden"], c["ids"], c["weights"], c["dOut"]
    S64 = scale_leaves(c)
    h64 = hidden.double().requires_grad_()
    restated_experts(c, h64, ids, weights.double(), dense_project(c, S64)).backward(dOut.double())

    def step(glu_blocks):
        experts = env.moe.FluteExperts.from_linears(*c["layers"], fused=True, native_routing=True, glu_blocks=glu_blocks)
        params = env.moe.make_experts_learnable(experts)
        assert len(params) == 3
        h = hidden.clone().requires_grad_()
        experts(h, ids, weights).backward(dOut)
        return [p.grad for p in params] + [h.grad]

    got, yard = step(True), step(False)
    for i in (0, 1, 3):
        assert got[i] is not None and torch.equal(bits16(got[i]), bits16(yard[i])), i
    err, yerr = max_rel_err(got[2], S64[2].grad), max_rel_err(yard[2], S64[2].grad)
    print("block GLU step, down scales.grad: %.3e (glu_blocks=False %.3e)" % (err, yerr))
    assert yerr > 0
    assert err <= 2 * yerr, (err, yerr)
