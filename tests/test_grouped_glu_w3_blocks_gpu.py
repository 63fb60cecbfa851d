"""flute_amd.qgemm_grouped_glu_w3_blocks (qgemm_block3.h, GM = 3) and FluteExperts(w3_glu_blocks=...) on the GPU, at the smallest
shapes at which the kernel can still go wrong: empty experts, both sides of a 128-row block edge, a ragged last block, every exit
of the K ring, one to three scale blocks, a block map that crosses 64-expert chunks, malformed tables and indices, non-finite rows.

Exact stacks (tests/glu_block_cases): g and u are exact in fp32 whatever the summation order, so H must be within assert_glu's
bound of E = g / (1 + e^-g) * u in fp64, element by element, and must equal the row form's bits.  Random stacks: within twice the
error of the unfused two-launch computation against fp64 on the dequantized weights.  (F is 512 or 1024: a 3-bit layer's column
block is 512 wide.)"""
import pytest
import torch

from tests import exact_cases as XC
from tests.glu_block_cases import (BLOCK_COUNTS as COUNTS, BLOCK_K_CASES, BLOCK_TSRC as TSRC, GluBlockCase, glu_block_reference,
                                   premised_case, segments_of)
from tests.grouped_cases import assert_glu, random_stack
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
BITS, TILE_P = 3, 32
R_ALL = sum(COUNTS)
EXACT = [(dtype, K, g, 512 if i % 2 == 0 else 1024, i % 3 == 1)
         for i, (dtype, (K, g)) in enumerate((d, kg) for d in (F16, BF16) for kg in BLOCK_K_CASES)]


def run(env, c, X, off, rows, blocks=True):
    op = env.fa.qgemm_grouped_glu_w3_blocks if blocks else env.fa.qgemm_grouped_glu
    return op(X, off, *c.ops(), BITS, c.lay.g, c.tid, env.num_sms, rows=rows)


def check(env, c, counts, ref, rows, what, use_rows=True):
    d = env.dev
    H = run(env, c, ref["X"].to(d), offsets_of(counts, d), rows.int().to(d) if use_rows else None)
    assert H.shape == (sum(counts), c.lay.F) and H.dtype == c.lay.dtype
    assert_glu(H, ref["E"], c.lay.dtype, (what, "p = %d" % ref["p"], "share %.2f" % ref["share"]))
    return H


@pytest.mark.parametrize("dtype,K,g,F,pair", EXACT)
def test_exact_matrix_and_equal_to_the_row_form(env, dtype, K, g, F, pair):
    lay, Xi, rows, ref, tries = premised_case(BITS, TILE_P, g, dtype, K, F, pair, COUNTS, TSRC, 230000 + K + (dtype == BF16))
    c = GluBlockCase(env, lay)
    H = check(env, c, COUNTS, ref, rows, (dtype, K, g, F, pair, "seed try %d" % tries))
    d = env.dev
    row_form = run(env, c, ref["X"].to(d), offsets_of(COUNTS, d), rows.int().to(d), blocks=False)
    assert torch.equal(bits16(H), bits16(row_form))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_random_componentwise(env, dtype):
    """K = 2304 (36 steps, nine scale blocks at group size 32), F = 512, rows drawn with repeats from 64 source rows.  R: fp64 on
    the dequantized weights; yardstick: the unfused sequence - gather, two plain grouped launches, silu and the product in T."""
    counts, K, F, g, tsrc = [7, 0, 140, 260], 2304, 512, 32, 64
    d, tid = env.dev, first_template(BITS, TILE_P)
    Qg, Sg, Tg, Wg = random_stack(env, BITS, TILE_P, g, dtype, K, F, len(counts), seed=311)
    Qu, Su, Tu, Wu = random_stack(env, BITS, TILE_P, g, dtype, K, F, len(counts), seed=351)
    R = sum(counts)
    X = (torch.randn(tsrc, K, generator=torch.Generator().manual_seed(6)) / 8).to(dtype)
    rows = torch.randint(0, tsrc, (R,), generator=torch.Generator().manual_seed(7))
    off = offsets_of(counts)
    Xd, offd, rowsd = X.to(d), off.to(d), rows.int().to(d)
    H = env.fa.qgemm_grouped_glu_w3_blocks(Xd, offd, Qg, Sg, Tg, Qu, Su, Tu, BITS, g, tid, env.num_sms, rows=rowsd)
    xs = Xd[rowsd.long()]
    two = torch.nn.functional.silu(env.fa.qgemm_grouped(xs, offd, Qg, Sg, Tg, BITS, g, tid, env.num_sms)) * \
        env.fa.qgemm_grouped(xs, offd, Qu, Su, Tu, BITS, g, tid, env.num_sms)
    ref = torch.zeros(R, F, dtype=torch.float64)
    for e in range(len(counts)):
        r0, r1 = int(off[e]), int(off[e + 1])
        x = X[rows[r0:r1]].double()
        ref[r0:r1] = torch.nn.functional.silu(x @ Wg[e]) * (x @ Wu[e])
    err, err_two = float((H.double().cpu() - ref).abs().max()), float((two.double().cpu() - ref).abs().max())
    print("glu w3 blocks random %s: max|H - R| = %.3e, two launches %.3e, max|R| = %.3e" % (dtype, err, err_two, float(ref.abs().max())))
    assert err_two > 0
    assert err <= 2 * err_two, (err, err_two)


@pytest.fixture(scope="module")
def small(env):
    """One exact bf16 pair of 3-bit stacks (K = 512, F = 512) shared by the tests below."""
    lay, Xi, rows, ref, _ = premised_case(BITS, TILE_P, 32, BF16, 512, 512, False, COUNTS, TSRC, 239500)
    return dict(lay=lay, case=GluBlockCase(env, lay), Xi=Xi, rows=rows, ref=ref)


def test_without_an_index(env, small):
    lay = small["lay"]
    Xi = XC.make_x(R_ALL, lay.K, 239601, lay.dtype)
    ref = lay.reference(COUNTS, Xi, torch.arange(R_ALL))
    check(env, small["case"], COUNTS, ref, torch.arange(R_ALL), "rows = None", use_rows=False)


@pytest.mark.parametrize("T", [1, 130])
def test_one_expert(env, T):
    lay, Xi, rows, ref, _ = premised_case(BITS, TILE_P, 32, BF16, 256, 512, False, [T], 16, 239700 + T)
    check(env, GluBlockCase(env, lay), [T], ref, rows, ("one expert", T))


def test_block_map_across_64_expert_chunks(env):
    """E = 130, rows in experts 0 and 129 only (129 each: two blocks, the second with one row): the scan over the table takes three
    rounds of 64 experts and the second expert's blocks are found in the last."""
    E = 130
    two, Xi, rows, ref, _ = premised_case(BITS, TILE_P, 32, F16, 256, 512, False, [129, 129], 64, 239800)
    c2 = GluBlockCase(env, two)
    ops = [torch.zeros((E,) + t.shape[1:], dtype=t.dtype, device=env.dev) for t in c2.ops()]
    for i, e in enumerate((0, 129)):
        for dst, src in zip(ops, c2.ops()):
            dst[e] = src[i]
    counts = [0] * E
    counts[0] = counts[129] = 129
    d = env.dev
    H = env.fa.qgemm_grouped_glu_w3_blocks(ref["X"].to(d), offsets_of(counts, d), *ops, BITS, 32, c2.tid, env.num_sms,
                                           rows=rows.int().to(d))
    assert_glu(H, ref["E"], F16, "E = 130")


def abi_call(env, c, X, rows, off, tsrc, guard=160, xfill=float("inf")):
    """The direct call with Xsrc (between rows of `xfill`) and H (between canary rows, asserted intact) inside larger buffers."""
    d, lay = env.dev, c.lay
    R = rows.shape[0]
    canary = XC.NAN_BITS[lay.dtype]
    hbuf = torch.full((guard + R + guard, lay.F), canary, dtype=torch.int16, device=d)
    xbuf = torch.full((guard + tsrc + guard, lay.K), xfill, dtype=lay.dtype, device=d)
    xbuf[guard:guard + tsrc] = X.to(d)
    off_d, rows_d = off.to(d), rows.int().to(d)
    with torch.cuda.device(d):
        rc = env.lib.flute_qgemm_grouped_glu_w3_blocks(
            0 if lay.dtype == F16 else 1, BITS, lay.g, off.shape[0] - 1, R, tsrc, lay.F, lay.K, c.Qg.shape[1], c.tid,
            xbuf[guard:].data_ptr(), rows_d.data_ptr(), off_d.data_ptr(), *[t.data_ptr() for t in c.ops()],
            hbuf[guard:].data_ptr(), env.num_sms, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(hbuf[:guard] == canary), "front guard"
    assert torch.all(hbuf[guard + R:] == canary), "rows >= R"
    return hbuf[guard:guard + R].cpu()


def test_direct_abi_hostile_tables_and_indices(env, small):
    """Out-of-range `rows` entries clamp; a decreasing entry, a negative first and a last entry far past R write exactly the rows
    one expert names, within the bound of that expert's result."""
    c, lay = small["case"], small["lay"]
    rows = small["rows"].clone()
    r3 = int(offsets_of(COUNTS)[3])
    rows[r3:r3 + 4] = torch.tensor([-1, 0, TSRC + 5, TSRC - 1])            # clamped to 0 and Tsrc - 1
    clamped = rows.clamp(0, TSRC - 1)

    def hostile(off, segments, what):
        ref = glu_block_reference(lay.gate, lay.up, segments, R_ALL, small["Xi"], clamped)
        H = abi_call(env, c, ref["X"], rows, off, TSRC)
        cov = ref["covered"]
        assert_glu(H.view(lay.dtype)[cov], ref["E"][cov], lay.dtype, what)
        return H, cov

    H, _ = hostile(offsets_of(COUNTS), segments_of(COUNTS), "clamped rows")
    assert torch.equal(H[r3], H[r3 + 1]) and torch.equal(H[r3 + 2], H[r3 + 3]) and not torch.equal(H[r3], H[r3 + 2])
    # expert 1 = [100, 50) has no rows, expert 2 = [50, 400) overlaps expert 0 = [0, 100) in rows [50, 100): unspecified, finite
    dec = torch.tensor([-5, 100, 50, 400, 400, 400, 400, R_ALL + 10 ** 6], dtype=torch.int32)
    H, _ = hostile(dec, [(0, 0, 50), (2, 100, 400), (6, 400, R_ALL)], "decreasing table")
    assert torch.isfinite(H.view(lay.dtype)[50:100]).all()
    H = abi_call(env, c, small["ref"]["X"], rows, torch.zeros(len(COUNTS) + 1, dtype=torch.int32), TSRC)     # no expert has a row
    assert torch.all(H == XC.NAN_BITS[lay.dtype])


def test_non_finite_rows_stay_in_their_rows(env, small):
    """A NaN and an Inf source row reach exactly the sorted rows that name them; every other row keeps the clean launch's bits."""
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
    assert torch.equal(H[finite], clean[finite])


def test_flute_experts_forward_and_backward_equal_the_default(env):
    """Inputs on which every sum is exact in fp32 in any order (one-hot tokens of 4, g = 4 t in [20, 30], u in +-{1 .. 4}, down
    weights integers / 16): output and hidden-state gradient of `w3_glu_blocks=True` have the bits of False, "auto"'s output too."""
    E, K, F, g, T, dtype, d = 2, 512, 512, 32, 300, F16, env.dev
    tid, gen = first_template(BITS, TILE_P), torch.Generator().manual_seed(239900)
    tables = (torch.tensor([5, 5.25, 5.5, 6, 6.25, 6.5, 7, 7.5]), torch.tensor([-1, -.75, -.5, -.25, .25, .5, .75, 1]),
              torch.arange(-4., 4.))

    def linear(kk, nn, table, scale):
        codes = torch.randint(0, 8, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        return env.FluteLinear.from_codes(codes, torch.full((nn, kk // g), scale, dtype=dtype, device=d), table.to(dtype).to(d),
                                          BITS, g, tid)

    layers = [[linear(kk, nn, table, scale) for _ in range(E)]
              for kk, nn, table, scale in ((K, F, tables[0], 1.0), (K, F, tables[1], 1.0), (F, K, tables[2], 2.0 ** -4))]
    hidden = torch.zeros(T, K, dtype=dtype)
    hidden[torch.arange(T), torch.randint(0, K, (T,), generator=gen)] = 4
    ids = torch.randint(0, E, (T, 1), generator=gen).to(d)
    weights = torch.ones(T, 1, dtype=dtype, device=d)
    dOut = XC.make_x(T, K, 239901, dtype).to(d)

    def step(value):
        experts = env.moe.FluteExperts.from_linears(*layers, fused=True, native_routing=True, w3_glu_blocks=value)
        h = hidden.to(d).requires_grad_()
        y = experts(h, ids, weights)
        y.backward(dOut)
        return y.detach(), h.grad

    (y, dh), (y0, dh0), (ya, _) = step(True), step(False), step("auto")
    assert torch.isfinite(y).all() and y.abs().max() > 0 and dh.abs().max() > 0
    assert torch.equal(bits16(y), bits16(y0)) and torch.equal(bits16(dh), bits16(dh0)) and torch.equal(bits16(ya), bits16(y0))
