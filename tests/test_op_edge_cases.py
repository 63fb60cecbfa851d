"""tests/op_edge_cases.py checked on the CPU: every construction the GPU tests launch is built here (the builders assert
their premises), and every non-finite rule is compared with an fp64 torch evaluation of the op's documented formula on
the poisoned data - IEEE arithmetic decides which elements are NaN, +inf or -inf, and the rule must give that pattern
and leave every other element as the clean evaluation has it."""
import pytest
import torch

from tests import exact_cases as XC
from tests import op_edge_cases as OE
from tests import scale_grad_ref as SR
from tests import table_grad_ref as TR
from tests.grouped_cases import counts_of

F16, BF16 = torch.float16, torch.bfloat16


def test_shapes_cross_the_kernels_boundaries():
    off = OE.offsets_list(OE.FWD_COUNTS)
    assert OE.FWD_COUNTS[0] == 0 and 0 in OE.FWD_COUNTS[1:-1]
    assert any(0 < o % 16 for o in off[1:-1]) and max(OE.FWD_COUNTS) > 32        # seams inside a tile, a second row pass
    assert OE.K_EDGE % 64 == 0 and OE.K_EDGE % 256 != 0
    assert OE.grad_counts() == counts_of(OE.ROW_BLOCK)
    for bits, g in OE.SG_CASES:
        K, N = OE.sg_shape(bits)
        assert OE.sg_splits(OE.SG_M, N, K, g, 256, 1 << 24)[0] >= 2 and OE.sg_splits(OE.SG_M, N, K, g, 256, 0)[0] == 1
    assert min(n for n in OE.SG_COUNTS if n) < 32 < max(OE.SG_COUNTS) and 0 in OE.SG_COUNTS


def served_by_the_block_forms(c, forward):
    """include/flute_amd.h: the forward's block form serves 4 / 2 bits, (K / group_size) % 8 == 0 and N % 256 == 0, the
    gradient's 4 / 2 bits and K % 256 == 0; and the layer itself is legal (N whole column blocks of the layout)."""
    assert c.bits in (4, 2) and c.N % XC.cols_per_block(c.bits, c.tile_p) == 0 and c.K % max(64, c.g) == 0
    assert c.counts == OE.grad_counts() and c.block
    if forward:
        assert c.N % 256 == 0 and c.K % c.g == 0 and (c.K // c.g) % 8 == 0, (c.K, c.N, c.g)
    else:
        assert c.K % 256 == 0, c.K
    return True


def test_block_shapes_are_what_the_block_forms_serve():
    """Every block-variant case the GPU tests launch, and what its shape crosses: an empty first and middle expert, one row,
    both sides of a 128-row block, a second block of one row and a ragged third; an expert of at most 64 rows (the second
    row group's waves of the gradient kernel sit out); two k blocks in the gradient, every K the forward's ring exits on."""
    counts, rb = OE.grad_counts(), OE.ROW_BLOCK
    assert counts == [0, 1, 127, 128, 129, 0, 259, 5] and counts == counts_of(rb)
    assert any(0 < n <= 64 for n in counts) and any(n % rb == 1 and n > rb for n in counts) and max(counts) > 2 * rb
    for op, kind, b, p, g in OE.block_forward_range_params():
        c = OE.forward_range_case(op, kind, b, p, g, block=True)
        assert served_by_the_block_forms(c, True) and c.K == (XC.OVERFLOW_K if kind == "overflow" else 8 * g)
    for b, p in OE.block_pushed_params():
        assert served_by_the_block_forms(OE.weighted_pushed_case(b, p, block=True), True)
    for op, b, p, g, dtype in OE.block_forward_nonfinite_params():
        c = OE.forward_nonfinite_case(op, b, p, g, dtype, block=True)
        assert served_by_the_block_forms(c, True) and c.K == 8 * g and c.N == max(256, XC.cols_per_block(b, p))
    for form, kind, b, p, g in OE.block_grad_range_params():
        c = OE.grad_range_case(form, kind, b, p, g, block=True)
        assert served_by_the_block_forms(c, False)
        assert (c.K, c.N) == ((256, OE.GRAD_OVERFLOW_N) if kind == "overflow" else (512, max(256, XC.cols_per_block(b, p))))
    for form, b, p, g, dtype in OE.block_grad_nonfinite_params():
        c = OE.grad_nonfinite_case(form, b, p, g, dtype, block=True)
        assert served_by_the_block_forms(c, False) and c.K == 512
    # the configurations: 4 and 2 bits at TileP 32 and 64 with g = 64 everywhere, (4, 32) at g = 32 where G_CASES adds it
    want = {(4, 32, 64), (2, 32, 64), (4, 64, 64), (2, 64, 64)}
    assert {p[2:] for p in OE.block_forward_range_params() if p[1] != "subw"} == want
    assert {p[2:] for p in OE.block_forward_range_params() if p[1] == "subw"} == want | {(4, 32, 32)}
    assert {p[1:4] for p in OE.block_forward_nonfinite_params() if p[4] == BF16} == want
    assert {p[1:4] for p in OE.block_forward_nonfinite_params() if p[4] == F16} == want | {(4, 32, 32)}
    assert {p[2:] for p in OE.block_grad_range_params()} == want | {(4, 32, 32)}
    assert {p[1:4] for p in OE.block_grad_nonfinite_params()} == want | {(4, 32, 32)}
    assert {p[0] for p in OE.block_grad_range_params()} == {p[0] for p in OE.block_grad_nonfinite_params()} == {"single", "pair", "weighted"}
    # the existing cases stay off the block forms: that is why the block variants exist
    assert not OE.forward_blocks_eligible(4, 64, OE.K_EDGE, 3 * 128) and not OE.grad_blocks_eligible(4, OE.K_EDGE)
    assert not OE.grad_blocks_eligible(4, OE.GRAD_OVERFLOW_K)


def check_forward_range_premises(c, kind):
    Rt = c.R.to(c.dtype)
    assert not torch.isnan(Rt).any()
    if kind != "overflow":                                  # a kernel that flushed the subnormal operand would be seen
        flushed = OE.forward_exact(c.layers, c.counts, c.X, flush_w=kind == "subw", flush_x=kind == "subx")[0]
        if c.rw is not None:
            flushed = flushed * c.rw.double()[:, None]
        assert not XC.exact_equal(Rt, flushed, c.dtype)
    else:
        assert not XC.exact_equal(Rt, c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX), c.dtype)


@pytest.mark.parametrize("op,kind,bits,tile_p,g", OE.block_forward_range_params())
def test_block_forward_range_premises(op, kind, bits, tile_p, g):
    c = OE.forward_range_case(op, kind, bits, tile_p, g, block=True)
    check_forward_range_premises(c, kind)
    off = OE.offsets_list(c.counts)
    if op == "weighted":                                     # the zero weight sits on a row of the largest expert
        assert float(c.rw[off[6] + 3]) == 0 and not c.R[off[6] + 3].any()
    if kind == "overflow":                                   # every expert with three rows or more overflows both ways
        for e, n in enumerate(c.counts):
            if n >= 3 and op == "plain":
                assert OE.has_both_infs(c.R[off[e]:off[e + 1]], c.dtype), e


@pytest.mark.parametrize("bits,tile_p", OE.block_pushed_params())
def test_block_weighted_pushed_premises(bits, tile_p):
    c = OE.weighted_pushed_case(bits, tile_p, block=True)
    assert torch.isinf(c.R.to(c.dtype)[c.a]).any() and float(c.rw[c.a]) == -float(c.rw[c.b])
    assert OE.expert_of_row(c.counts, c.a) == OE.expert_of_row(c.counts, c.b) == 6


@pytest.mark.parametrize("op,kind,bits,tile_p,g", OE.forward_range_params())
def test_forward_range_premises(op, kind, bits, tile_p, g):
    c = OE.forward_range_case(op, kind, bits, tile_p, g)
    Rt = c.R.to(c.dtype)
    assert not torch.isnan(Rt).any()
    if kind != "overflow":                                  # a kernel that flushed the subnormal operand would be seen
        flushed = OE.forward_exact(c.layers, c.counts, c.X, flush_w=kind == "subw", flush_x=kind == "subx")[0]
        if c.rw is not None:
            flushed = flushed * c.rw.double()[:, None]
        assert not XC.exact_equal(Rt, flushed, c.dtype)
    else:
        assert not XC.exact_equal(Rt, c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX), c.dtype)


@pytest.mark.parametrize("bits,tile_p", OE.pushed_params())
def test_weighted_pushed_premises(bits, tile_p):
    c = OE.weighted_pushed_case(bits, tile_p)
    assert torch.isinf(c.R.to(c.dtype)[c.a]).any() and float(c.rw[c.a]) == -float(c.rw[c.b])


@pytest.mark.parametrize("bits,tile_p,g,dtype,use_rows", OE.glu_saturation_params())
def test_glu_saturation_premises(bits, tile_p, g, dtype, use_rows):
    c = OE.glu_saturation_case(bits, tile_p, g, dtype, use_rows)
    # the rewrite g e^g / (1 + e^g) in fp32 is NaN for g > 88: the class it would fail is populated
    assert int((c.G > 89).sum()) >= 64
    # in fp64 the documented formula agrees with the saturated forms to far below the rounding to T
    E = c.Eref
    assert float(((E - c.P)[c.hi].abs() / c.P[c.hi].abs().clamp(min=1)).max()) < 2.0 ** -24
    assert float(E[c.lo].abs().max()) < 2.0 ** -100


@pytest.mark.parametrize("op,bits,tile_p,g,dtype,use_rows", OE.forward_nonfinite_params())
def test_forward_nonfinite_rule(op, bits, tile_p, g, dtype, use_rows):
    c = OE.forward_nonfinite_case(op, bits, tile_p, g, dtype, use_rows)
    clean = OE.forward_ieee(c, c.X)
    assert torch.isfinite(clean).all()
    if op == "weighted":
        assert not clean[40].any()                          # a row weight of zero on a finite row: zeros
    for la in c.launches:
        exp = OE.rowwise_expected(clean, la.poisons)
        assert XC.nonfinite_equal(OE.forward_ieee(c, la.X), exp), la.name
        assert len({OE.expert_of_row(c.counts, r) for r, _ in la.poisons}) >= (2 if la.name != "second row pass" else 1)
        for r, s in la.poisons:
            if s is not None and not (op == "weighted" and float(c.rw[r]) == 0):
                assert torch.isinf(exp[r]).any(), "the Inf row shows infinities"
    if use_rows:
        for t in (7, 22):
            assert len({OE.expert_of_row(c.counts, r) for r in (c.rows == t).nonzero().reshape(-1).tolist()}) == 2


def check_block_places(c, launches):
    """The four places of op_edge_cases.block_places, as (name, NaN row, Inf row): what each one crosses."""
    off = OE.offsets_list(c.counts)
    rb = OE.ROW_BLOCK
    assert [la[0] for la in launches] == [p[0] for p in OE.block_places(None, None, None)]
    (_, n0, i0), (_, n1, i1), (_, n2, i2), (_, n3, i3) = launches
    assert n0 == off[3] - 1 and i0 == off[3] and (n0 - off[2]) % rb != rb - 1          # the last valid row of a ragged block | the next expert
    assert n1 == off[5] - 1 and i1 == off[6] and c.counts[5] == 0                     # across the empty expert
    assert (n2 - off[6]) // rb == 1 and (i2 - off[6]) // rb == 2 and off[6] <= n2 and i2 < off[7]   # the second and the third block
    assert (n3, i3) == (i0, n0)                                                     # the Inf in the last valid row
    if c.rw is not None:
        assert float(c.rw[i0]) < 0 and float(c.rw[i1]) == 0 and float(c.rw[i2]) > 0 and float(c.rw[i3]) != 0
        assert float(c.rw[OE.BLOCK_ZERO_WEIGHT_ROW]) == 0 and off[6] <= OE.BLOCK_ZERO_WEIGHT_ROW < off[7]


@pytest.mark.parametrize("op,bits,tile_p,g,dtype", OE.block_forward_nonfinite_params())
def test_block_forward_nonfinite_rule(op, bits, tile_p, g, dtype):
    c = OE.forward_nonfinite_case(op, bits, tile_p, g, dtype, block=True)
    clean = OE.forward_ieee(c, c.X)
    assert torch.isfinite(clean).all()
    if op == "weighted":
        assert not clean[OE.BLOCK_ZERO_WEIGHT_ROW].any()
    check_block_places(c, [(la.name, la.poisons[0][0], la.poisons[1][0]) for la in c.launches])
    for la in c.launches:
        exp = OE.rowwise_expected(clean, la.poisons)
        assert XC.nonfinite_equal(OE.forward_ieee(c, la.X), exp), la.name
        (r_nan, s_nan), (r_inf, s_inf) = la.poisons
        assert s_nan is None and torch.isnan(exp[r_nan]).all()
        if op == "weighted" and float(c.rw[r_inf]) == 0:
            assert torch.isnan(exp[r_inf]).all()             # zero times Inf
        else:
            assert torch.isinf(exp[r_inf]).any(), "the Inf row shows infinities"


@pytest.mark.parametrize("form,kind,bits,tile_p,g", OE.grad_range_params())
def test_grad_range_premises(form, kind, bits, tile_p, g):
    c = OE.grad_range_case(form, kind, bits, tile_p, g)
    Rt = c.R.to(c.dtype)
    if kind == "overflow":
        assert c.N == 4096 and c.K == 128
        assert not XC.exact_equal(Rt, c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX), c.dtype)
    elif form == "single":
        flushed = OE.grad_exact(c.layers, c.counts, c.dY, flush_w=kind == "subw", flush_y=kind == "subx")[0]
        assert not XC.exact_equal(Rt, flushed, c.dtype)


@pytest.mark.parametrize("form,bits,tile_p,g,dtype", OE.grad_nonfinite_params())
def test_grad_nonfinite_rule(form, bits, tile_p, g, dtype):
    c = OE.grad_nonfinite_case(form, bits, tile_p, g, dtype)
    clean = OE.grad_ieee(c, c.dY, c.dY2)
    assert torch.isfinite(clean).all()
    for la in c.launches:
        exp = OE.rowwise_expected(clean, la.poisons)
        assert XC.nonfinite_equal(OE.grad_ieee(c, la.dY, la.dY2), exp), la.name


@pytest.mark.parametrize("form,kind,bits,tile_p,g", OE.block_grad_range_params())
def test_block_grad_range_premises(form, kind, bits, tile_p, g):
    c = OE.grad_range_case(form, kind, bits, tile_p, g, block=True)
    Rt = c.R.to(c.dtype)
    off = OE.offsets_list(c.counts)
    if kind == "overflow":
        assert c.N == 4096 and c.K == 256
        assert not XC.exact_equal(Rt, c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX), c.dtype)
        assert c.big == [2, 3, 4, 6, 7]                     # the experts with five rows or more carry the edge rows
        if form == "pair":                                  # two halves that overflow alone cancel to exactly zero; rows 3, 4 overflow
            for e in c.big:
                assert not c.R[off[e]:off[e] + 2].any() and torch.isinf(Rt[off[e] + 3:off[e] + 5]).any()
    elif form == "single":
        flushed = OE.grad_exact(c.layers, c.counts, c.dY, flush_w=kind == "subw", flush_y=kind == "subx")[0]
        assert not XC.exact_equal(Rt, flushed, c.dtype)


@pytest.mark.parametrize("form,bits,tile_p,g,dtype", OE.block_grad_nonfinite_params())
def test_block_grad_nonfinite_rule(form, bits, tile_p, g, dtype):
    c = OE.grad_nonfinite_case(form, bits, tile_p, g, dtype, block=True)
    clean = OE.grad_ieee(c, c.dY, c.dY2)
    assert torch.isfinite(clean).all()
    if form == "weighted":
        assert not clean[OE.BLOCK_ZERO_WEIGHT_ROW].any()
    check_block_places(c, [(la.name, la.poisons[0][0], la.poisons[1][0]) for la in c.launches])
    for i, la in enumerate(c.launches):
        exp = OE.rowwise_expected(clean, la.poisons)
        assert XC.nonfinite_equal(OE.grad_ieee(c, la.dY, la.dY2), exp), la.name
        assert not torch.isfinite(exp[la.poisons[1][0]]).any()
        # the pair form's second place poisons the second stack, every other launch the first
        second = form == "pair" and i == 1
        assert torch.isfinite(la.dY).all() == second and (la.dY2 is None or torch.isfinite(la.dY2).all() != second)


@pytest.mark.parametrize("kind,bits,tile_p", OE.dequant_params())
def test_dequant_premises(kind, bits, tile_p):
    c = OE.dequant_case(kind, bits, tile_p)
    assert c.want.shape == (c.lay.N, c.lay.K)


@pytest.mark.parametrize("kind,bits,g", OE.sg_range_params())
def test_scale_grad_range_premises(kind, bits, g):
    c = OE.sg_dense_case(kind, bits, g)
    assert c.M >= 256 + 3
    gc = OE.sg_grouped_case(kind, bits, g)
    off = OE.offsets_list(gc.counts)
    for e, n in enumerate(gc.counts):                       # the grouped reference per expert is the dense one on its rows
        if n:
            R = SR.scale_grad(gc.dY[off[e]:off[e + 1]], gc.X[off[e]:off[e + 1]], OE.lut(gc.layers[e]), g)
            assert torch.equal(R, gc.R[e])
        else:
            assert not gc.R[e].any()


@pytest.mark.parametrize("bits,g", OE.SG_CASES)
def test_scale_grad_row_weight_premises(bits, g):
    c = OE.sg_row_weight_case(bits, g)
    assert torch.isinf(c.pre[c.r_big]).any()


def check_scale_grad_rule(dY, X, L, g, dtype, xs, ys):
    clean = SR.scale_grad(dY, X, L, g).to(dtype)
    assert torch.isfinite(clean).all()
    dYp, Xp = OE.poison(dY, ys), OE.poison(X, xs)
    exp = OE.scale_grad_expected(clean, dYp, Xp, L, g)
    assert XC.nonfinite_equal(OE.scale_grad_ieee(dYp, Xp, L, g).to(dtype), exp)
    return exp


@pytest.mark.parametrize("bits,g,dtype", OE.sg_nonfinite_params())
def test_scale_grad_nonfinite_rule(bits, g, dtype):
    c = OE.sg_nonfinite_dense_case(bits, g, dtype)
    L = OE.lut(c.lay)
    _, sps = OE.sg_splits(c.M, c.lay.N, c.lay.K, g, 256, 1 << 24)
    cut = 32 * sps
    for launches in (c.unsplit, c.tail, OE.mreduce_launches(cut - 1, cut, c.lay.K, c.lay.N, g)):
        for name, xs, ys in launches:
            exp = check_scale_grad_rule(c.dY, c.X, L, g, dtype, xs, ys)
            assert torch.isnan(exp).any() and (torch.isinf(exp).any() or name.startswith("on dY"))
    assert c.M % 32 and any(r == c.M - 1 and v == OE.INF for r, _, v in c.tail[0][1])      # an Inf in a last row before masked rows
    for weighted in (False, True):
        gc = OE.sg_nonfinite_grouped_case(bits, g, dtype, weighted)
        off = OE.offsets_list(gc.counts)
        for name, xs, ys in gc.launches:
            dYp = OE.premultiplied(OE.poison(gc.dY, ys), gc.rw)
            Xp = OE.poison(gc.X, xs)
            for e, n in enumerate(gc.counts):
                if not n:
                    continue
                sl = slice(off[e], off[e + 1])
                Le = OE.lut(gc.layers[e])
                clean = SR.scale_grad(OE.premultiplied(gc.dY, gc.rw)[sl], gc.X[sl], Le, g).to(dtype)
                exp = OE.scale_grad_expected(clean, dYp[sl], Xp[sl], Le, g)
                assert XC.nonfinite_equal(OE.scale_grad_ieee(dYp[sl], Xp[sl], Le, g).to(dtype), exp)
                # an Inf or a NaN in expert a leaves expert b's block untouched
                assert (not torch.isfinite(exp).all()) == (e in gc.touched), (name, e)


@pytest.mark.parametrize("bits,g,dtype", OE.sg_nonfinite_params())
def test_table_grad_nonfinite_rule(bits, g, dtype):
    c = OE.tg_nonfinite_case(bits, g, dtype)
    lay = c.lay
    clean = TR.table_grad(c.dY, c.X, lay.W, lay.S, bits, g).float()
    for name, xs, ys in c.launches:
        dYp, Xp = OE.poison(c.dY, ys), OE.poison(c.X, xs)
        exp = OE.table_grad_expected(clean, dYp, Xp, lay.W, lay.S, bits, g)
        got = OE.table_grad_ieee(dYp, Xp, lay.W, lay.S, bits, g).float()
        nd, ne = torch.isnan(got), torch.isnan(exp)
        assert torch.equal(nd, ne) and torch.equal(got.masked_fill(nd, 0), exp.masked_fill(ne, 0)), name
        assert ne.any() and (torch.isfinite(exp).any() or name.startswith("on dY"))      # (a column of dY feeds every bin of a small table)
        if name.startswith("on X"):                         # exactly the bins of one pair row, one half
            k0 = xs[0][1]
            bins = TR.pair_index(lay.W, bits)[k0 >> 1].unique()
            assert torch.equal(torch.isnan(exp[:, k0 & 1]).nonzero().reshape(-1), bins) or (xs[1][1] & 1) == (k0 & 1)


def table_rule_holds(clean, dYp, Xp, lay):
    """table_grad_expected against the fp64 IEEE evaluation, compared in fp32; returns the expectation."""
    exp = OE.table_grad_expected(clean, dYp, Xp, lay.W, lay.S, lay.bits, lay.g)
    got = OE.table_grad_ieee(dYp, Xp, lay.W, lay.S, lay.bits, lay.g).float()
    nd, ne = torch.isnan(got), torch.isnan(exp)
    assert torch.equal(nd, ne) and torch.equal(got.masked_fill(nd, 0), exp.masked_fill(ne, 0))
    return exp


@pytest.mark.parametrize("bits,g,dtype,weighted", OE.tg_nonfinite_grouped_params())
def test_table_grad_nonfinite_grouped_rule(bits, g, dtype, weighted):
    """Per expert the dense rule on the expert's rows of the premultiplied dY: only the two experts at the seam are touched."""
    c = OE.tg_nonfinite_grouped_case(bits, g, dtype, weighted)
    assert c.counts == OE.SG_COUNTS and (c.layers[0].K, c.layers[0].N) == OE.sg_shape(bits) and c.layers[0].tile_p == 32
    off = OE.offsets_list(c.counts)
    assert [n for n, _, _ in c.launches] == [n for n, _, _ in OE.seam_launches(off[2] - 1, off[2], *OE.sg_shape(bits), g)]
    pre = OE.premultiplied(c.dY, c.rw)
    for name, xs, ys in c.launches:
        dYp, Xp = OE.premultiplied(OE.poison(c.dY, ys), c.rw), OE.poison(c.X, xs)
        for e, n in enumerate(c.counts):
            if not n:
                continue
            sl, lay = slice(off[e], off[e + 1]), c.layers[e]
            clean = TR.table_grad(pre[sl], c.X[sl], lay.W, lay.S, bits, g).float()
            exp = table_rule_holds(clean, dYp[sl], Xp[sl], lay)
            assert (not torch.isfinite(exp).all()) == (e in c.touched), (name, e)
            clean_s = SR.scale_grad(pre[sl], c.X[sl], OE.lut(lay), g).to(dtype)
            exp_s = OE.scale_grad_expected(clean_s, dYp[sl], Xp[sl], OE.lut(lay), g)
            assert XC.nonfinite_equal(OE.scale_grad_ieee(dYp[sl], Xp[sl], OE.lut(lay), g).to(dtype), exp_s)


@pytest.mark.parametrize("kind,bits,g", OE.tg_range_params())
def test_table_grad_range_premises(kind, bits, g):
    """tg_exact asserts the exactness; here: the references are the documented formula per expert, and non-trivial."""
    c = OE.tg_range_case(kind, bits, g, grouped=False)
    assert c.M >= 256 + 3 and c.RT.shape == (4 ** bits, 2) and XC.is_subnormal_f16((c.dY if kind == "subdy" else c.X).double()).any()
    assert torch.equal(c.RT, TR.table_grad(c.dY, c.X, c.lay.W, c.lay.S, bits, g))
    gc = OE.tg_range_case(kind, bits, g, grouped=True)
    off = OE.offsets_list(gc.counts)
    assert gc.counts == OE.SG_COUNTS
    for e, n in enumerate(gc.counts):
        sl = slice(off[e], off[e + 1])
        if n:
            lay = gc.layers[e]
            assert torch.equal(gc.RT[e], TR.table_grad(gc.dY[sl], gc.X[sl], lay.W, lay.S, bits, g)) and gc.RT[e].any()
            assert torch.equal(gc.R[e], SR.scale_grad(gc.dY[sl], gc.X[sl], OE.lut(lay), g))
        else:
            assert not gc.RT[e].any() and not gc.R[e].any()


@pytest.mark.parametrize("bits,g", OE.SG_CASES)
def test_table_grad_row_weight_rule(bits, g):
    """round_T(rw dY) overflows on one row: that expert's bins and dS entries by the rules on the premultiplied dY, from the
    clean values of the premultiplied dY with the infinite entries zero; every other expert is finite."""
    c = OE.tg_row_weight_case(bits, g)
    assert torch.equal(c.pre, OE.premultiplied(c.dY, c.rw))
    off = OE.offsets_list(c.counts)
    for e, n in enumerate(c.counts):
        if not n:
            continue
        sl, lay = slice(off[e], off[e + 1]), c.layers[e]
        assert torch.isfinite(c.pre[sl]).all() == (e != c.e_big)
        clean = TR.table_grad(c.pre_finite[sl], c.X[sl], lay.W, lay.S, bits, g).float()
        exp = table_rule_holds(clean, c.pre[sl], c.X[sl], lay)
        assert torch.isfinite(exp).all() == (e != c.e_big)
        clean_s = SR.scale_grad(c.pre_finite[sl], c.X[sl], OE.lut(lay), g).to(F16)
        exp_s = OE.scale_grad_expected(clean_s, c.pre[sl], c.X[sl], OE.lut(lay), g)
        assert XC.nonfinite_equal(OE.scale_grad_ieee(c.pre[sl], c.X[sl], OE.lut(lay), g).to(F16), exp_s)
        if e == c.e_big:                                    # a column of dS whose dY entry stayed finite keeps its clean bits
            cols = torch.isinf(c.pre[c.r_big])
            assert not torch.isfinite(exp_s[cols]).any() and (~cols).any()
            assert torch.equal(exp_s[~cols].view(torch.int16), clean_s[~cols].view(torch.int16)) and not torch.isnan(clean_s).any()


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_combine_rule(dtype):
    c = OE.combine_case(dtype)
    clean = OE.combine_ieee(c, c.Y)
    assert not torch.isnan(clean).any() and int(torch.isinf(clean).sum()) == (dtype == F16)      # 80000 rounds to +inf in fp16
    assert torch.isfinite(c.Y).all() and float(clean[c.t_inf, 50]) >= 65520
    exp = OE.combine_expected(clean, c)
    assert XC.nonfinite_equal(OE.combine_ieee(c, c.Yp), exp)
    assert int(torch.isnan(exp).sum()) == 2 and int(torch.isinf(exp).sum()) == 1 + (dtype == F16) and c.t_nan != c.t_inf
