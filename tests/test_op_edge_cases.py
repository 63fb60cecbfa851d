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


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_combine_rule(dtype):
    c = OE.combine_case(dtype)
    clean = OE.combine_ieee(c, c.Y)
    assert not torch.isnan(clean).any() and int(torch.isinf(clean).sum()) == (dtype == F16)      # 80000 rounds to +inf in fp16
    assert torch.isfinite(c.Y).all() and float(clean[c.t_inf, 50]) >= 65520
    exp = OE.combine_expected(clean, c)
    assert XC.nonfinite_equal(OE.combine_ieee(c, c.Yp), exp)
    assert int(torch.isnan(exp).sum()) == 2 and int(torch.isinf(exp).sum()) == 1 + (dtype == F16) and c.t_nan != c.t_inf
