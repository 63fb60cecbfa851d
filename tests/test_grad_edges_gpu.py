"""dequantize, the scale gradients (dense unsplit and split, grouped, row-weighted), the table gradient, moe_combine and the
dense qgemm backward on hostile operands (tests/op_edge_cases.py).

Range edges: dequantize returns round_T(lut * s) bit for bit with subnormals kept and +-inf where due; the scale gradients
return round_T of the fp64 sum by value for subnormal dY, subnormal X and sums that overflow fp16 in both directions,
with equal bits unsplit and through the fp32 scratch of a split M, and per expert the dense op's bits.  Non-finite: a NaN
or an Inf in one row reaches exactly the elements the documented formula connects it to - one k group or one column of
one expert's dS, the bins of dT2 its pair row feeds, one token of moe_combine - and everything else keeps the bits of
the clean launch.  The table gradients, dense and grouped, return the fp64 sum by value in fp32 for fp16-subnormal dY and X;
the grouped one keeps a NaN or an Inf on either side of a seam between two experts inside the expert that owns the row, by
the dense rules on that expert's rows, and a row weight whose product with dY overflows T is a premultiplied dY.
Every launch goes through the C ABI between poisoned guards (edge_runs.guarded)."""
import pytest
import torch

from tests import exact_cases as XC
from tests import op_edge_cases as OE
from tests import scale_grad_ref as SR
from tests.edge_runs import (Out, carve, check_rule, dev_stack, diagnose, differing, grouped_call, grouped_table_grad_call,
                             guarded, offsets_tensor)
from tests.qgemm_cases import Carved, guard_bits
from tests.support import bits16, bits32, env, fp32_blas_reduction  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
SPLIT_SCRATCH, SPLIT_SMS = 1 << 24, 256             # test_scale_grad_gpu.test_split_and_unsplit_agree_and_repeat's


def stream(env):
    return torch.cuda.current_stream(env.dev).cuda_stream


def dense_layer(env, lay):
    """One layer on the device, built once per module."""
    return dev_stack(env, OE.as_stack(lay))


def dtype_id(T):
    return 0 if T == F16 else 1


# ---- dequantize --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,bits,tile_p", OE.dequant_params())
def test_dequantize_range_edges(env, kind, bits, tile_p):
    c = OE.dequant_case(kind, bits, tile_p)
    lay, st = c.lay, dense_layer(env, c.lay)
    S, t2 = (Carved(t, env.dev, guard_bits(t, F16)) for t in (lay.S, lay.table2))
    out = Out(env, (lay.N, lay.K), F16)
    args = (0, bits, lay.g, lay.N, lay.K, st.Q.shape[1], 0, lay.K, st.Q[0].data_ptr(), S.t.data_ptr(), t2.t.data_ptr(),
            out.t.data_ptr(), st.tid, stream(env))
    W = guarded(env, env.lib.flute_dequantize, args, [S, t2], [out], nan_expected=True)[0].cpu()
    assert not torch.isnan(W).any()
    if not torch.equal(bits16(W), bits16(c.want)):
        w = lay.w_exact().T
        alt = [("subnormals flushed", XC.flush_subnormal_f16(w)), ("saturates at 65504", w.clamp(-XC.FP16_MAX, XC.FP16_MAX))]
        raise AssertionError((kind, bits, tile_p, int((bits16(W) != bits16(c.want)).sum()), diagnose(W, F16, alt)))


# ---- the scale gradients -------------------------------------------------------------------------------------------------

def scale_grad_abi(env, lay, dY, X, split=False, nan_expected=False):
    """flute_qgemm_scale_grad with dY, X and dS between guards; split: with the scratch that splits M in two."""
    st = dense_layer(env, lay)
    T, (M, N), K = lay.dtype, dY.shape, X.shape[1]
    cy, cx = carve(env, dY, T), carve(env, X, T)
    out = Out(env, (N, K // lay.g), T)
    scratch = torch.empty(SPLIT_SCRATCH, dtype=torch.uint8, device=env.dev) if split else None
    if split:
        assert OE.sg_splits(M, N, K, lay.g, SPLIT_SMS, SPLIT_SCRATCH)[0] >= 2
    args = (dtype_id(T), lay.bits, lay.g, M, N, K, st.Q.shape[1], st.tid, cy.t.data_ptr(), cx.t.data_ptr(), st.Q[0].data_ptr(),
            st.t2[0].data_ptr(), out.t.data_ptr(), scratch.data_ptr() if split else None, SPLIT_SCRATCH if split else 0,
            SPLIT_SMS, stream(env))
    return guarded(env, env.lib.flute_qgemm_scale_grad, args, [cy, cx], [out], nan_expected)[0]


def grouped_scale_grad(env, layers, counts, dY, X, rw=None, nan_expected=False):
    st = dev_stack(env, layers)
    K, N = X.shape[1], dY.shape[1]
    return grouped_call(env, "qgemm_grouped_scale_grad", st, (dY.shape[0],), N, (dY, X, offsets_tensor(counts), st.Q, st.t2, rw),
                        (len(counts), N, K // st.g), nan_expected)


def sg_alternatives(dY, X, L, g):
    f = XC.flush_subnormal_f16
    R = SR.scale_grad(dY, X, L, g)
    return [("subnormal dY flushed", SR.scale_grad(f(dY.double()), X, L, g)), ("subnormal X flushed", SR.scale_grad(dY, f(X.double()), L, g)),
            ("saturates at 65504", R.clamp(-XC.FP16_MAX, XC.FP16_MAX))]


@pytest.mark.parametrize("kind,bits,g", OE.sg_range_params())
def test_scale_grad_range_edges(env, kind, bits, g):
    """Dense: round_T(fp64) by value unsplit, the same bits through the fp32 scratch of a split M.  Grouped: the same kinds over
    counts [0, 31, 33, 0, 64, 5], round_T(fp64) by value and per expert the dense op's bits on that expert's rows."""
    c = OE.sg_dense_case(kind, bits, g)
    unsplit = scale_grad_abi(env, c.lay, c.dY, c.X)
    assert XC.exact_equal(unsplit, c.R, F16), (differing(unsplit, c.R, F16),
                                               diagnose(unsplit, F16, sg_alternatives(c.dY, c.X, OE.lut(c.lay), g)))
    split = scale_grad_abi(env, c.lay, c.dY, c.X, split=True)
    assert torch.equal(bits16(split), bits16(unsplit)), int((bits16(split) != bits16(unsplit)).sum())
    gc = OE.sg_grouped_case(kind, bits, g)
    dS = grouped_scale_grad(env, gc.layers, gc.counts, gc.dY, gc.X)
    st = dev_stack(env, gc.layers)
    off = OE.offsets_list(gc.counts)
    for e, n in enumerate(gc.counts):
        if not n:
            assert torch.all(bits16(dS[e]) == 0), e
            continue
        assert XC.exact_equal(dS[e], gc.R[e], F16), (e, differing(dS[e], gc.R[e], F16))
        sl = slice(off[e], off[e + 1])
        dense = env.fa.qgemm_scale_grad(gc.dY[sl].to(env.dev), gc.X[sl].to(env.dev), st.Q[e], st.t2[e], bits, g, st.tid)
        assert torch.equal(bits16(dS[e]), bits16(dense)), e


@pytest.mark.parametrize("bits,g", OE.SG_CASES)
def test_grouped_scale_grad_row_weight_range_edges(env, bits, g):
    """round_T(row_weight dY) subnormal on some rows and +-inf on one: bit for bit the unweighted launch on the premultiplied dY."""
    c = OE.sg_row_weight_case(bits, g)
    weighted = grouped_scale_grad(env, c.layers, c.counts, c.dY, c.X, rw=c.rw, nan_expected=True)
    pre = grouped_scale_grad(env, c.layers, c.counts, c.pre, c.X, nan_expected=True)
    assert XC.nonfinite_equal(weighted, pre)
    e_big = OE.expert_of_row(c.counts, c.r_big)
    for e, n in enumerate(c.counts):
        assert torch.isfinite(weighted[e]).all() == (e != e_big), e
        assert bool(weighted[e].any()) == (n > 0)


@pytest.mark.parametrize("bits,g,dtype", OE.sg_nonfinite_params())
def test_scale_grad_nonfinite_dense(env, bits, g, dtype):
    """Rows 31 | 32, the two sides of a 32-row step, unsplit; through the scratch the two rows on either side of the split; in
    both the last two rows, the Inf in the very last one, in front of the masked rows of the last step."""
    c = OE.sg_nonfinite_dense_case(bits, g, dtype)
    lay, L = c.lay, OE.lut(c.lay)
    clean = scale_grad_abi(env, lay, c.dY, c.X)
    assert XC.exact_equal(clean, SR.scale_grad(c.dY, c.X, L, g), dtype)
    assert torch.equal(bits16(scale_grad_abi(env, lay, c.dY, c.X, split=True)), bits16(clean))
    splits, sps = OE.sg_splits(c.M, lay.N, lay.K, g, SPLIT_SMS, SPLIT_SCRATCH)
    cut = 32 * sps
    assert splits >= 2 and 0 < cut < c.M
    for split, launches in ((False, c.unsplit + c.tail), (True, OE.mreduce_launches(cut - 1, cut, lay.K, lay.N, g) + c.tail)):
        for name, xs, ys in launches:
            dYp, Xp = OE.poison(c.dY, ys), OE.poison(c.X, xs)
            D = scale_grad_abi(env, lay, dYp, Xp, split=split, nan_expected=True)
            check_rule(D, OE.scale_grad_expected(clean, dYp, Xp, L, g), (bits, g, dtype, "split" if split else "unsplit", name))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("bits,g,dtype", OE.sg_nonfinite_params())
def test_scale_grad_nonfinite_grouped(env, bits, g, dtype, weighted):
    """NaN in the last row of expert 1, Inf in the first row of expert 2: their dS by rule, experts 4 and 5 bit for bit the
    clean launch, the empty experts zeros."""
    c = OE.sg_nonfinite_grouped_case(bits, g, dtype, weighted)
    clean = grouped_scale_grad(env, c.layers, c.counts, c.dY, c.X, rw=c.rw)
    off = OE.offsets_list(c.counts)
    for name, xs, ys in c.launches:
        dYp, Xp = OE.poison(c.dY, ys), OE.poison(c.X, xs)
        D = grouped_scale_grad(env, c.layers, c.counts, dYp, Xp, rw=c.rw, nan_expected=True)
        dYw = OE.premultiplied(dYp, c.rw)
        for e, n in enumerate(c.counts):
            sl = slice(off[e], off[e + 1])
            if not n:
                assert torch.all(bits16(D[e]) == 0), (name, e)
            elif e in c.touched:
                exp = OE.scale_grad_expected(clean[e], dYw[sl], Xp[sl], OE.lut(c.layers[e]), g)
                assert not torch.isfinite(exp).all()
                check_rule(D[e], exp, (bits, g, dtype, weighted, name, e))
            else:
                assert torch.equal(bits16(D[e]), bits16(clean[e])), (name, e)


def table_grad_abi(env, lay, dY, X, nan_expected=False):
    """flute_qgemm_table_grad with the fused dS: dY, X, S and both outputs between guards."""
    st = dense_layer(env, lay)
    T, (M, N), K = lay.dtype, dY.shape, X.shape[1]
    cy, cx, cs = carve(env, dY, T), carve(env, X, T), carve(env, lay.S, T)
    n = 2 ** lay.bits
    dT2, dS = Out(env, (n * n, 2), torch.float32), Out(env, (N, K // lay.g), T)
    nbytes = env.lib.flute_qgemm_table_grad_scratch_bytes(lay.bits, lay.g, M, N, K, 1, env.num_sms)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=env.dev)
    args = (dtype_id(T), lay.bits, lay.g, M, N, K, st.Q.shape[1], st.tid, cy.t.data_ptr(), cx.t.data_ptr(), st.Q[0].data_ptr(),
            cs.t.data_ptr(), st.t2[0].data_ptr(), dT2.t.data_ptr(), dS.t.data_ptr(), scratch.data_ptr(), nbytes, env.num_sms,
            stream(env))
    return guarded(env, env.lib.flute_qgemm_table_grad, args, [cy, cx, cs], [dT2, dS], nan_expected)


def equal_with_nans(a, b):
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0).view(torch.int32), b.masked_fill(nb, 0).view(torch.int32))


@pytest.mark.parametrize("bits,g,dtype", OE.sg_nonfinite_params())
def test_table_grad_nonfinite(env, bits, g, dtype):
    """dT2 by the bin rule against the clean launch's bits; the fused dS bit for bit qgemm_scale_grad's on the same data."""
    c = OE.tg_nonfinite_case(bits, g, dtype)
    lay, st = c.lay, dense_layer(env, c.lay)
    clean, clean_dS = table_grad_abi(env, lay, c.dY, c.X)
    assert torch.isfinite(clean).all() and torch.isfinite(clean_dS).all()
    for name, xs, ys in c.launches:
        dYp, Xp = OE.poison(c.dY, ys), OE.poison(c.X, xs)
        dT2, dS = table_grad_abi(env, lay, dYp, Xp, nan_expected=True)
        exp = OE.table_grad_expected(clean, dYp, Xp, lay.W, lay.S, bits, g)
        assert equal_with_nans(dT2, exp), (bits, g, dtype, name, (~torch.isfinite(dT2.cpu())).nonzero().tolist()[:10],
                                           (~torch.isfinite(exp)).nonzero().tolist()[:10])
        ref = env.fa.qgemm_scale_grad(dYp.to(env.dev), Xp.to(env.dev), st.Q[0], st.t2[0], bits, g, st.tid)
        assert XC.nonfinite_equal(dS, ref), name
        check_rule(dS, OE.scale_grad_expected(clean_dS, dYp, Xp, OE.lut(lay), g), (bits, g, dtype, name, "fused dS"))


@pytest.mark.parametrize("kind,bits,g", OE.tg_range_params())
def test_table_grad_range_edges(env, kind, bits, g):
    """dY or X is j 2^-20, all of it fp16-subnormal: every partial sum of every bin is exact in fp32 (op_edge_cases.tg_exact),
    so dT2 equals the fp64 sum by value, and the by-product dS round_T of its fp64 sum - dense over 259 rows and grouped over
    counts [0, 31, 33, 0, 64, 5].  A kernel that flushes the subnormal operand returns zeros."""
    c = OE.tg_range_case(kind, bits, g, grouped=False)
    dT2, dS = table_grad_abi(env, c.lay, c.dY, c.X)
    assert torch.equal(dT2.double().cpu(), c.RT), (kind, bits, g, int((dT2.double().cpu() != c.RT).sum()),
                                                   "all zeros: the subnormal operand was flushed" if not dT2.any() else "")
    assert XC.exact_equal(dS, c.R, F16), differing(dS, c.R, F16)
    gc = OE.tg_range_case(kind, bits, g, grouped=True)
    dT2, dS = grouped_table_grad(env, gc.layers, gc.counts, gc.dY, gc.X)
    for e, n in enumerate(gc.counts):
        if not n:
            assert torch.all(bits32(dT2[e]) == 0) and torch.all(bits16(dS[e]) == 0), e
            continue
        assert torch.equal(dT2[e].double().cpu(), gc.RT[e]), (kind, bits, g, e, int((dT2[e].double().cpu() != gc.RT[e]).sum()),
                                                              "all zeros: the subnormal operand was flushed" if not dT2[e].any() else "")
        assert XC.exact_equal(dS[e], gc.R[e], F16), (e, differing(dS[e], gc.R[e], F16))


def grouped_table_grad(env, layers, counts, dY, X, rw=None, nan_expected=False):
    return grouped_table_grad_call(env, dev_stack(env, layers), counts, dY, X, rw, nan_expected)


def check_expert_by_rule(c, e, dT2, dS, clean, clean_s, dYw, Xp, what):
    """Expert e of a grouped table-gradient launch on (dYw, Xp) - dYw the premultiplied dY - by the dense rules on its rows."""
    off = OE.offsets_list(c.counts)
    sl, lay = slice(off[e], off[e + 1]), c.layers[e]
    exp = OE.table_grad_expected(clean[e], dYw[sl], Xp[sl], lay.W, lay.S, lay.bits, lay.g)
    assert not torch.isfinite(exp).all()
    assert equal_with_nans(dT2[e], exp), (what, e, (~torch.isfinite(dT2[e].cpu())).nonzero().tolist()[:10],
                                          (~torch.isfinite(exp)).nonzero().tolist()[:10])
    exp_s = OE.scale_grad_expected(clean_s[e], dYw[sl], Xp[sl], OE.lut(lay), lay.g)
    assert not torch.isfinite(exp_s).all()
    check_rule(dS[e], exp_s, (what, e, "fused dS"))


@pytest.mark.parametrize("bits,g,dtype,weighted", OE.tg_nonfinite_grouped_params())
def test_table_grad_nonfinite_grouped(env, bits, g, dtype, weighted):
    """NaN in the last row of expert 1, Inf in the first row of expert 2, then the other way round - the Inf in a last row
    is what a tail masked by `clamp to the last row and multiply by zero` turns into NaN: the two experts' dT2 and dS by the
    dense rules on their own rows, experts 4 and 5 bit for bit the clean launch, the empty experts zeros; the fused dS has
    the bits of flute_qgemm_grouped_scale_grad on the same operands."""
    c = OE.tg_nonfinite_grouped_case(bits, g, dtype, weighted)
    clean, clean_s = grouped_table_grad(env, c.layers, c.counts, c.dY, c.X, rw=c.rw)
    assert torch.isfinite(clean).all() and torch.isfinite(clean_s).all()
    for name, xs, ys in c.launches:
        dYp, Xp = OE.poison(c.dY, ys), OE.poison(c.X, xs)
        dT2, dS = grouped_table_grad(env, c.layers, c.counts, dYp, Xp, rw=c.rw, nan_expected=True)
        dYw = OE.premultiplied(dYp, c.rw)
        for e, n in enumerate(c.counts):
            if not n:
                assert torch.all(bits32(dT2[e]) == 0) and torch.all(bits16(dS[e]) == 0), (name, e)
            elif e in c.touched:
                check_expert_by_rule(c, e, dT2, dS, clean, clean_s, dYw, Xp, (bits, g, dtype, weighted, name))
            else:
                assert torch.equal(bits32(dT2[e]), bits32(clean[e])) and torch.equal(bits16(dS[e]), bits16(clean_s[e])), (name, e)
        alone = grouped_scale_grad(env, c.layers, c.counts, dYp, Xp, rw=c.rw, nan_expected=True)
        assert XC.nonfinite_equal(dS, alone), name


@pytest.mark.parametrize("bits,g", OE.SG_CASES)
def test_grouped_table_grad_row_weight_range_edges(env, bits, g):
    """round_T(row_weight dY) subnormal on some rows and +-inf on one: bit for bit the unweighted launch on the premultiplied
    dY; the expert that owns the overflowing row by the rules on the premultiplied dY, from the clean bits of a launch on the
    premultiplied dY with the infinite entries zero; every other expert that launch's bits."""
    c = OE.tg_row_weight_case(bits, g)
    weighted = grouped_table_grad(env, c.layers, c.counts, c.dY, c.X, rw=c.rw, nan_expected=True)
    pre = grouped_table_grad(env, c.layers, c.counts, c.pre, c.X, nan_expected=True)
    clean, clean_s = grouped_table_grad(env, c.layers, c.counts, c.pre_finite, c.X, nan_expected=True)
    assert equal_with_nans(weighted[0], pre[0]) and XC.nonfinite_equal(weighted[1], pre[1])
    assert torch.isfinite(clean).all() and not torch.isnan(clean_s).any()
    dT2, dS = weighted
    for e, n in enumerate(c.counts):
        if e == c.e_big:
            check_expert_by_rule(c, e, dT2, dS, clean, clean_s, c.pre, c.X, (bits, g, "row weight"))
        else:
            assert torch.equal(bits32(dT2[e]), bits32(clean[e])) and torch.equal(bits16(dS[e]), bits16(clean_s[e])), e
            assert bool(dT2[e].any()) == (n > 0)


# ---- moe_combine ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16])
def test_moe_combine_nonfinite(env, dtype):
    """A NaN in a served row reaches its token's row in its column; +Inf and -Inf in two slots of one token give NaN there;
    what the rows no expert served hold stays out; every other element has the clean launch's bits."""
    c = OE.combine_case(dtype)

    def run(Y, nan_expected):
        cy, cp, co = carve(env, Y, dtype), carve(env, c.pos, dtype), carve(env, c.offsets, dtype)
        out = Out(env, (c.T, c.N), dtype)
        args = (dtype_id(dtype), c.T, c.k, c.E, c.N, cy.t.data_ptr(), cp.t.data_ptr(), co.t.data_ptr(), out.t.data_ptr(), stream(env))
        return guarded(env, env.lib.flute_moe_combine, args, [cy, cp, co], [out], nan_expected)[0]

    Yclean = c.Y.clone()
    Yclean[c.served:] = float("nan")                       # rows no expert served: never read
    clean = run(Yclean, False)
    assert torch.equal(bits16(clean.cpu()), bits16(OE.combine_ieee(c, c.Y)))
    check_rule(run(c.Yp, True), OE.combine_expected(clean, c), dtype)


# ---- the dense qgemm backward: dequantize plus mm --------------------------------------------------------------------------

def qgemm_backward(env, lay, dY):
    st = dense_layer(env, lay)
    d = env.dev
    x = torch.zeros(dY.shape[0], lay.K, dtype=lay.dtype, device=d, requires_grad=True)
    with fp32_blas_reduction():
        y = env.fa.qgemm(x, st.Q[0], st.S[0], lay.table.to(d), st.t2[0], env.ws, lay.bits, lay.g, st.tid, env.num_sms)
        y.backward(dY.to(d))
    return x.grad.cpu()


def test_qgemm_backward_subnormal_weights(env):
    lay = XC.Layer(4, OE.K_EDGE, 3 * 128, 64, F16, XC.seed_of("dense backward subw"), **XC.SUBW)
    dY = XC.make_x(40, lay.N, lay.seed + 1, F16, witness=False)
    R, A = OE.grad_exact([lay], [40], dY)
    OE.grad_premise("subw", dY, lay, A)
    assert XC.is_subnormal_f16(R.to(F16).double()).any()
    D = qgemm_backward(env, lay, dY)
    assert XC.exact_equal(D, R, F16), (differing(D, R, F16), diagnose(D, F16, [
        ("subnormal w flushed", OE.grad_exact([lay], [40], dY, flush_w=True)[0])]))


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_qgemm_backward_nonfinite_rows(env, dtype):
    lay = XC.Layer(4, OE.K_EDGE, 3 * 128, 64, dtype, XC.seed_of("dense backward nonfinite", dtype))
    M, N = 40, lay.N
    dY = XC.make_x(M, N, lay.seed + 1, dtype, witness=False)
    clean = qgemm_backward(env, lay, dY)
    assert XC.exact_equal(clean, OE.grad_exact([lay], [M], dY)[0], dtype)
    for r_nan, r_inf, n_nan, n_inf in ((15, 16, 3, 6), (31, 32, N - 2, N - 5)):
        D = qgemm_backward(env, lay, XC.poison_x(dY, r_nan, r_inf, n_nan, n_inf))
        exp = OE.rowwise_expected(clean, [(r_nan, None), (r_inf, torch.sign(lay.w_exact()[:, n_inf]))])
        check_rule(D, exp, (dtype, r_nan, r_inf))
