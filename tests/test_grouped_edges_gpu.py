"""The grouped forward (Plain, Weighted, Glu) and the grouped input gradient (single, pair, row-weighted) on hostile
operands (tests/op_edge_cases.py): fp16-subnormal weights, a subnormal row operand, results that overflow fp16 in both
directions, the GLU outside |g| <= 88, and one NaN and one +Inf on the two sides of a seam between two experts.

Range edges have one allowed answer, round_T of the fp64 result by value, infinities included.  Non-finite launches follow
by rule from the bits of the same launch on the unpoisoned operands: the NaN row is NaN, the Inf row is +-inf by the sign
of the weight it meets, every other row - the neighbour across the seam, in the same 16-row tile, included - is untouched.
These kernels mask out-of-range rows by not loading them; a mask by multiplication would leak exactly here.

Every launch goes through the C ABI with the output and every row operand (X / dY / dY2 / row_weight / rows / offsets) in
the middle of poisoned buffers: afterwards the guards are intact, the inputs unmodified and (clean launches) no canary is
left in the rows the op promises to write."""
import pytest
import torch

from tests import exact_cases as XC
from tests import op_edge_cases as OE
from tests.edge_runs import (check_rule, diagnose, differing, forward_alternatives, grad_alternatives, grad_reference,
                             run_forward, run_grad)
from tests.grouped_cases import assert_glu
from tests.support import env  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16


# ---- the grouped forward -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op,kind,bits,tile_p,g", OE.forward_range_params())
def test_forward_range_edges(env, op, kind, bits, tile_p, g):
    c = OE.forward_range_case(op, kind, bits, tile_p, g)
    D = run_forward(env, c, c.X)
    if not XC.exact_equal(D, c.R, c.dtype):
        raise AssertionError((op, kind, bits, tile_p, g, differing(D, c.R, c.dtype), diagnose(D, c.dtype, forward_alternatives(c))))


@pytest.mark.parametrize("bits,tile_p", OE.pushed_params())
def test_weighted_row_weight_alone_overflows(env, bits, tile_p):
    """The unweighted result is finite: the power-of-two row weight pushes row a to +inf and, negated, row b to -inf."""
    c = OE.weighted_pushed_case(bits, tile_p)
    D = run_forward(env, c, c.X).cpu()
    assert XC.exact_equal(D, c.R, c.dtype), (differing(D, c.R, c.dtype),
                                             diagnose(D, c.dtype, [("saturates at 65504", c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX))]))
    assert (D[c.a] == OE.INF).any() and torch.equal(D[c.b].double(), -D[c.a].double())


@pytest.mark.parametrize("bits,tile_p,g,dtype,use_rows", OE.glu_saturation_params())
def test_glu_saturation(env, bits, tile_p, g, dtype, use_rows):
    """silu32(g) = g / (1 + expf(-g)) outside |g| <= 88.  g >= 18: 1 + expf(-g) is 1 in fp32 (e^-18 < 2^-25), so
    H = round_T(g u) exactly (the product is exact in fp32: op_edge_cases asserts |g u| < 2^18 in multiples of 2^-6).
    g <= -90: expf(-g) is +inf, H is zero by value.  -88 <= g < 18: grouped_cases.assert_glu's bound.  -90 < g < -88
    (expf near its overflow) is left out: a condition on g, at most 2 % of the case."""
    c = OE.glu_saturation_case(bits, tile_p, g, dtype, use_rows)
    H = run_forward(env, c, c.X, nan_expected=True).double().cpu()      # (nothing non-finite goes in: a NaN is a failure below)
    want_hi = c.P.to(dtype).double()
    bad_hi = int((H[c.hi] != want_hi[c.hi]).sum())
    bad_lo = int((H[c.lo] != 0).sum())
    print("glu saturation %s: %d elements g >= 18 (%d of them +-inf in T), %d with g <= -90, %d mid, sign_k %d; wrong: %d, %d; NaN %d"
          % ((bits, tile_p, g, dtype, use_rows), int(c.hi.sum()), int(torch.isinf(want_hi[c.hi]).sum()), int(c.lo.sum()),
             int(c.mid.sum()), c.sign_k, bad_hi, bad_lo, int(torch.isnan(H).sum())))
    assert bad_hi == 0, ("g >= 18: H != round_T(g u)", bad_hi, int(torch.isnan(H[c.hi]).sum()))
    assert bad_lo == 0, ("g <= -90: H != 0", bad_lo)
    assert_glu(H[c.mid], c.Eref[c.mid], dtype, ("mid range", bits, tile_p, g))


@pytest.mark.parametrize("op,bits,tile_p,g,dtype,use_rows", OE.forward_nonfinite_params())
def test_forward_nonfinite(env, op, bits, tile_p, g, dtype, use_rows):
    c = OE.forward_nonfinite_case(op, bits, tile_p, g, dtype, use_rows)
    clean = run_forward(env, c, c.X)
    assert torch.isfinite(clean).all()
    if op != "glu":
        R = OE.forward_exact(c.layers, c.counts, c.X)[0]
        assert XC.exact_equal(clean, R if c.rw is None else R * c.rw.double()[:, None], dtype)
    for la in c.launches:
        D = run_forward(env, c, la.X, nan_expected=True)
        check_rule(D, OE.rowwise_expected(clean, la.poisons), (op, bits, tile_p, g, dtype, use_rows, la.name))


# ---- the grouped input gradient ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,kind,bits,tile_p,g", OE.grad_range_params())
def test_input_grad_range_edges(env, form, kind, bits, tile_p, g):
    c = OE.grad_range_case(form, kind, bits, tile_p, g)
    D = run_grad(env, c, c.dY, c.dY2)
    if not XC.exact_equal(D, c.R, c.dtype):
        raise AssertionError((form, kind, bits, tile_p, g, differing(D, c.R, c.dtype), diagnose(D, c.dtype, grad_alternatives(c))))


@pytest.mark.parametrize("form,bits,tile_p,g,dtype", OE.grad_nonfinite_params())
def test_input_grad_nonfinite(env, form, bits, tile_p, g, dtype):
    c = OE.grad_nonfinite_case(form, bits, tile_p, g, dtype)
    clean = run_grad(env, c, c.dY, c.dY2)
    assert XC.exact_equal(clean, grad_reference(c), dtype)
    for la in c.launches:
        D = run_grad(env, c, la.dY, la.dY2, nan_expected=True)
        check_rule(D, OE.rowwise_expected(clean, la.poisons), (form, bits, tile_p, g, dtype, la.name))
