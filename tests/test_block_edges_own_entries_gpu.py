"""The block forms behind entries of their own on hostile operands: the 3-bit block form (qgemm_block3.h, GM = 1 / 2;
flute_qgemm_grouped_w3_blocks and flute_qgemm_grouped_weighted_w3_blocks) and the block form of the fused SwiGLU launch
(qgemm_block2.h, GM = 3; flute_qgemm_grouped_glu_blocks), on the block variants of tests/op_edge_cases.py: counts
[0, 1, 127, 128, 129, 0, 259, 5], K of eight groups (K = 4096 for the overflow kind), N = 512 at 3 bits and
F = max(256, column block) for the SwiGLU launch.  Every launch names its entry (edge_runs.FORWARD_FORM_W3_BLOCKS /
_GLU_BLOCKS) and goes through the C ABI between poisoned guards (edge_runs.guarded); an entry refuses what it does not serve.

3 bits: range edges have one allowed answer, round_T of the fp64 product by value - fp16-subnormal weights and activations
multiplied as they are, a sum past 65520 is +-inf and not 65504, also where only the row weight takes it there (the weighted
epilogue multiplies in fp32 and rounds once).  Non-finite launches follow by rule from the bits of the clean launch: the NaN row
is NaN, the Inf row +-inf by the sign of the weight it meets (a zero row weight: NaN), every other row untouched, the last
valid row of a ragged block and the first row of the next expert included.

SwiGLU: silu32(g) = g / (1 + expf(-g)) outside |g| <= 88 in the three classes of test_grouped_edges_gpu.test_glu_saturation,
and the non-finite rule - g = +inf gives +-inf by the sign of u, g = -inf or a zero weight NaN - on both sides of the seams,
with a row index and without."""
import pytest
import torch

from tests import exact_cases as XC
from tests import op_edge_cases as OE
from tests.edge_runs import (FORWARD_FORM_GLU_BLOCKS, FORWARD_FORM_W3_BLOCKS, check_rule, diagnose, differing,
                             forward_alternatives, run_forward)
from tests.grouped_cases import assert_glu
from tests.support import bits16, env  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_SHAPE = -4                                  # include/flute_amd.h FLUTE_ERR_SHAPE


def test_a_named_entry_refuses_what_it_does_not_serve(env):
    """The 3-bit entries refuse a 4-bit stack at a shape the 4-bit block form serves, and a 3-bit stack of five groups; the
    SwiGLU block entry refuses the row-form case's K = 320.  Nothing answers in their place."""
    for op in ("plain", "weighted"):
        c = OE.forward_range_case(op, "subx", 4, 32, block=True)
        assert OE.forward_blocks_eligible(c.bits, c.g, c.K, c.N) and not OE.w3_blocks_eligible(c.bits, c.g, c.K, c.N)
        with pytest.raises(AssertionError, match=str(ERR_SHAPE)):
            run_forward(env, c, c.X, form=FORWARD_FORM_W3_BLOCKS)
        c = OE.forward_range_case(op, "subx", 3, 32)
        assert not OE.w3_blocks_eligible(c.bits, c.g, c.K, c.N)
        with pytest.raises(AssertionError, match=str(ERR_SHAPE)):
            run_forward(env, c, c.X, form=FORWARD_FORM_W3_BLOCKS)
    c = OE.glu_saturation_case(4, 32, 64, torch.float16, False)
    assert not OE.glu_blocks_eligible(c.bits, c.g, c.K, c.N)
    with pytest.raises(AssertionError, match=str(ERR_SHAPE)):
        run_forward(env, c, c.X, form=FORWARD_FORM_GLU_BLOCKS)


# ---- 3 bits ---------------------------------------------------------------------------------------------------------------

def w3_blocks(env, c, X, nan_expected=False, counts=None):
    return run_forward(env, c, X, nan_expected, FORWARD_FORM_W3_BLOCKS, counts)


@pytest.mark.parametrize("op,kind,bits,tile_p,g", OE.w3_block_forward_range_params())
def test_w3_blocks_range_edges(env, op, kind, bits, tile_p, g):
    c = OE.forward_range_case(op, kind, bits, tile_p, g, block=True)
    D = w3_blocks(env, c, c.X)
    if not XC.exact_equal(D, c.R, c.dtype):
        raise AssertionError((op, kind, bits, tile_p, g, differing(D, c.R, c.dtype), diagnose(D, c.dtype, forward_alternatives(c))))


@pytest.mark.parametrize("bits,tile_p", OE.w3_block_pushed_params())
def test_w3_blocks_row_weight_alone_overflows(env, bits, tile_p):
    """The unweighted result is finite: the power-of-two row weight pushes row a to +inf exactly where round_T(w R) is and,
    negated, row b to -inf; everything else is finite and exact."""
    c = OE.weighted_pushed_case(bits, tile_p, block=True)
    D = w3_blocks(env, c, c.X).cpu()
    assert XC.exact_equal(D, c.R, c.dtype), (differing(D, c.R, c.dtype),
                                             diagnose(D, c.dtype, [("saturates at 65504", c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX))]))
    want = c.R.to(c.dtype)
    assert (D[c.a] == OE.INF).any() and torch.equal(D[c.a] == OE.INF, want[c.a] == OE.INF)
    assert torch.equal(D[c.b].double(), -D[c.a].double())
    rest = torch.ones(D.shape[0], dtype=torch.bool)
    rest[[c.a, c.b]] = False
    assert torch.isfinite(D[rest]).all()


@pytest.mark.parametrize("op,bits,tile_p,g,dtype", OE.w3_block_forward_nonfinite_params())
def test_w3_blocks_nonfinite(env, op, bits, tile_p, g, dtype):
    c = OE.forward_nonfinite_case(op, bits, tile_p, g, dtype, block=True)
    clean = w3_blocks(env, c, c.X)
    R = OE.forward_exact(c.layers, c.counts, c.X)[0]
    assert XC.exact_equal(clean, R if c.rw is None else R * c.rw.double()[:, None], dtype)
    for la in c.launches:
        D = w3_blocks(env, c, la.X, nan_expected=True)
        check_rule(D, OE.rowwise_expected(clean, la.poisons), (op, bits, tile_p, g, dtype, la.name))
    if op == "weighted":
        # the zero fill: a table that ends before the last expert leaves its rows unserved; the weighted launch writes them as
        # zeros whatever they hold (a NaN and an Inf here), and the rows that are served keep the clean launch's bits
        counts = c.counts[:-1] + [0]
        served = sum(counts)
        X = XC.poison_x(c.X, served, served + 1, 3, 6)
        D = w3_blocks(env, c, X, counts=counts)
        assert served < D.shape[0] and torch.all(bits16(D[served:]) == 0)
        assert torch.equal(bits16(D[:served]), bits16(clean[:served]))


# ---- the fused SwiGLU launch ------------------------------------------------------------------------------------------------

def glu_blocks(env, c, X, nan_expected=False):
    return run_forward(env, c, X, nan_expected, FORWARD_FORM_GLU_BLOCKS)


@pytest.mark.parametrize("bits,tile_p,g,dtype,use_rows", OE.glu_block_saturation_params())
def test_glu_blocks_saturation(env, bits, tile_p, g, dtype, use_rows):
    """test_grouped_edges_gpu.test_glu_saturation's three-way statement on the block launch.  g >= 18: 1 + expf(-g) is 1 in
    fp32, so H = round_T(g u) exactly (the product is exact in fp32: op_edge_cases asserts |g u| < 2^18 in multiples of 2^-6).
    g <= -90: expf(-g) is +inf, H is zero by value.  -88 <= g < 18: grouped_cases.assert_glu's bound.  -90 < g < -88 is left
    out: a condition on g, at most 2 % of the case (asserted where the case is built)."""
    c = OE.glu_saturation_case(bits, tile_p, g, dtype, use_rows, block=True)
    H = glu_blocks(env, c, c.X, nan_expected=True).double().cpu()      # (nothing non-finite goes in: a NaN is a failure below)
    want_hi = c.P.to(dtype).double()
    bad_hi = int((H[c.hi] != want_hi[c.hi]).sum())
    bad_lo = int((H[c.lo] != 0).sum())
    print("glu blocks saturation %s: %d elements g >= 18 (%d of them +-inf in T), %d with g <= -90, %d mid, sign_k %d; wrong: %d, %d; "
          "NaN %d" % ((bits, tile_p, g, dtype, use_rows), int(c.hi.sum()), int(torch.isinf(want_hi[c.hi]).sum()), int(c.lo.sum()),
                      int(c.mid.sum()), c.sign_k, bad_hi, bad_lo, int(torch.isnan(H).sum())))
    assert bad_hi == 0, ("g >= 18: H != round_T(g u)", bad_hi, int(torch.isnan(H[c.hi]).sum()))
    assert bad_lo == 0, ("g <= -90: H != 0", bad_lo)
    assert_glu(H[c.mid], c.Eref[c.mid], dtype, ("mid range", bits, tile_p, g))


@pytest.mark.parametrize("bits,tile_p,g,dtype,use_rows", OE.glu_block_nonfinite_params())
def test_glu_blocks_nonfinite(env, bits, tile_p, g, dtype, use_rows):
    c = OE.forward_nonfinite_case("glu", bits, tile_p, g, dtype, use_rows, block=True)
    clean = glu_blocks(env, c, c.X)
    assert torch.isfinite(clean).all()
    for la in c.launches:
        D = glu_blocks(env, c, la.X, nan_expected=True)
        check_rule(D, OE.rowwise_expected(clean, la.poisons), ("glu", bits, tile_p, g, dtype, use_rows, la.name))
