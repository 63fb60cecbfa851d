"""The block forms of the grouped forward (qgemm_grouped_blocks.h) and of the grouped input gradient
(qgemm_grouped_input_grad_blocks.h) on hostile operands: the block variants of tests/op_edge_cases.py, at shapes only these
forms serve - counts [0, 1, 127, 128, 129, 0, 259, 5], N a multiple of 256, K of eight groups (forward) or two 256-k blocks
(gradient) - and every launch names its form: a shape the form does not serve is refused, never answered by the row or
slab form.

Range edges have one allowed answer, round_T of the fp64 result by value: fp16-subnormal weights and row operands are
multiplied as they are, a result past 65520 is +-inf and not 65504, also where only the row weight takes it there, and the
pair form's two overflowing halves cancel to exactly zero in the one fp32 accumulator.  Non-finite launches follow by rule
from the bits of the clean launch: the NaN row is NaN, the Inf row +-inf by the sign of the weight it meets (a zero row
weight: NaN), every other row is untouched - the last valid row of a ragged block and the first row of the next expert,
which follows it directly in memory, included.  The block forms read a block's rows past its expert's end as zeros and
never store them; a mask by multiplication, or a tile staged from the neighbour's rows, would leak exactly here.  The
gradient's block form promises the slab form's bits on all inputs: every launch is repeated on the slab form.

Every launch goes through the C ABI between poisoned guards (edge_runs.guarded)."""
import pytest
import torch

from tests import exact_cases as XC
from tests import op_edge_cases as OE
from tests.edge_runs import (FORWARD_FORM_BLOCKS, GRAD_FORM_BLOCKS, GRAD_FORM_SLABS, check_rule, diagnose, differing,
                             forward_alternatives, grad_alternatives, grad_reference, run_forward, run_grad)
from tests.support import bits16, env  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_SHAPE = -4                                  # include/flute_amd.h FLUTE_ERR_SHAPE


# ---- the forms are named, and a named form does not fall back ---------------------------------------------------------------

def test_a_named_form_refuses_what_it_does_not_serve(env):
    """The shapes of the row- and slab-form cases: the block forms refuse them before anything is enqueued."""
    c = OE.forward_range_case("plain", "subx", 4, 32)
    assert not OE.forward_blocks_eligible(c.bits, c.g, c.K, c.N)
    with pytest.raises(AssertionError, match=str(ERR_SHAPE)):
        run_forward(env, c, c.X, form=FORWARD_FORM_BLOCKS)
    c = OE.grad_range_case("single", "subx", 4, 32)
    assert not OE.grad_blocks_eligible(c.bits, c.K)
    with pytest.raises(AssertionError, match=str(ERR_SHAPE)):
        run_grad(env, c, c.dY, c.dY2, form=GRAD_FORM_BLOCKS)


# ---- the grouped forward, block form --------------------------------------------------------------------------------------

def forward_blocks(env, c, X, nan_expected=False, counts=None):
    return run_forward(env, c, X, nan_expected, FORWARD_FORM_BLOCKS, counts)


@pytest.mark.parametrize("op,kind,bits,tile_p,g", OE.block_forward_range_params())
def test_forward_blocks_range_edges(env, op, kind, bits, tile_p, g):
    c = OE.forward_range_case(op, kind, bits, tile_p, g, block=True)
    D = forward_blocks(env, c, c.X)
    if not XC.exact_equal(D, c.R, c.dtype):
        raise AssertionError((op, kind, bits, tile_p, g, differing(D, c.R, c.dtype), diagnose(D, c.dtype, forward_alternatives(c))))


@pytest.mark.parametrize("bits,tile_p", OE.block_pushed_params())
def test_forward_blocks_row_weight_alone_overflows(env, bits, tile_p):
    """The unweighted result is finite: the power-of-two row weight pushes row a to +inf and, negated, row b to -inf."""
    c = OE.weighted_pushed_case(bits, tile_p, block=True)
    D = forward_blocks(env, c, c.X).cpu()
    assert XC.exact_equal(D, c.R, c.dtype), (differing(D, c.R, c.dtype),
                                             diagnose(D, c.dtype, [("saturates at 65504", c.R.clamp(-XC.FP16_MAX, XC.FP16_MAX))]))
    assert (D[c.a] == OE.INF).any() and torch.equal(D[c.b].double(), -D[c.a].double())


@pytest.mark.parametrize("op,bits,tile_p,g,dtype", OE.block_forward_nonfinite_params())
def test_forward_blocks_nonfinite(env, op, bits, tile_p, g, dtype):
    c = OE.forward_nonfinite_case(op, bits, tile_p, g, dtype, block=True)
    clean = forward_blocks(env, c, c.X)
    R = OE.forward_exact(c.layers, c.counts, c.X)[0]
    assert XC.exact_equal(clean, R if c.rw is None else R * c.rw.double()[:, None], dtype)
    for la in c.launches:
        D = forward_blocks(env, c, la.X, nan_expected=True)
        check_rule(D, OE.rowwise_expected(clean, la.poisons), (op, bits, tile_p, g, dtype, la.name))
    if op == "weighted":
        # the zero fill: a table that ends before the last expert leaves its rows unserved; the weighted launch writes them as
        # zeros whatever they hold (a NaN and an Inf here), and the rows that are served keep the clean launch's bits
        counts = c.counts[:-1] + [0]
        served = sum(counts)
        X = XC.poison_x(c.X, served, served + 1, 3, 6)
        D = forward_blocks(env, c, X, counts=counts)
        assert served < D.shape[0] and torch.all(bits16(D[served:]) == 0)
        assert torch.equal(bits16(D[:served]), bits16(clean[:served]))


# ---- the grouped input gradient, block form ---------------------------------------------------------------------------------

def grad_both_forms(env, c, dY, dY2, what, nan_expected=False):
    """The block form's result, after asserting that the slab form returns the same bits on the same operands."""
    B = run_grad(env, c, dY, dY2, nan_expected, GRAD_FORM_BLOCKS)
    S = run_grad(env, c, dY, dY2, nan_expected, GRAD_FORM_SLABS)
    check_rule(B, S.cpu(), ("blocks against slabs",) + tuple(what))
    return B


@pytest.mark.parametrize("form,kind,bits,tile_p,g", OE.block_grad_range_params())
def test_input_grad_blocks_range_edges(env, form, kind, bits, tile_p, g):
    c = OE.grad_range_case(form, kind, bits, tile_p, g, block=True)
    D = grad_both_forms(env, c, c.dY, c.dY2, (form, kind, bits, tile_p, g))
    if not XC.exact_equal(D, c.R, c.dtype):
        raise AssertionError((form, kind, bits, tile_p, g, differing(D, c.R, c.dtype), diagnose(D, c.dtype, grad_alternatives(c))))
    if form == "pair" and kind == "overflow":              # two halves that would each overflow alone: exactly zero
        off = OE.offsets_list(c.counts)
        for e in c.big:
            assert not D[off[e]:off[e] + 2].any() and torch.isinf(D[off[e] + 3:off[e] + 5]).any(), e


@pytest.mark.parametrize("form,bits,tile_p,g,dtype", OE.block_grad_nonfinite_params())
def test_input_grad_blocks_nonfinite(env, form, bits, tile_p, g, dtype):
    c = OE.grad_nonfinite_case(form, bits, tile_p, g, dtype, block=True)
    what = (form, bits, tile_p, g, dtype)
    clean = grad_both_forms(env, c, c.dY, c.dY2, what + ("clean",))
    assert XC.exact_equal(clean, grad_reference(c), dtype)
    for la in c.launches:
        D = grad_both_forms(env, c, la.dY, la.dY2, what + (la.name,), nan_expected=True)
        check_rule(D, OE.rowwise_expected(clean, la.poisons), what + (la.name,))
