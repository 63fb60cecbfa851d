"""The premises of the long-row GPU tests (tests/test_grouped_long_rows_gpu.py, tests/test_row_stream_long_rows_gpu.py) without
a GPU: the constants of tests/long_rows_cases.py, the two row tables, the checkers on CPU tensors, and what the library's host-side rules say at K = 7168 on
both sides of T_EDGE and TSRC_EDGE and at R_LONG - the form queries, and the `_ex` / block entries asked with null pointers
(a shape is refused before a pointer is looked at, so FLUTE_ERR_NULL means "served" and FLUTE_ERR_SHAPE "not served")."""
import pytest
import torch

from flute_amd import _lib, dev
from tests import long_rows_cases as LC
from tests.support import first_template

ERR_SHAPE, ERR_NULL = -4, -9
AUTO, ROWS, BLOCKS = 0, 1, 2
PLAIN, WEIGHTED = 0, 2
K = LC.K
SHAPES = [(4, 0), (4, 1), (2, 0)]                  # (bits, dtype id) of the GPU cases: 4-bit fp16 / bf16, 2-bit fp16


def test_constants_and_tables():
    LC.check_constants()
    assert (LC.ROW_2G, LC.ROW_4G, LC.T_EDGE, LC.TSRC_EDGE, LC.R_LONG) == (149796, 299593, 299337, 299593, 300000)
    for T in (LC.T_EDGE, LC.T_EDGE + 1, LC.R_LONG):
        fat, spread = LC.fat_counts(T), LC.spread_counts(T)
        assert len(fat) == 3 and len(spread) == 8 and spread.count(0) == 1
        off = LC.served_offsets(spread)
        assert any(o * LC.ROW_BYTES > 1 << 31 for o in off[:-1])
        assert any(o * LC.ROW_BYTES > 1 << 32 for o in off[:-1]) == (T == LC.R_LONG)
        assert LC.served_offsets(spread, T - 300)[-1] == T - 300
    # the fat expert's relative offsets reach the descriptor limit: its last block's idle rows end below 2^32 - 16, within four
    # blocks of it
    rows = LC.fat_counts(LC.T_EDGE)[1]
    assert (rows + 127) * LC.ROW_BYTES < LC.LIMIT < (rows + 127 + 4 * 128) * LC.ROW_BYTES
    b = LC.bands(LC.R_LONG)
    assert b[:64] == list(range(64)) and b[-64:] == list(range(LC.R_LONG - 64, LC.R_LONG))
    assert {LC.ROW_2G - 1, LC.ROW_2G, LC.ROW_2G + 1, LC.ROW_4G - 1, LC.ROW_4G, LC.ROW_4G + 1} <= set(b)
    assert LC.ROW_4G not in LC.bands(LC.TSRC_EDGE) and LC.ROW_4G - 1 in LC.bands(LC.TSRC_EDGE)
    assert len(LC.bands(LC.R_LONG, 3000, 1)) > 3000 and LC.bands(LC.R_LONG, 3000, 1) == LC.bands(LC.R_LONG, 3000, 1)


def test_the_checkers_see_one_wrong_element():
    """The guarded buffer and the row comparisons on CPU tensors: one element in the last row, one word in a guard band, one
    unwritten element and one -0 where +0 bits are owed each fail their check, and nothing else does."""
    rows, cols, dtype = 2 * LC.ROWS + 3, 8, LC.F16
    out = LC.Guarded((rows, cols), dtype, "cpu")
    out.assert_untouched()
    out.assert_unwritten(0, rows)
    R = torch.arange(rows * cols, dtype=torch.float32).remainder(7).view(rows, cols).to(dtype)
    out.out.copy_(R)
    out.assert_guards(), out.assert_written(), LC.assert_equal_rows(out.out, R, "same"), LC.assert_equal_bits(out.out, R, "same")
    with pytest.raises(AssertionError):
        out.assert_untouched()
    out.out[-1, -1] += 1
    with pytest.raises(pytest.fail.Exception, match="last row %d" % (rows - 1)):
        LC.assert_equal_rows(out.out, R, "one element")
    LC.assert_equal_rows(out.out, R, "the rows before it", 0, rows - 1)
    with pytest.raises(AssertionError):
        LC.assert_equal_bits(out.out, R, "one element")
    out.ints()[-1, -1] = out.canary
    with pytest.raises(AssertionError):
        out.assert_written()
    out.assert_written(0, rows - 1)
    out.out[-2:] = 0
    out.assert_zero_bits(rows - 2)
    out.out[-1, 0] = -0.0
    with pytest.raises(AssertionError):
        out.assert_zero_bits(rows - 2)
    for i in (0, LC.GUARD - 1, -LC.GUARD, -1):
        out.buf[i] = 0
        with pytest.raises(AssertionError):
            out.assert_guards()
        out.buf[i] = out.canary
    out.assert_guards()
    w = LC.Guarded((5,), torch.float32, "cpu")
    assert w.buf.dtype == torch.int32 and torch.isnan(w.out).all()
    before = LC.snapshot(R, None)
    LC.assert_unchanged(before, R, None)
    R[-1, -1] = -R[-1, -1]
    with pytest.raises(AssertionError):
        LC.assert_unchanged(before, R, None)


@pytest.mark.parametrize("bits,dtype", SHAPES)
@pytest.mark.parametrize("mode", [PLAIN, WEIGHTED])
def test_forward_forms_on_both_sides_of_t_edge(bits, dtype, mode):
    lib, tid = _lib.get(), first_template(bits, 32)
    N = 256
    P = bits * N // 16
    entry = lib.flute_qgemm_grouped_ex if mode == PLAIN else lib.flute_qgemm_grouped_weighted_ex
    nptr = 6 if mode == PLAIN else 7
    for E in (3, 8):
        form = lambda T: lib.flute_qgemm_grouped_form(mode, dtype, bits, 64, E, T, N, K, tid, 256)
        forced = lambda T, f: entry(dtype, bits, 64, E, T, N, K, P, tid, *(None,) * nptr, 256, None, f)
        assert form(LC.T_EDGE) == BLOCKS and forced(LC.T_EDGE, BLOCKS) == ERR_NULL
        for T in (LC.T_EDGE + 1, LC.R_LONG):
            assert form(T) == ROWS
            assert forced(T, BLOCKS) == ERR_SHAPE
            assert forced(T, ROWS) == ERR_NULL and forced(T, AUTO) == ERR_NULL
    name = {PLAIN: "plain", WEIGHTED: "weighted"}[mode]
    dt = {0: LC.F16, 1: LC.BF16}[dtype]
    assert dev.grouped_form(name, 8, LC.T_EDGE, N, K, bits, 64, tid, 256, dt) == "blocks"
    assert dev.grouped_form(name, 8, LC.T_EDGE + 1, N, K, bits, 64, tid, 256, dt) == "rows"


@pytest.mark.parametrize("bits,dtype", SHAPES)
def test_glu_blocks_on_both_sides_of_tsrc_edge(bits, dtype):
    lib, tid = _lib.get(), first_template(bits, 32)
    F, E, R = 256, 7, 4096
    P = bits * F // 16
    asked = lambda R, Tsrc, rows: lib.flute_qgemm_grouped_glu_blocks(dtype, bits, 64, E, R, Tsrc, F, K, P, tid, None, rows,
                                                                     *(None,) * 8, 0, None)
    assert asked(R, LC.TSRC_EDGE, 1) == ERR_NULL
    assert asked(R, LC.TSRC_EDGE + 1, 1) == ERR_SHAPE and asked(R, LC.R_LONG, 1) == ERR_SHAPE
    assert asked(LC.TSRC_EDGE, LC.TSRC_EDGE, None) == ERR_NULL                # rows = None: R = Tsrc
    assert asked(LC.TSRC_EDGE + 1, LC.TSRC_EDGE + 1, None) == ERR_SHAPE
    # the row form serves every one of them
    for Tsrc in (LC.TSRC_EDGE, LC.TSRC_EDGE + 1, LC.R_LONG):
        assert lib.flute_qgemm_grouped_glu_ex(dtype, bits, 64, E, R, Tsrc, F, K, P, tid, None, 1, *(None,) * 8, 256, None,
                                              ROWS) == ERR_NULL                # (`rows` is compared with null only)
    dt = {0: LC.F16, 1: LC.BF16}[dtype]
    assert dev.grouped_glu_blocks_form(E, R, LC.TSRC_EDGE, F, K, bits, 64, tid, 256, dt) == "blocks"
    assert dev.grouped_glu_blocks_form(E, R, LC.TSRC_EDGE + 1, F, K, bits, 64, tid, 256, dt) == "rows"


@pytest.mark.parametrize("bits,dtype", SHAPES)
def test_input_grad_forms_have_no_row_limit_here(bits, dtype):
    """Every base of the input gradient's block form is 64-bit and it builds no descriptor: it serves all five row counts."""
    lib, tid = _lib.get(), first_template(bits, 32)
    N = 16 * 16 // bits * 2                       # one column block of the layout at TileP 32: 128 / 256
    P = bits * N // 16
    dt = {0: LC.F16, 1: LC.BF16}[dtype]
    for R in (LC.T_EDGE, LC.T_EDGE + 1, LC.TSRC_EDGE, LC.TSRC_EDGE + 1, LC.R_LONG):
        for E in (3, 8):
            assert dev.grouped_input_grad_form(E, R, N, K, bits, 64, tid, 256, dt) == "blocks"
            for form in (AUTO, 1, BLOCKS):
                assert lib.flute_qgemm_grouped_input_grad_ex(dtype, bits, 64, E, R, N, K, P, tid, *(None,) * 11, 256, None,
                                                             form) == ERR_NULL
