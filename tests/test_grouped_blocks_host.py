"""The block form of the grouped forward launches without a GPU: the form query, the `_ex` entries' refusals (returned
before anything is enqueued or dereferenced, on null pointers), the old entries unchanged, the Python `form` keyword, and
the bound on the row-block count the grid is sized by."""
import os
import random

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
AUTO, ROWS, BLOCKS = 0, 1, 2
PLAIN, GLU, WEIGHTED = 0, 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind


def template_or_zero(bits, tile_p):
    try:
        return first_template(bits, tile_p)
    except ValueError:       # no template has this bit width: the call is refused before the id is read
        return 0


def thresholds():
    """(mean rows per expert from which the rule takes the block form where E * (N / 256) fills the chip, ... where it does not)"""
    with open(HEADER) as f:
        d = dict(l.split()[1:3] for l in f if l.startswith("#define FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS"))
    return int(d["FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS"]), int(d["FLUTE_GROUPED_BLOCKS_MIN_MEAN_ROWS_PARTIAL"])


def query(mode=PLAIN, dtype=0, bits=4, g=64, E=8, rows=4096, N=1024, K=512, tid=None, num_sms=256):
    tid = template_or_zero(bits, 32) if tid is None else tid
    return _lib.get().flute_qgemm_grouped_form(mode, dtype, bits, g, E, rows, N, K, tid, num_sms)


def plain_ex(form, dtype=0, bits=4, g=64, E=8, T=4096, N=1024, K=512, P=None, tid=None, ptrs=(None,) * 6):
    tid = template_or_zero(bits, 32) if tid is None else tid
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_ex(dtype, bits, g, E, T, N, K, P, tid, *ptrs, 256, None, form)


def weighted_ex(form, dtype=0, bits=4, g=64, E=8, T=4096, N=1024, K=512, P=None, tid=None, ptrs=(None,) * 7):
    tid = template_or_zero(bits, 32) if tid is None else tid
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_weighted_ex(dtype, bits, g, E, T, N, K, P, tid, *ptrs, 256, None, form)


def glu_ex(form, dtype=0, bits=4, g=64, E=8, R=4096, Tsrc=4096, F=1024, K=512, tid=None, ptrs=(None,) * 10):
    tid = template_or_zero(bits, 32) if tid is None else tid
    return _lib.get().flute_qgemm_grouped_glu_ex(dtype, bits, g, E, R, Tsrc, F, K, bits * F // 16, tid, *ptrs, 256, None, form)


def test_symbols_declared():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_ex", "flute_qgemm_grouped_glu_ex", "flute_qgemm_grouped_weighted_ex",
                 "flute_qgemm_grouped_form"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "fast for\n * decode-sized ones" not in text
    full, partial = thresholds()
    assert 1 <= full <= partial


def test_query_rows_where_not_eligible():
    assert query() == BLOCKS                                               # the eligible shape the cases below vary
    assert query(bits=3, N=1024, rows=8192) == ROWS
    assert query(N=1024 + 128) == ROWS                                     # N % 256
    assert query(bits=2, N=1024 + 256) == BLOCKS and query(bits=2, N=1024 + 128, tid=template_or_zero(2, 32)) == ERR_SHAPE
    assert query(K=448, g=64) == ROWS                                      # (K / g) % 8 = 7
    assert query(K=256, g=64) == ROWS                                      # 4 groups
    assert query(K=256, g=32) == BLOCKS
    assert query(mode=GLU) == ROWS                                         # no block form of the GLU launch is built
    assert query(mode=WEIGHTED) == BLOCKS
    assert query(mode=3) == ERR_SHAPE
    assert query(dtype=1) == BLOCKS and query(dtype=2) == ERR_DTYPE
    assert query(bits=5) == ERR_NUM_BITS and query(g=48) == ERR_GROUP_SIZE
    # the 32-bit activation offsets: (T + 256) K 2 must stay below 2^32 - 16
    assert query(rows=2 ** 20, K=2048) == ROWS and query(rows=2 ** 20 - 512, K=2048) == BLOCKS


def test_query_threshold_on_mean_rows_per_expert():
    full, partial = thresholds()
    for E in (1, 8, 64):                                                   # N = 1024: 4 E workgroups with rows, 256 compute units
        thr = full if 4 * E >= 256 else partial
        assert query(E=E, rows=thr * E) == BLOCKS
        assert query(E=E, rows=thr * E - 1) == ROWS
        assert query(E=E, rows=1) == ROWS
    # the same stack on fewer compute units, and a wider one on the whole chip: the experts' column blocks fill it
    assert query(E=8, rows=full * 8, num_sms=32) == BLOCKS and query(E=8, rows=full * 8 - 1, num_sms=32) == ROWS
    assert query(E=8, N=8192, rows=full * 8) == BLOCKS and query(E=8, N=8192, rows=full * 8 - 1) == ROWS
    assert query(E=8, N=8192 - 256, rows=partial * 8) == BLOCKS and query(E=8, N=8192 - 256, rows=partial * 8 - 1) == ROWS
    assert query(E=8, rows=partial * 8, num_sms=0) == query(E=8, rows=partial * 8, num_sms=256)      # num_sms < 1: 256
    assert query(E=0) == ROWS and query(rows=0) == ROWS
    assert dev.grouped_form("plain", 8, partial * 8, 1024, 512, 4, 64, template_or_zero(4, 32), 256) == "blocks"
    assert dev.grouped_form("weighted", 8, partial * 8 - 1, 1024, 512, 4, 64, template_or_zero(4, 32), 256) == "rows"
    assert dev.grouped_form("glu", 8, 4096, 1024, 512, 4, 64, template_or_zero(4, 32)) == "rows"
    with pytest.raises(RuntimeError):
        dev.grouped_form("plain", 8, 4096, 1000, 512, 4, 64, template_or_zero(4, 32))


@pytest.mark.parametrize("call", [plain_ex, weighted_ex])
def test_forcing_blocks_where_not_eligible_is_refused_first(call):
    """FLUTE_ERR_SHAPE with null pointers: the refusal comes before the pointers are looked at."""
    assert call(BLOCKS, bits=3, tid=template_or_zero(3, 32)) == ERR_SHAPE
    assert call(BLOCKS, N=1024 + 128) == ERR_SHAPE
    assert call(BLOCKS, K=448) == ERR_SHAPE
    assert call(BLOCKS, T=2 ** 20, K=2048) == ERR_SHAPE
    assert call(BLOCKS, T=0) == ERR_SHAPE and call(BLOCKS, E=0) == ERR_SHAPE
    assert call(3) == ERR_SHAPE and call(-1) == ERR_SHAPE
    n = 6 if call is plain_ex else 7
    assert call(BLOCKS, N=1024 + 128, ptrs=(FAKE,) * n) == ERR_SHAPE
    # an eligible shape passes the form and reaches the null pointers, in every form; below the threshold too when forced
    for form in (AUTO, ROWS, BLOCKS):
        assert call(form) == ERR_NULL
    assert call(BLOCKS, T=5) == ERR_NULL
    # the old refusals come first, in their order
    assert call(BLOCKS, dtype=2, bits=5) == ERR_DTYPE
    assert call(BLOCKS, bits=5, g=48) == ERR_NUM_BITS
    assert call(BLOCKS, g=48) == ERR_GROUP_SIZE
    assert call(BLOCKS, P=255) == ERR_SHAPE and call(BLOCKS, E=-1) == ERR_SHAPE
    assert call(AUTO, T=0) == OK and call(ROWS, E=0) == OK


def test_glu_has_no_block_form():
    assert glu_ex(BLOCKS) == ERR_SHAPE
    assert glu_ex(BLOCKS, ptrs=(FAKE,) * 10) == ERR_SHAPE
    assert glu_ex(AUTO) == ERR_NULL and glu_ex(ROWS) == ERR_NULL
    assert glu_ex(AUTO, R=0, Tsrc=0) == OK
    assert glu_ex(BLOCKS, Tsrc=5) == ERR_SHAPE                            # (its own shape refusal comes first either way)
    assert glu_ex(4) == ERR_SHAPE


def test_old_entries_unchanged():
    """The old entry points are the `_ex` ones with the automatic form: the same refusals in the same order, on shapes on
    either side of the threshold."""
    lib = _lib.get()
    tid = template_or_zero(4, 32)
    for T in (8, 4096):
        for kw in (dict(), dict(dtype=2), dict(bits=5), dict(g=48), dict(N=1000), dict(K=480), dict(P=255), dict(E=-1),
                   dict(T=-1), dict(T=0), dict(E=0), dict(N=1024 + 128), dict(K=448)):
            a = dict(dtype=0, bits=4, g=64, E=8, T=T, N=1024, K=512)
            a.update(kw)
            P = kw.get("P", a["bits"] * a["N"] // 16)
            head = (a["dtype"], a["bits"], a["g"], a["E"], a["T"], a["N"], a["K"], P, tid)
            old = lib.flute_qgemm_grouped(*head, *(None,) * 6, 256, None)
            assert old == lib.flute_qgemm_grouped_ex(*head, *(None,) * 6, 256, None, AUTO), kw
            assert old == lib.flute_qgemm_grouped_ex(*head, *(None,) * 6, 256, None, ROWS), kw
            oldw = lib.flute_qgemm_grouped_weighted(*head, *(None,) * 7, 256, None)
            assert oldw == old == lib.flute_qgemm_grouped_weighted_ex(*head, *(None,) * 7, 256, None, AUTO), kw
    assert lib.flute_qgemm_grouped(2, 5, 64, 8, 8, 1024, 512, 256, tid, *(None,) * 6, 256, None) == ERR_DTYPE
    assert lib.flute_qgemm_grouped(0, 4, 64, 8, 8, 1024, 512, 256, tid, *(None,) * 6, 256, None) == ERR_NULL
    for i in range(6):
        ptrs = [FAKE] * 6
        ptrs[i] = None
        assert lib.flute_qgemm_grouped(0, 4, 64, 8, 4096, 1024, 512, 256, tid, *ptrs, 256, None) == ERR_NULL, i


def test_python_form_keyword_is_validated():
    E, K, N, bits, g = 2, 256, 256, 4, 32
    meta = lambda *s, dtype=torch.float16: torch.empty(s, dtype=dtype, device="meta")
    args = (meta(8, K), meta(E + 1, dtype=torch.int32), meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g),
            meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))
    for op, extra in ((flute_amd.qgemm_grouped, ()), (flute_amd.qgemm_grouped_weighted, (meta(8, dtype=torch.float32),))):
        with pytest.raises(ValueError, match="form"):
            op(*args, *extra, bits, g, template_or_zero(bits, 32), form="block")
    with pytest.raises(ValueError, match="form"):
        flute_amd.qgemm_grouped_glu(*args, *args[2:], bits, g, template_or_zero(bits, 32), form=2)


def row_blocks_bound(E, T):
    """The grid's row-block count: floor((T + 127 E) / 128), from T and E alone."""
    return (T + 127 * E) // 128


def test_row_block_bound_is_the_maximum_over_monotone_tables():
    """sum_e ceil(r_e / 128) over tables with sum r_e <= T never passes the bound, and a table reaches it: E - 1 experts with
    one row each (r = 1 mod 128 wastes 127 rows of a block) and the rest to the last - where T has a row for each of them."""
    rng = random.Random(7)
    for E, T in [(1, 1), (1, 128), (1, 129), (7, 685), (8, 4096), (64, 4096), (130, 258), (512, 3), (5, 0)] + \
                [(rng.randint(1, 600), rng.randint(0, 5000)) for _ in range(40)]:
        bound = row_blocks_bound(E, T)
        best = 0
        for _ in range(50):
            cuts = sorted(rng.randint(0, T) for _ in range(E))             # offsets[1 .. E], non-decreasing, offsets[E] <= T
            counts = [b - a for a, b in zip([0] + cuts[:-1], cuts)]
            total = sum(-(-r // 128) for r in counts)
            assert total <= bound, (E, T, counts)
            best = max(best, total)
        # the extremal table: as many experts as possible with r = 1 (mod 128)
        counts, left = [], T
        for e in range(E - 1):
            r = 1 if left >= 1 else 0
            counts.append(r)
            left -= r
        counts.append(left)
        reached = sum(-(-r // 128) for r in counts)
        if T >= E - 1:
            assert reached == bound, (E, T)                                # the bound is the maximum
        else:
            assert best <= reached == T <= bound, (E, T)                   # fewer rows than experts: every row its own block
