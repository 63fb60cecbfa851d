"""The two forms of the grouped input gradient without a GPU: the exports, the host-only form query
(flute_qgemm_grouped_input_grad_form) and its rule, every refusal of flute_qgemm_grouped_input_grad_ex - returned before
anything is enqueued, on null or host pointers - the old entry as the automatic form, and the Python `form` keyword."""
import os
import re

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
AUTO, SLABS, BLOCKS = 0, 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
BASE = dict(dtype=0, bits=4, g=64, E=8, R=4096, N=1024, K=512, tid=0)


def header():
    with open(HEADER) as f:
        return f.read()


def thresholds():
    """The header's two constants: where one row block per expert fills the chip, and where it does not."""
    get = lambda name: int(re.search(r"#define %s (\d+)\b" % name, header()).group(1))
    return get("FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS"), get("FLUTE_GROUPED_INPUT_GRAD_BLOCKS_MIN_MEAN_ROWS_PARTIAL")


def min_mean(E, K, num_sms):
    """The rule's threshold, restated: E * (K / 256) workgroups against the compute units; num_sms < 1 means 256."""
    full, partial = thresholds()
    return full if E * (K // 256) >= (num_sms if num_sms >= 1 else 256) else partial


def query(pair=0, num_sms=256, **kw):
    a = dict(BASE, **kw)
    return _lib.get().flute_qgemm_grouped_input_grad_form(pair, a["dtype"], a["bits"], a["g"], a["E"], a["R"], a["N"], a["K"],
                                                          a["tid"], num_sms)


def ex(form, ptrs=(None,) * 11, P=None, num_sms=256, **kw):
    """ptrs: dY, offsets, Q, S, QM2, row_weight, dY2, Q2, S2, QM22, dX"""
    a = dict(BASE, **kw)
    P = a["bits"] * a["N"] // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_input_grad_ex(a["dtype"], a["bits"], a["g"], a["E"], a["R"], a["N"], a["K"], P,
                                                        a["tid"], *ptrs, num_sms, None, form)


def old(ptrs=(None,) * 11, P=None, num_sms=256, **kw):
    a = dict(BASE, **kw)
    P = a["bits"] * a["N"] // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_input_grad(a["dtype"], a["bits"], a["g"], a["E"], a["R"], a["N"], a["K"], P,
                                                     a["tid"], *ptrs, num_sms, None)


SINGLE = [FAKE] * 5 + [None] * 5 + [FAKE]
PAIR = [FAKE] * 5 + [None] + [FAKE] * 5
# shapes the block form does not serve: 3 bits, K no multiple of 256, no expert, no row
INELIGIBLE = [dict(bits=3, tid=first_template(3, 32)), dict(K=640), dict(K=128), dict(E=0), dict(R=0)]


def test_symbols_declared_abi_unchanged():
    text = header()
    for name in ("flute_qgemm_grouped_input_grad_ex", "flute_qgemm_grouped_input_grad_form"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    full, partial = thresholds()
    assert 1 <= full <= partial
    assert flute_amd.dev.grouped_input_grad_form is dev.grouped_input_grad_form


def test_form_query():
    assert query() == BLOCKS
    assert query(bits=3, tid=first_template(3, 32)) == SLABS
    assert query(K=640) == SLABS
    assert query(dtype=1) == BLOCKS
    assert query(bits=2, tid=first_template(2, 64)) == BLOCKS
    assert query(dtype=2) == ERR_DTYPE
    assert query(bits=5) == ERR_NUM_BITS
    assert query(g=48) == ERR_GROUP_SIZE
    assert query(dtype=2, bits=5, g=48) == ERR_DTYPE                    # the old order: dtype, the layer, the group size
    assert query(bits=5, g=48) == ERR_NUM_BITS
    assert query(tid=10 ** 6) == ERR_TEMPLATE_ID
    assert query(N=1000) == ERR_SHAPE and query(K=480) == ERR_SHAPE and query(E=-1) == ERR_SHAPE and query(R=-1) == ERR_SHAPE
    assert query(E=0) == SLABS and query(R=0) == SLABS
    # the pair form is eligible where the single form is
    for kw in (dict(), dict(dtype=1), dict(K=640), dict(bits=3, tid=first_template(3, 32)), dict(R=8), dict(E=0)):
        assert query(pair=1, **kw) == query(pair=0, **kw), kw


def test_form_rule_on_both_sides_of_the_threshold():
    """Shapes alone: blocks from a mean row count per expert on - the header's first constant where E * (K / 256) workgroups
    fill the chip, its second where they do not; num_sms < 1 means 256."""
    kinds = set()
    for E in (1, 8, 64):
        for K in (512, 8192):
            for sms in (256, 0, -3, 8, 304):
                t = min_mean(E, K, sms)
                kinds.add(t)
                assert query(E=E, R=t * E, K=K, num_sms=sms) == BLOCKS, (E, K, sms)
                assert query(E=E, R=t * E - 1, K=K, num_sms=sms) == SLABS, (E, K, sms)
            for R in (1, 31 * E, 32 * E, 127 * E, 128 * E, 1000 * E):
                assert query(E=E, R=R, K=K, num_sms=0) == query(E=E, R=R, K=K, num_sms=256) == query(E=E, R=R, K=K, num_sms=-1)
        assert query(E=E, R=1000 * E, K=640) == SLABS                  # ineligible on either side
    assert kinds == set(thresholds())                                  # both kinds of shape were met
    assert min_mean(8, 8192, 256) == thresholds()[0] and min_mean(8, 512, 256) == thresholds()[1]
    t = min_mean(8, 512, 256)
    assert dev.grouped_input_grad_form(8, 8 * t, 1024, 512, 4, 64, 0) == "blocks"
    assert dev.grouped_input_grad_form(8, 8 * t - 1, 1024, 512, 4, 64, 0) == "slabs"


def test_forced_blocks_refused_where_not_eligible():
    for kw in INELIGIBLE:
        assert ex(BLOCKS, **kw) == ERR_SHAPE, kw                        # before "nothing to do" and the null pointers
        assert ex(BLOCKS, ptrs=SINGLE, **kw) == ERR_SHAPE, kw           # ... and before any pointer is looked at
        assert ex(BLOCKS, ptrs=PAIR, **kw) == ERR_SHAPE, kw
    for form in (3, -1, 100):
        assert ex(form) == ERR_SHAPE and ex(form, ptrs=SINGLE) == ERR_SHAPE and ex(form, R=0) == ERR_SHAPE
    # the old refusals come first
    assert ex(BLOCKS, dtype=2, K=640) == ERR_DTYPE
    assert ex(BLOCKS, bits=5) == ERR_NUM_BITS
    assert ex(BLOCKS, g=48) == ERR_GROUP_SIZE
    assert ex(3, P=255) == ERR_SHAPE
    # slabs and automatic keep the old answers there
    assert ex(SLABS, R=0) == OK and ex(AUTO, R=0) == OK
    assert ex(SLABS, K=640) == ERR_NULL and ex(AUTO, K=640) == ERR_NULL


def test_eligible_shapes_reach_the_null_check_in_all_forms():
    for form in (AUTO, SLABS, BLOCKS):
        assert ex(form) == ERR_NULL, form
        assert ex(form, dtype=1) == ERR_NULL
        assert ex(form, R=5) == ERR_NULL, form                          # blocks forced below the threshold: served
        for i in (0, 1, 2, 3, 4, 10):
            ptrs = list(SINGLE)
            ptrs[i] = None
            assert ex(form, ptrs=ptrs) == ERR_NULL, (form, i)
        for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):                       # the pair form given in part
            ptrs = list(PAIR)
            ptrs[i] = None
            assert ex(form, ptrs=ptrs) == ERR_NULL, (form, i)
        # a row weight together with a pointer of the pair form is refused first, as in the old entry
        for i in range(6, 10):
            ptrs = [FAKE] * 6 + [None] * 4 + [FAKE]
            ptrs[i] = FAKE
            assert ex(form, ptrs=ptrs) == ERR_SHAPE, (form, i)
            assert ex(form, R=0, ptrs=ptrs) == ERR_SHAPE, (form, i)


def test_old_entry_is_the_automatic_form():
    """The shapes and refusals of test_grouped_input_grad_host.py's test_layer_and_shape_refusals_with_null_pointers, at its
    own base shape (E 4, R 8) and at this module's."""
    cases = [dict(), dict(dtype=2), dict(bits=5), dict(g=0), dict(g=16), dict(g=48), dict(g=512), dict(tid=10 ** 6),
             dict(bits=3, tid=first_template(3, 64), N=512), dict(dtype=2, bits=5), dict(N=1000),
             dict(tid=first_template(4, 64), N=128), dict(K=480), dict(K=384, g=256), dict(P=255), dict(E=-1), dict(R=-1),
             dict(R=0), dict(E=0)]
    want = [ERR_NULL, ERR_DTYPE, ERR_NUM_BITS] + [ERR_GROUP_SIZE] * 4 + [ERR_TEMPLATE_ID] * 2 + [ERR_DTYPE] + \
        [ERR_SHAPE] * 7 + [OK, ERR_NULL]
    for base in (dict(E=4, R=8), dict()):
        for kw, w in zip(cases, want):
            kw = dict(base, **kw)
            assert old(**kw) == ex(AUTO, **kw) == w, kw
            if w != ERR_NULL:                                           # (a refusal or nothing to do: no pointer is looked behind)
                assert old(ptrs=SINGLE, **kw) == ex(AUTO, ptrs=SINGLE, **kw) == w, kw


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_python_form_keyword():
    E, K, N, bits, g = 4, 512, 1024, 4, 64
    w = (meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g), meta(E, 16, 16, 1, dtype=torch.float32))
    dy, off = meta(8, N), meta(E + 1, dtype=torch.int32)
    for form in ("rows", "block", 2, "", "Blocks"):
        with pytest.raises(ValueError, match="form"):
            flute_amd.qgemm_grouped_input_grad(dy, off, *w, bits, g, 0, form=form)
    for form in (None, "slabs", "blocks"):                              # valid: on to the device check
        with pytest.raises(RuntimeError, match="GPU"):
            flute_amd.qgemm_grouped_input_grad(dy, off, *w, bits, g, 0, form=form)
    with pytest.raises(ValueError):                                     # the shapes are validated whatever the form
        flute_amd.qgemm_grouped_input_grad(meta(8, 512), off, *w, bits, g, 0, form="blocks")


def test_dev_form_agrees_with_the_query():
    name = {SLABS: "slabs", BLOCKS: "blocks"}
    t = min_mean(64, 512, 256)
    for kw in (dict(), dict(K=640), dict(dtype=1), dict(R=8), dict(E=64, R=64 * t), dict(E=64, R=64 * t - 1),
               dict(K=8192, R=8 * 32), dict(K=8192, R=8 * 32 - 1),
               dict(bits=2, tid=first_template(2, 32)), dict(bits=3, tid=first_template(3, 32)), dict(g=128, K=1024)):
        a = dict(BASE, **kw)
        dtype = torch.float16 if a["dtype"] == 0 else torch.bfloat16
        for pair in (False, True):
            got = dev.grouped_input_grad_form(a["E"], a["R"], a["N"], a["K"], a["bits"], a["g"], a["tid"], 256, dtype, pair=pair)
            assert got == name[query(pair=int(pair), **kw)], kw
    with pytest.raises(RuntimeError):
        dev.grouped_input_grad_form(8, 4096, 1024, 512, 5, 64, 0)
