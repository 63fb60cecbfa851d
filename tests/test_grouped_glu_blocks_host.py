"""The block form of the fused SwiGLU grouped launch without a GPU (flute_qgemm_grouped_glu_blocks and its query): the symbols,
the query's eligibility list and thresholds, the launch's refusals in their order (returned before anything is enqueued or
dereferenced, on null and on fake pointers), and the Python keyword checks."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from flute_amd.integrations import moe
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
ROWS, BLOCKS = 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
NPTR = 10                # Xsrc, rows, offsets, three gate and three up operands, H
ROWS_PTR = 1             # `rows` among them: the one pointer that may be null


def template_or_zero(bits, tile_p):
    try:
        return first_template(bits, tile_p)
    except ValueError:       # no template has this bit width: the call is refused before the id is read
        return 0


def header_text():
    with open(HEADER) as f:
        return f.read()


def thresholds():
    d = dict(l.split()[1:3] for l in header_text().splitlines() if l.startswith("#define FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS"))
    return int(d["FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS"]), int(d["FLUTE_GROUPED_GLU_BLOCKS_MIN_MEAN_ROWS_PARTIAL"])


def query(dtype=0, bits=4, g=64, E=8, R=4096, Tsrc=None, F=1024, K=512, tid=None, num_sms=256):
    tid = template_or_zero(bits, 32) if tid is None else tid
    return _lib.get().flute_qgemm_grouped_glu_blocks_form(dtype, bits, g, E, R, R if Tsrc is None else Tsrc, F, K, tid, num_sms)


def launch(dtype=0, bits=4, g=64, E=8, R=4096, Tsrc=None, F=1024, K=512, P=None, tid=None, ptrs=(None,) * NPTR):
    tid = template_or_zero(bits, 32) if tid is None else tid
    P = bits * F // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_glu_blocks(dtype, bits, g, E, R, R if Tsrc is None else Tsrc, F, K, P, tid, *ptrs,
                                                     256, None)


# shapes the form does not serve: 3 bits, F % 256, (K / g) % 8, Tsrc * K * 2 past 2^32 - 16 (2^20 * 2048 * 2 = 2^32)
INELIGIBLE = [dict(bits=3, tid=template_or_zero(3, 32)), dict(F=1024 + 128), dict(K=448), dict(K=256),
              dict(R=2 ** 20, K=2048)]


def test_symbols_and_version():
    text = header_text()
    for name in ("flute_qgemm_grouped_glu_blocks", "flute_qgemm_grouped_glu_blocks_form"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9\n" in text and _lib.get().flute_abi_version() == 9
    full, partial = thresholds()
    assert 1 <= full <= partial


def test_query_eligibility():
    assert query() == BLOCKS                                               # the eligible shape the cases below vary
    for kw in INELIGIBLE:
        assert query(**kw) == ROWS, kw
    assert query(K=256, g=32) == BLOCKS and query(bits=2, F=1024 + 256) == BLOCKS and query(dtype=1) == BLOCKS
    # the descriptor spans Xsrc: Tsrc * K * 2 < 2^32 - 16 (a multiple of 128, so the last legal size is 2^32 - 128), whatever R
    assert query(R=2 ** 20, Tsrc=2 ** 20 - 1, K=2048) == BLOCKS
    assert query(R=2 ** 20 - 1, Tsrc=2 ** 20, K=2048) == ROWS
    assert query(R=2 ** 21, Tsrc=4096, K=2048) == BLOCKS                   # more sorted rows than (T + 256) K 2 lets the plain form take
    assert query(dtype=2) == ERR_DTYPE and query(bits=5) == ERR_NUM_BITS and query(g=48) == ERR_GROUP_SIZE
    assert query(F=1000) == ERR_SHAPE and query(E=-1) == ERR_SHAPE and query(R=-1) == ERR_SHAPE and query(Tsrc=-1) == ERR_SHAPE
    assert query(E=0) == ROWS and query(R=0) == ROWS
    # the existing query keeps its answer for the GLU mode
    assert _lib.get().flute_qgemm_grouped_form(1, 0, 4, 64, 8, 4096, 1024, 512, template_or_zero(4, 32), 256) == ROWS


def test_query_threshold_on_mean_rows_per_expert():
    full, partial = thresholds()
    for E in (1, 8, 64):                                                   # F = 1024: 4 E workgroups per row block, 256 compute units
        thr = full if 4 * E >= 256 else partial
        assert query(E=E, R=thr * E) == BLOCKS
        assert query(E=E, R=thr * E - 1) == ROWS
    assert query(E=8, F=8192, R=full * 8) == BLOCKS and query(E=8, F=8192, R=full * 8 - 1) == ROWS          # fills the chip
    assert query(E=8, F=8192 - 256, R=partial * 8) == BLOCKS and query(E=8, F=8192 - 256, R=partial * 8 - 1) == ROWS
    assert query(E=8, R=full * 8, num_sms=32) == BLOCKS and query(E=8, R=full * 8 - 1, num_sms=32) == ROWS
    for R in (partial * 8, partial * 8 - 1):                               # num_sms < 1: 256
        assert query(E=8, R=R, num_sms=0) == query(E=8, R=R, num_sms=256)
    tid = template_or_zero(4, 32)
    assert dev.grouped_glu_blocks_form(8, partial * 8, 100, 1024, 512, 4, 64, tid, 256) == "blocks"
    assert dev.grouped_glu_blocks_form(8, partial * 8 - 1, 100, 1024, 512, 4, 64, tid, 256) == "rows"
    assert dev.grouped_form("glu", 8, 4096, 1024, 512, 4, 64, tid) == "rows"
    with pytest.raises(RuntimeError):
        dev.grouped_glu_blocks_form(8, 4096, 4096, 1000, 512, 4, 64, tid)


def test_launch_refuses_ineligible_shapes_before_the_pointers():
    for kw in INELIGIBLE:
        assert launch(**kw) == ERR_SHAPE, kw
        assert launch(ptrs=(FAKE,) * NPTR, **kw) == ERR_SHAPE, kw
        assert launch(**{**kw, "E": 0}) == ERR_SHAPE, kw                   # before the empty-launch return
        if "R" not in kw:
            assert launch(**{**kw, "R": 0}) == ERR_SHAPE, kw
    assert launch(R=2 ** 20 - 1, Tsrc=2 ** 20, K=2048, ptrs=(FAKE,) * NPTR) == ERR_SHAPE


def test_launch_null_pointers_and_empty_launches():
    assert launch() == ERR_NULL
    for i in range(NPTR):
        ptrs = [FAKE] * NPTR
        ptrs[i] = None
        if i == ROWS_PTR:
            continue                                                       # null rows with Tsrc == R is a launch: not made here
        assert launch(ptrs=tuple(ptrs)) == ERR_NULL, i
    ptrs = [None] * NPTR
    ptrs[ROWS_PTR] = FAKE                                                  # rows alone is looked at for null, never behind
    assert launch(ptrs=tuple(ptrs), Tsrc=7) == ERR_NULL
    assert launch(E=0) == OK and launch(R=0) == OK
    assert launch(E=0, ptrs=(FAKE,) * NPTR) == OK and launch(R=0, Tsrc=5, ptrs=(FAKE,) * NPTR) == OK
    assert launch(R=5) == ERR_NULL                                         # below the query's threshold: still served


def test_launch_keeps_the_old_refusals_first():
    assert launch(dtype=2, bits=5) == ERR_DTYPE
    assert launch(bits=5, g=48) == ERR_NUM_BITS
    assert launch(g=48) == ERR_GROUP_SIZE
    assert launch(F=1000) == ERR_SHAPE and launch(K=480) == ERR_SHAPE
    assert launch(P=255) == ERR_SHAPE and launch(E=-1) == ERR_SHAPE and launch(R=-1) == ERR_SHAPE
    # the GLU-only refusals: a negative Tsrc, Tsrc != R without rows, Tsrc == 0 with rows and R > 0
    assert launch(Tsrc=-1) == ERR_SHAPE and launch(Tsrc=5) == ERR_SHAPE
    ptrs = [None] * NPTR
    ptrs[ROWS_PTR] = FAKE
    assert launch(Tsrc=0, ptrs=tuple(ptrs)) == ERR_SHAPE
    assert launch(dtype=2, F=1024 + 128) == ERR_DTYPE                      # ... all of them before the eligibility
    # the same calls on the row form's entry answer the same wherever both refuse
    lib, tid = _lib.get(), template_or_zero(4, 32)
    for kw in (dict(dtype=2), dict(bits=5), dict(g=48), dict(F=1000), dict(P=255), dict(E=-1), dict(Tsrc=5)):
        a = dict(dtype=0, bits=4, g=64, E=8, R=4096, Tsrc=4096, F=1024, K=512)
        a.update({k: v for k, v in kw.items() if k != "P"})
        P = kw.get("P", a["bits"] * a["F"] // 16)
        old = lib.flute_qgemm_grouped_glu(a["dtype"], a["bits"], a["g"], a["E"], a["R"], a["Tsrc"], a["F"], a["K"], P, tid,
                                          *(None,) * NPTR, 256, None)
        assert old == launch(**kw) < 0, kw


def meta_args(E=2, K=256, F=256, bits=4, g=32, T=8):
    meta = lambda *s, dtype=torch.float16: torch.empty(s, dtype=dtype, device="meta")
    stack = (meta(E, bits * F // 16, K, dtype=torch.int16), meta(E, F, K // g), meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))
    return (meta(T, K), meta(E + 1, dtype=torch.int32)) + stack + stack + (bits, g, template_or_zero(bits, 32))


def test_python_op_refuses_an_ineligible_shape_before_a_launch():
    assert flute_amd.qgemm_grouped_glu_blocks is flute_amd.ops.qgemm_grouped_glu_blocks
    with pytest.raises(ValueError, match="not eligible"):
        flute_amd.qgemm_grouped_glu_blocks(*meta_args(F=128))              # F % 256
    with pytest.raises(ValueError, match="not eligible"):
        flute_amd.qgemm_grouped_glu_blocks(*meta_args(K=256, g=64))        # 4 scale groups
    with pytest.raises(ValueError, match="not eligible"):
        flute_amd.qgemm_grouped_glu_blocks(*meta_args(bits=3))
    # an eligible shape passes the check and stops where the launch needs a GPU tensor
    with pytest.raises(RuntimeError, match="same GPU"):
        flute_amd.qgemm_grouped_glu_blocks(*meta_args())
    with pytest.raises(TypeError):
        flute_amd.qgemm_grouped_glu_blocks(*meta_args(), form="blocks")    # the op has no `form`
    with pytest.raises(ValueError, match="form"):
        flute_amd.qgemm_grouped_glu(*meta_args(), form="glu_blocks")       # ... and the old op's `form` did not grow a value


def test_flute_experts_validates_glu_blocks():
    E, K, F, bits, g = 2, 256, 256, 4, 32
    tid = template_or_zero(bits, 32)
    stack = lambda kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, tid, torch.device("cpu"), torch.float16)
    gate, up, down = stack(K, F), stack(K, F), stack(F, K)
    assert moe.FluteExperts(gate, up, down, fused=True).glu_blocks is False
    for value in (False, True, "auto"):
        assert moe.FluteExperts(gate, up, down, fused=True, glu_blocks=value).glu_blocks is value
    for value in ("blocks", 1, 0, None, "rows"):
        with pytest.raises(ValueError, match="glu_blocks"):
            moe.FluteExperts(gate, up, down, fused=True, glu_blocks=value)
    for value in (True, "auto"):
        with pytest.raises(ValueError, match="fused=True"):
            moe.FluteExperts(gate, up, down, fused=False, glu_blocks=value)
    assert moe.FluteExperts(gate, up, down, fused=False, glu_blocks=False).glu_blocks is False
    experts = moe.FluteExperts(gate, up, down, fused=True, native_routing=True, glu_blocks="auto")
    assert moe.FluteSparseMoeBlock(torch.zeros(E, K), experts, top_k=1).experts.glu_blocks == "auto"   # the block runs the experts as built
    # "auto" is decided from the shapes alone, no tensor is read
    assert experts._takes_glu_blocks(torch.empty(300, K, dtype=torch.float16, device="meta"), 300, 256) is True
    assert experts._takes_glu_blocks(torch.empty(60, K, dtype=torch.float16, device="meta"), 60, 256) is False
