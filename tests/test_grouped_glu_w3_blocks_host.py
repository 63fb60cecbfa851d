"""The 3-bit block form of the fused SwiGLU grouped launch without a GPU (flute_qgemm_grouped_glu_w3_blocks and its query): what the
entry refuses, the empty launch, the query's flip at the two header constants, and FluteExperts' keyword checks."""
import os

import pytest
import torch

from flute_amd import _lib, dev
from flute_amd.integrations import moe
from tests.support import first_template

OK, ERR_SHAPE, ERR_NULL = 0, -4, -9
ROWS, BLOCKS = 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
LIMIT = 2 ** 32 - 16


def tid_of(bits):
    return first_template(bits, 32)


def thresholds():
    with open(HEADER) as f:
        d = dict(l.split()[1:3] for l in f if l.startswith("#define FLUTE_GROUPED_GLU_W3_BLOCKS_MIN_MEAN_ROWS"))
    return int(d["FLUTE_GROUPED_GLU_W3_BLOCKS_MIN_MEAN_ROWS"]), int(d["FLUTE_GROUPED_GLU_W3_BLOCKS_MIN_MEAN_ROWS_PARTIAL"])


def launch(dtype=0, bits=3, g=64, E=8, R=4096, Tsrc=None, F=1024, K=512, ptrs=None):
    return _lib.get().flute_qgemm_grouped_glu_w3_blocks(dtype, bits, g, E, R, R if Tsrc is None else Tsrc, F, K, bits * F // 16,
                                                        tid_of(bits), *((ptrs,) * 10), 256, None)


def query(bits=3, g=64, E=8, R=4096, F=1024, K=512, num_sms=256):
    return _lib.get().flute_qgemm_grouped_glu_w3_blocks_form(0, bits, g, E, R, R, F, K, tid_of(bits), num_sms)


# Tsrc K 2 and one expert's packed bytes 3 (F / 16) K 2 on both sides of 2^32 - 16
ACT_IN, ACT_OUT = dict(R=4096, Tsrc=2 ** 20 - 1, K=2048), dict(R=4096, Tsrc=2 ** 20, K=2048)
PACKED_IN, PACKED_OUT = dict(F=65536, K=341 * 512), dict(F=65536, K=342 * 512)


@pytest.mark.parametrize("kw", [dict(bits=4), dict(bits=2), dict(F=1024 + 128), dict(K=448), ACT_OUT, PACKED_OUT])
def test_entry_refuses_before_the_pointers(kw):
    assert (3 * (65536 // 16)) * PACKED_IN["K"] * 2 < LIMIT <= (3 * (65536 // 16)) * PACKED_OUT["K"] * 2
    assert ACT_IN["Tsrc"] * 2048 * 2 < LIMIT <= ACT_OUT["Tsrc"] * 2048 * 2
    for ptrs in (None, FAKE):
        assert launch(ptrs=ptrs, **kw) == ERR_SHAPE
    assert launch(**{**kw, "E": 0}) == ERR_SHAPE                           # before the empty-launch return


def test_served_layers_and_empty_launches():
    assert "int flute_qgemm_grouped_glu_w3_blocks(" in open(HEADER).read()
    for kw in (dict(), dict(dtype=1), dict(K=256, g=32), dict(R=5), PACKED_IN):
        assert launch(**kw) == ERR_NULL, kw
    rows_only = (None, FAKE) + (None,) * 8                                 # Tsrc != R needs `rows`, compared with null only
    assert _lib.get().flute_qgemm_grouped_glu_w3_blocks(0, 3, 64, 8, 4096, ACT_IN["Tsrc"], 1024, 2048, 192, tid_of(3), *rows_only,
                                                        256, None) == ERR_NULL
    assert launch(E=0) == OK and launch(R=0) == OK and launch(E=0, ptrs=FAKE) == OK and launch(R=0, ptrs=FAKE) == OK


def test_query_flips_at_the_header_constants():
    full, partial = thresholds()
    assert 1 <= full and 1 <= partial
    for E, F in ((64, 1024), (8, 8192), (8, 8192 - 512), (1, 1024)):       # E (F / 256) against 256 compute units
        thr = full if E * (F // 256) >= 256 else partial
        assert query(E=E, F=F, R=thr * E) == BLOCKS and query(E=E, F=F, R=thr * E - 1) == ROWS
    assert query(E=8, R=full * 8, num_sms=32) == BLOCKS and query(E=8, R=full * 8 - 1, num_sms=32) == ROWS
    assert query(bits=4) == ERR_SHAPE and query(E=0) == ROWS and query(K=448) == ROWS
    big = max(full, partial) * 8
    assert dev.grouped_glu_w3_blocks_form(8, big, 100, 1024, 512, 64, tid_of(3)) == "blocks"
    assert dev.grouped_glu_w3_blocks_form(8, min(full, partial) * 8 - 1, 100, 1024, 512, 64, tid_of(3), 256, torch.bfloat16) == "rows"


def test_flute_experts_validates_w3_glu_blocks():
    E, K, F, g = 2, 512, 512, 32
    stack = lambda bits, kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, tid_of(bits), torch.device("cpu"), torch.float16)
    gate, up, down = stack(3, K, F), stack(3, K, F), stack(3, F, K)
    assert moe.FluteExperts(gate, up, down, fused=True).w3_glu_blocks is False
    for value in (False, True, "auto"):
        assert moe.FluteExperts(gate, up, stack(4, F, K), fused=True, w3_glu_blocks=value).w3_glu_blocks is value
    for value in ("maybe", "blocks", 1, None):
        with pytest.raises(ValueError, match="w3_glu_blocks"):
            moe.FluteExperts(gate, up, down, fused=True, w3_glu_blocks=value)
    for value in (True, "auto"):
        with pytest.raises(ValueError, match="fused=True"):
            moe.FluteExperts(gate, up, down, w3_glu_blocks=value)
        with pytest.raises(ValueError, match="3-bit"):
            moe.FluteExperts(stack(4, K, F), stack(4, K, F), down, fused=True, w3_glu_blocks=value)
    with pytest.raises(ValueError, match="one of them"):
        moe.FluteExperts(gate, up, down, fused=True, glu_blocks=True, w3_glu_blocks=True)
    full, partial = thresholds()                                           # "auto" reads the shapes alone: E (F / 256) = 4
    hidden = torch.empty(7, K, dtype=torch.float16, device="meta")
    auto = moe.FluteExperts(gate, up, down, fused=True, w3_glu_blocks="auto")
    assert auto._takes_w3_glu_blocks(hidden, partial * E, 256) is True and auto._takes_w3_glu_blocks(hidden, partial * E - 1, 256) is False
    forced = moe.FluteExperts(gate, up, down, fused=True, w3_glu_blocks=True)
    moe.make_experts_learnable(forced)
    moe.make_experts_learnable(auto)
    with pytest.raises(ValueError, match="learnable"):
        forced._takes_w3_glu_blocks(hidden, 4096, 256)
    assert auto._takes_w3_glu_blocks(hidden, 4096, 256) is False
