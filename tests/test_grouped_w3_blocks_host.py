"""The 3-bit block form of the grouped qgemm without a GPU (flute_qgemm_grouped_w3_blocks, _weighted_w3_blocks and their query):
the symbols, the refusals in their order (returned before anything is enqueued or dereferenced, on null and on fake pointers),
the query's flip at the two header constants, the old entries' unchanged answers at 3 bits, and the Python keyword checks."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from flute_amd.integrations import moe
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -4, -7, -9
ROWS, BLOCKS = 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
LIMIT = 2 ** 32 - 16


def tid_of(bits):
    return first_template(bits, 32) if bits in (2, 3, 4) else 0


def thresholds():
    with open(HEADER) as f:
        d = dict(l.split()[1:3] for l in f if l.startswith("#define FLUTE_GROUPED_W3_BLOCKS_MIN_MEAN_ROWS"))
    return int(d["FLUTE_GROUPED_W3_BLOCKS_MIN_MEAN_ROWS"]), int(d["FLUTE_GROUPED_W3_BLOCKS_MIN_MEAN_ROWS_PARTIAL"])


def launch(weighted=False, dtype=0, bits=3, g=64, E=8, T=4096, N=1024, K=512, P=None, ptrs=None):
    nptr = 7 if weighted else 6                  # X, offsets, Q, S, QM2, (row_weight,) Y
    fn = _lib.get().flute_qgemm_grouped_weighted_w3_blocks if weighted else _lib.get().flute_qgemm_grouped_w3_blocks
    ptrs = (None,) * nptr if ptrs is None else (ptrs,) * nptr if isinstance(ptrs, int) else ptrs
    return fn(dtype, bits, g, E, T, N, K, bits * N // 16 if P is None else P, tid_of(bits), *ptrs, 256, None)


def query(mode=0, dtype=0, g=64, E=8, rows=4096, N=1024, K=512, num_sms=256):
    return _lib.get().flute_qgemm_grouped_w3_blocks_form(mode, dtype, g, E, rows, N, K, tid_of(3), num_sms)


# (T + 256) K 2 and one expert's packed bytes 3 (N / 16) K 2 on both sides of 2^32 - 16
ACT_IN, ACT_OUT = dict(T=2 ** 20 - 257, K=2048), dict(T=2 ** 20 - 256, K=2048)
PACKED_IN, PACKED_OUT = dict(N=65536, K=341 * 512), dict(N=65536, K=342 * 512)
INELIGIBLE = [dict(bits=4), dict(bits=2), dict(N=1024 + 128), dict(K=448), ACT_OUT, PACKED_OUT]


def test_symbols():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_w3_blocks", "flute_qgemm_grouped_weighted_w3_blocks", "flute_qgemm_grouped_w3_blocks_form"):
        assert name in _lib.SYMBOLS and "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9\n" in text and _lib.get().flute_abi_version() == 9
    full, partial = thresholds()
    assert 1 <= full and 1 <= partial


@pytest.mark.parametrize("weighted", [False, True])
def test_refusals_in_their_order(weighted):
    run = lambda **kw: launch(weighted, **kw)
    # the old entry's: dtype, the layer checks, P and the negative counts - each ahead of the one after it
    assert run(dtype=2, bits=5) == ERR_DTYPE and run(bits=5, g=48) == ERR_NUM_BITS and run(g=48, P=1) == ERR_GROUP_SIZE
    assert run(P=191) == ERR_SHAPE and run(E=-1) == ERR_SHAPE and run(T=-1) == ERR_SHAPE
    assert run(dtype=2, N=1024 + 128) == ERR_DTYPE and run(g=48, K=448) == ERR_GROUP_SIZE
    # then the bit width and the eligibility rule, before the empty launch and before any pointer
    assert (3 * (65536 // 16)) * PACKED_IN["K"] * 2 < LIMIT <= (3 * (65536 // 16)) * PACKED_OUT["K"] * 2
    assert (ACT_IN["T"] + 256) * 2048 * 2 < LIMIT <= (ACT_OUT["T"] + 256) * 2048 * 2
    for kw in INELIGIBLE:
        assert run(**kw) == ERR_SHAPE and run(ptrs=FAKE, **kw) == ERR_SHAPE, kw
        assert run(**{**kw, "E": 0}) == ERR_SHAPE, kw
        if "T" not in kw:
            assert run(**{**kw, "T": 0}) == ERR_SHAPE, kw
    for kw in (ACT_IN, PACKED_IN, dict(K=256, g=32), dict(dtype=1), dict(T=5)):
        assert run(**kw) == ERR_NULL, kw
    # then the empty launches, then the pointers one by one
    assert run(E=0) == OK and run(T=0) == OK and run(E=0, ptrs=FAKE) == OK and run(T=0, ptrs=FAKE) == OK
    nptr = 7 if weighted else 6
    for i in range(nptr):
        assert run(ptrs=tuple(None if j == i else FAKE for j in range(nptr))) == ERR_NULL, i


def test_query_flips_at_the_header_constants():
    full, partial = thresholds()
    for mode in (0, 2):
        for E, N in ((64, 1024), (8, 8192), (8, 8192 - 512), (1, 1024)):      # E (N / 256) against 256 compute units
            thr = full if E * (N // 256) >= 256 else partial
            assert query(mode, E=E, N=N, rows=thr * E) == BLOCKS and query(mode, E=E, N=N, rows=thr * E - 1) == ROWS
    assert query(E=8, rows=full * 8, num_sms=32) == BLOCKS and query(E=8, rows=full * 8 - 1, num_sms=32) == ROWS
    for rows in (partial * 8, partial * 8 - 1, full * 8, full * 8 - 1):       # num_sms < 1: 256
        assert query(E=8, rows=rows, num_sms=0) == query(E=8, rows=rows, num_sms=-3) == query(E=8, rows=rows, num_sms=256)
    assert query(mode=1) == ERR_SHAPE and query(dtype=2) == ERR_DTYPE and query(g=48) == ERR_GROUP_SIZE and query(E=-1) == ERR_SHAPE
    assert query(E=0) == ROWS and query(rows=0) == ROWS and query(K=448) == ROWS and query(N=1024 + 512) == BLOCKS
    big = max(full, partial) * 8
    assert dev.grouped_w3_blocks_form("weighted", 8, big, 1024, 512, 64, tid_of(3)) == "blocks"
    assert dev.grouped_w3_blocks_form("plain", 8, min(full, partial) * 8 - 1, 1024, 512, 64, tid_of(3), 256, torch.bfloat16) == "rows"


def test_old_entries_keep_their_answers_at_three_bits():
    lib, tid = _lib.get(), tid_of(3)
    for mode in (0, 1, 2):
        assert lib.flute_qgemm_grouped_form(mode, 0, 3, 64, 8, 8192, 1024, 512, tid, 256) == ROWS
    head = (0, 3, 64, 8, 4096, 1024, 512, 192, tid)
    assert lib.flute_qgemm_grouped_ex(*head, *(FAKE,) * 6, 256, None, BLOCKS) == ERR_SHAPE
    assert lib.flute_qgemm_grouped_weighted_ex(*head, *(FAKE,) * 7, 256, None, BLOCKS) == ERR_SHAPE
    assert dev.grouped_form("plain", 8, 8192, 1024, 512, 3, 64, tid) == "rows"


def meta_args(weighted, E=2, K=256, N=512, bits=3, g=32, T=8):
    meta = lambda *s, dtype=torch.float16: torch.empty(s, dtype=dtype, device="meta")
    args = (meta(T, K), meta(E + 1, dtype=torch.int32), meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g),
            meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))
    return args + ((meta(T, dtype=torch.float32),) if weighted else ()) + (bits, g, tid_of(bits))


@pytest.mark.parametrize("weighted", [False, True])
def test_python_ops_validate_before_a_launch(weighted):
    op = flute_amd.qgemm_grouped_weighted_w3_blocks if weighted else flute_amd.qgemm_grouped_w3_blocks
    for kw in (dict(bits=4), dict(K=256, g=64), dict(N=128)):
        with pytest.raises(ValueError, match="not eligible"):
            op(*meta_args(weighted, **kw))
    with pytest.raises(RuntimeError, match="same GPU"):                       # an eligible layer stops where the launch needs a GPU tensor
        op(*meta_args(weighted))
    with pytest.raises(TypeError):
        op(*meta_args(weighted), form="blocks")                              # the ops have no `form`
    old = flute_amd.qgemm_grouped_weighted if weighted else flute_amd.qgemm_grouped
    with pytest.raises(ValueError, match="form"):
        old(*meta_args(weighted), form="w3_blocks")                          # ... and the old ops' `form` did not grow a value
    bad = list(meta_args(weighted))
    bad[0] = bad[0].to(torch.bfloat16)
    with pytest.raises(TypeError):
        op(*bad)


def test_flute_experts_validates_w3_blocks():
    E, K, F, g = 2, 512, 512, 32
    stack = lambda bits, kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, tid_of(bits), torch.device("cpu"), torch.float16)
    gate, up, down = stack(3, K, F), stack(3, K, F), stack(3, F, K)
    assert moe.FluteExperts(gate, up, down).w3_blocks is False
    for value in (False, True, "auto"):
        assert moe.FluteExperts(gate, up, down, w3_blocks=value).w3_blocks is value
        assert moe.FluteExperts(gate, up, down, fused=True, w3_blocks=value).w3_blocks is value
    for value in ("maybe", "blocks", 1, None):
        with pytest.raises(ValueError, match="w3_blocks"):
            moe.FluteExperts(gate, up, down, w3_blocks=value)
    for value in (True, "auto"):
        with pytest.raises(ValueError, match="3-bit"):
            moe.FluteExperts(gate, up, stack(4, F, K), w3_blocks=value)
    assert moe.FluteExperts(gate, up, stack(4, F, K), w3_blocks=False).w3_blocks is False
    experts = moe.FluteExperts(gate, up, down, fused=True, native_routing=True, w3_blocks="auto")
    assert moe.FluteSparseMoeBlock(torch.zeros(E, K), experts, top_k=1).experts.w3_blocks == "auto"
    full, partial = thresholds()                                             # "auto" reads the shapes alone: E (N / 256) = 4
    assert experts._takes_w3_blocks(down, "weighted", partial * E, 256, torch.float16) is True
    assert experts._takes_w3_blocks(down, "weighted", partial * E - 1, 256, torch.float16) is False
