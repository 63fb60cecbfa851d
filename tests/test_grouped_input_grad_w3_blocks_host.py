"""The 3-bit block form of the grouped input gradient without a GPU (flute_qgemm_grouped_input_grad_w3_blocks and its query): the
symbols, the refusals in their order (returned before anything is enqueued or dereferenced, on null and on fake pointers), the
query's flip at the two header constants, and the Python op's and the `w3_grad_blocks` keyword's checks on meta tensors."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from flute_amd.integrations import moe
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -4, -7, -9
SLABS, BLOCKS = 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind
NAME = "FLUTE_GROUPED_INPUT_GRAD_W3_BLOCKS_MIN_MEAN_ROWS"


def tid_of(bits):
    return first_template(bits, 32) if bits in (2, 3, 4) else 0


def thresholds():
    with open(HEADER) as f:
        d = dict(l.split()[1:3] for l in f if l.startswith("#define " + NAME))
    return int(d[NAME]), int(d[NAME + "_PARTIAL"])


def launch(dtype=0, bits=3, g=64, E=8, R=4096, N=1024, K=512, P=None, ptrs=None):
    # dY, offsets, Q, S, QM2, row_weight, dY2, Q2, S2, QM22, dX: the single form unless `ptrs` says otherwise
    ptrs = (None,) * 11 if ptrs is None else (ptrs,) * 5 + (None,) * 5 + (ptrs,) if isinstance(ptrs, int) else ptrs
    return _lib.get().flute_qgemm_grouped_input_grad_w3_blocks(dtype, bits, g, E, R, N, K, bits * N // 16 if P is None else P,
                                                               tid_of(bits), *ptrs, 256, None)


def query(pair=0, dtype=0, g=64, E=8, R=4096, N=1024, K=512, num_sms=256):
    return _lib.get().flute_qgemm_grouped_input_grad_w3_blocks_form(pair, dtype, g, E, R, N, K, tid_of(3), num_sms)


def test_symbols():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_input_grad_w3_blocks", "flute_qgemm_grouped_input_grad_w3_blocks_form"):
        assert name in _lib.SYMBOLS and "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9\n" in text and _lib.get().flute_abi_version() == 9
    full, partial = thresholds()
    assert 1 <= full and 1 <= partial
    assert flute_amd.qgemm_grouped_input_grad_w3_blocks is flute_amd.ops.qgemm_grouped_input_grad_w3_blocks


def test_refusals_in_their_order():
    # the old entry's: dtype, the layer checks, P and the negative counts, a row weight with the pair form - each ahead of the next
    assert launch(dtype=2, bits=5) == ERR_DTYPE and launch(bits=5, g=48) == ERR_NUM_BITS and launch(g=48, P=1) == ERR_GROUP_SIZE
    assert launch(P=191) == ERR_SHAPE and launch(E=-1) == ERR_SHAPE and launch(R=-1) == ERR_SHAPE
    assert launch(bits=4, P=1) == ERR_SHAPE and launch(dtype=2, K=640) == ERR_DTYPE
    both = (FAKE,) * 5 + (FAKE, FAKE, None, None, None, FAKE)               # a row weight and one pointer of the pair form
    assert launch(ptrs=both) == ERR_SHAPE and launch(bits=4, ptrs=both) == ERR_SHAPE
    # then the bit width, then the eligibility rule, before the empty launch and before any pointer
    for bits in (4, 2):
        for kw in (dict(), dict(K=640), dict(R=0), dict(E=0)):
            assert launch(bits=bits, **kw) == ERR_NUM_BITS and launch(bits=bits, ptrs=FAKE, **kw) == ERR_NUM_BITS, (bits, kw)
    for K in (640, 128):
        for kw in (dict(), dict(R=0), dict(E=0), dict(ptrs=FAKE)):
            assert launch(K=K, **kw) == ERR_SHAPE, (K, kw)
    assert launch(R=2 ** 31 - 256) == ERR_SHAPE and launch(R=2 ** 31 - 257) == ERR_NULL
    # then the empty launches, then the pointers
    assert launch(R=0) == OK and launch(R=0, ptrs=FAKE) == OK and launch(E=0, R=0) == OK and launch(E=0, R=0, ptrs=FAKE) == OK
    assert launch(E=0) == ERR_NULL                                           # R > 0 rows of zeros need a dX
    for kw in (dict(), dict(dtype=1), dict(K=256, g=32), dict(R=5), dict(N=1536, K=14336)):
        assert launch(**kw) == ERR_NULL, kw
    single = (FAKE,) * 5 + (None,) * 5 + (FAKE,)
    for i in (0, 1, 2, 3, 4, 10):
        assert launch(ptrs=tuple(None if j == i else p for j, p in enumerate(single))) == ERR_NULL, i
    assert launch(ptrs=(FAKE,) * 5 + (None, FAKE, FAKE, None, FAKE, FAKE)) == ERR_NULL        # a pair form given in part


def test_query_flips_at_the_header_constants():
    full, partial = thresholds()
    for pair in (0, 1):
        for E, K in ((64, 1024), (8, 8192), (8, 8192 - 256), (1, 512)):     # E (K / 256) against 256 compute units
            thr = full if E * (K // 256) >= 256 else partial
            assert query(pair, E=E, K=K, R=thr * E) == BLOCKS and query(pair, E=E, K=K, R=thr * E - 1) == SLABS
    assert query(E=8, R=full * 8, num_sms=16) == BLOCKS and query(E=8, R=full * 8 - 1, num_sms=16) == SLABS
    for R in (partial * 8, partial * 8 - 1, full * 8, full * 8 - 1):        # num_sms < 1: 256
        assert query(E=8, R=R, num_sms=0) == query(E=8, R=R, num_sms=-3) == query(E=8, R=R, num_sms=256)
    assert query(dtype=2) == ERR_DTYPE and query(g=48) == ERR_GROUP_SIZE and query(E=-1) == ERR_SHAPE
    big = max(full, partial) * 8
    assert query(E=0) == SLABS and query(R=0) == SLABS and query(K=640, R=big) == SLABS and query(K=128, g=32, R=big) == SLABS
    assert dev.grouped_input_grad_w3_blocks_form(8, big, 1024, 512, 64, tid_of(3)) == "blocks"
    assert dev.grouped_input_grad_w3_blocks_form(8, min(full, partial) * 8 - 1, 1024, 512, 64, tid_of(3), 256, torch.bfloat16,
                                                 pair=True) == "slabs"
    # the old query and the old entry keep their answers at 3 bits
    assert _lib.get().flute_qgemm_grouped_input_grad_form(0, 0, 3, 64, 8, big, 1024, 512, tid_of(3), 256) == SLABS
    assert _lib.get().flute_qgemm_grouped_input_grad_ex(0, 3, 64, 8, big, 1024, 512, 192, tid_of(3), *(FAKE,) * 5, *(None,) * 5,
                                                        FAKE, 256, None, BLOCKS) == ERR_SHAPE


def meta_args(weighted=False, E=2, K=256, N=512, bits=3, g=32, R=8, grad=False):
    """The operands of the input gradient (dY [R, N] first), or with `grad` of the forward ops (x [R, K] first, requiring grad)."""
    meta = lambda *s, dtype=torch.float16: torch.empty(s, dtype=dtype, device="meta")
    first = meta(R, K).requires_grad_() if grad else meta(R, N)
    args = (first, meta(E + 1, dtype=torch.int32), meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g),
            meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))
    return args + ((meta(R, dtype=torch.float32),) if weighted else ()) + (bits, g, tid_of(bits))


def test_python_op_validates_before_a_launch():
    op = flute_amd.qgemm_grouped_input_grad_w3_blocks
    for kw in (dict(bits=4), dict(bits=2), dict(K=128), dict(K=640, g=64)):
        with pytest.raises(ValueError, match="not eligible"):
            op(*meta_args(**kw))
    with pytest.raises(RuntimeError, match="same GPU"):                       # an eligible layer stops where the launch needs a GPU tensor
        op(*meta_args())
    with pytest.raises(TypeError):
        op(*meta_args(), form="blocks")                                      # the op has no `form`
    with pytest.raises(ValueError, match="pair form"):
        op(*meta_args(), grad_output2=meta_args()[0])
    bad = list(meta_args())
    bad[0] = bad[0].to(torch.bfloat16)
    with pytest.raises(TypeError):
        op(*bad)


@pytest.mark.parametrize("name", ["qgemm_grouped", "qgemm_grouped_w3_blocks", "qgemm_grouped_weighted",
                                  "qgemm_grouped_weighted_w3_blocks", "qgemm_grouped_glu"])
def test_the_keyword_validates(name):
    op, weighted = getattr(flute_amd, name), "weighted" in name

    def args(**kw):
        a = meta_args(weighted, **kw)
        return a[:2] + a[2:5] * 2 + a[5:] if name.endswith("glu") else a     # the GLU op takes two stacks
    for value in ("maybe", "blocks", 1, None):
        with pytest.raises(ValueError, match="w3_grad_blocks is False, True or 'auto'"):
            op(*args(grad=True), w3_grad_blocks=value)
    if "w3" not in name:                                                     # (the w3 ops refuse other bit widths first)
        for value in (True, "auto"):
            with pytest.raises(ValueError, match="3-bit stacks"):
                op(*args(grad=True, bits=4, N=256), w3_grad_blocks=value)
    for value in (False, True, "auto"):                                      # a legal value passes on to the launch's GPU check
        with pytest.raises(RuntimeError, match="same GPU"):
            op(*args(grad=True), w3_grad_blocks=value)


def test_flute_experts_validates_w3_grad_blocks():
    E, K, F, g = 2, 512, 512, 32
    stack = lambda bits, kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, tid_of(bits), torch.device("cpu"), torch.float16)
    gate, up, down = stack(3, K, F), stack(3, K, F), stack(3, F, K)
    assert moe.FluteExperts(gate, up, down).w3_grad_blocks is False
    for value in (False, True, "auto"):
        assert moe.FluteExperts(gate, up, down, w3_grad_blocks=value).w3_grad_blocks is value
        assert moe.FluteExperts(gate, up, down, fused=True, w3_blocks="auto", w3_grad_blocks=value)._w3_grad_blocks(gate, up) is value
    for value in ("maybe", "blocks", 1, None):
        with pytest.raises(ValueError, match="w3_grad_blocks"):
            moe.FluteExperts(gate, up, down, w3_grad_blocks=value)
    for value in (True, "auto"):
        with pytest.raises(ValueError, match="3-bit"):
            moe.FluteExperts(gate, up, stack(4, F, K), w3_grad_blocks=value)
    learnable = moe.LearnableGroupedFluteLinear(down)
    assert moe.FluteExperts(gate, up, learnable, w3_grad_blocks="auto")._w3_grad_blocks(learnable) is False
    with pytest.raises(ValueError, match="learnable"):
        moe.FluteExperts(gate, up, learnable, w3_grad_blocks=True)._w3_grad_blocks(gate, learnable)
