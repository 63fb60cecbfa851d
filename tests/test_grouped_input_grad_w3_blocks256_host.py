"""The 256-row block form of the grouped input gradient for 3-bit stacks without a GPU (flute_qgemm_grouped_input_grad_w3_blocks256
and its query): the symbols, the refusals in their order on null pointers, the query on both sides of the header's thresholds,
and the `w3_grad_blocks256` keyword's checks and defaults."""
import inspect
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib, dev
from flute_amd.integrations import moe
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -4, -7, -9
BLOCKS256 = 3
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
NAME = "FLUTE_GROUPED_INPUT_GRAD_W3_BLOCKS256_MIN_MEAN_ROWS"
FORWARD_OPS = ["qgemm_grouped", "qgemm_grouped_w3_blocks", "qgemm_grouped_weighted", "qgemm_grouped_weighted_w3_blocks",
               "qgemm_grouped_glu", "qgemm_grouped_glu_w3_blocks"]


def tid_of(bits):
    return first_template(bits, 32) if bits in (2, 3, 4) else 0


def thresholds():
    """(where the experts' k blocks fill the chip, where they do not) from the header; 0 is never."""
    with open(HEADER) as f:
        d = dict(l.split()[1:3] for l in f if l.startswith("#define " + NAME))
    return int(d[NAME]), int(d[NAME + "_PARTIAL"])


def launch(dtype=0, bits=3, g=64, E=8, R=4096, N=1024, K=512, P=None, ptrs=(None,) * 11):
    # dY, offsets, Q, S, QM2, row_weight, dY2, Q2, S2, QM22, dX
    return _lib.get().flute_qgemm_grouped_input_grad_w3_blocks256(dtype, bits, g, E, R, N, K, bits * N // 16 if P is None else P,
                                                                  tid_of(bits), *ptrs, 256, None)


def query(pair=0, dtype=0, g=64, E=8, R=4096, N=1024, K=512, num_sms=256):
    return _lib.get().flute_qgemm_grouped_input_grad_w3_blocks256_form(pair, dtype, g, E, R, N, K, tid_of(3), num_sms)


def test_symbols():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_input_grad_w3_blocks256", "flute_qgemm_grouped_input_grad_w3_blocks256_form"):
        assert name in _lib.SYMBOLS and "int %s(" % name in text
        getattr(_lib.get(), name)
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_grouped_input_grad_w3_blocks256 is flute_amd.ops.qgemm_grouped_input_grad_w3_blocks256


def test_refusals_in_their_order_at_null_pointers():
    # dtype, the layer (bit width, group size, template), the shape - each ahead of the next
    assert launch(dtype=2, bits=5) == ERR_DTYPE and launch(bits=5, g=48) == ERR_NUM_BITS and launch(g=48, P=1) == ERR_GROUP_SIZE
    assert launch(P=255) == ERR_SHAPE and launch(E=-1) == ERR_SHAPE and launch(R=-1) == ERR_SHAPE
    # then what the form serves - 3 bits, then grouped_input_grad_w3_blocks256_eligible - before the null pointers
    for bits in (4, 2):
        assert launch(bits=bits) == ERR_NUM_BITS and launch(bits=bits, K=640) == ERR_NUM_BITS
    for kw in (dict(K=640), dict(K=128), dict(R=0), dict(E=0)):
        assert launch(**kw) == ERR_SHAPE, kw
    assert launch(R=2 ** 31 - 512) == ERR_SHAPE and launch(R=2 ** 31 - 513) == ERR_NULL
    for kw in (dict(), dict(dtype=1), dict(g=32), dict(R=1), dict(N=1536, K=14336)):
        assert launch(**kw) == ERR_NULL, kw


def test_query_on_both_sides_of_the_header_thresholds():
    full, partial = thresholds()
    old = lambda pair, E, K, R: _lib.get().flute_qgemm_grouped_input_grad_w3_blocks_form(pair, 0, 64, E, R, 1024, K, tid_of(3), 256)
    for pair in (0, 1):
        for E, K in ((64, 1024), (8, 8192), (8, 8192 - 256), (1, 512)):     # E (K / 256) against 256 compute units
            thr = full if E * (K // 256) >= 256 else partial
            if thr == 0:                                                     # the form never pays on this kind of shape
                assert query(pair, E=E, K=K, R=2 ** 20) == old(pair, E, K, 2 ** 20) != BLOCKS256
                continue
            assert query(pair, E=E, K=K, R=thr * E) == BLOCKS256
            assert query(pair, E=E, K=K, R=thr * E - 1) == old(pair, E, K, thr * E - 1) != BLOCKS256
    assert query(dtype=2) == ERR_DTYPE and query(g=48) == ERR_GROUP_SIZE and query(E=-1) == ERR_SHAPE
    big = max(full, partial, 128) * 64                                       # (a mean of 128: the 128-row form's at the least)
    assert query(E=64, K=1024 + 128, R=big) != BLOCKS256 and query(R=0) != BLOCKS256
    assert dev.grouped_input_grad_w3_blocks256_form(64, 7, 1024, 1024, 64, tid_of(3)) == "slabs"
    want = "blocks256" if full else "blocks"
    assert dev.grouped_input_grad_w3_blocks256_form(64, big, 1024, 1024, 64, tid_of(3), 256, torch.bfloat16, pair=True) == want


def meta_args(name, bits=3, E=2, K=256, N=512, g=32, R=8):
    """The operands of forward op `name` on meta tensors, the input requiring grad."""
    meta = lambda *s, dtype=torch.float16: torch.empty(s, dtype=dtype, device="meta")
    stack = (meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g), meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))
    args = (meta(R, K).requires_grad_(), meta(E + 1, dtype=torch.int32)) + stack * (2 if "glu" in name else 1)
    return args + ((meta(R, dtype=torch.float32),) if "weighted" in name else ()) + (bits, g, tid_of(bits))


@pytest.mark.parametrize("name", FORWARD_OPS)
def test_the_keyword_validates(name):
    op = getattr(flute_amd, name)
    for value in ("maybe", "blocks256", 1, None):
        with pytest.raises(ValueError, match="w3_grad_blocks256 is False, True or 'auto'"):
            op(*meta_args(name), w3_grad_blocks256=value)
    if "w3_blocks" not in name:                                              # (those ops refuse 4 bits first)
        for value in (True, "auto"):
            with pytest.raises(ValueError, match="w3_grad_blocks256 selects the input-gradient kernel of 3-bit stacks"):
                op(*meta_args(name, bits=4), w3_grad_blocks256=value)
    for value in (False, True, "auto"):                                      # a legal value passes on to the launch's GPU check
        with pytest.raises(RuntimeError, match="same GPU"):
            op(*meta_args(name), w3_grad_blocks256=value, w3_grad_blocks="auto")


def test_the_defaults_are_false_and_the_module_validates():
    for fn in [getattr(flute_amd, n) for n in FORWARD_OPS] + [moe.FluteExperts.__init__, moe.FluteExperts.from_linears]:
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "w3_grad_blocks256" and params[-1].default is False, fn
    E, K, F, g = 2, 512, 512, 32
    stack = lambda bits, kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, tid_of(bits), torch.device("cpu"), torch.float16)
    gate, up, down = stack(3, K, F), stack(3, K, F), stack(3, F, K)
    assert moe.FluteExperts(gate, up, down).w3_grad_blocks256 is False
    for value in (False, True, "auto"):
        experts = moe.FluteExperts(gate, up, down, fused=True, w3_grad_blocks=True, w3_grad_blocks256=value)
        assert experts._w3_grad_blocks256(gate, up, down) is value and experts._w3_grad_blocks(gate, up, down) is True
    for value in ("maybe", 1, None):
        with pytest.raises(ValueError, match="w3_grad_blocks256"):
            moe.FluteExperts(gate, up, down, w3_grad_blocks256=value)
    with pytest.raises(ValueError, match="w3_grad_blocks256 .* must be 3-bit"):
        moe.FluteExperts(gate, up, stack(4, F, K), w3_grad_blocks256=True)
    learnable = moe.LearnableGroupedFluteLinear(down)
    assert moe.FluteExperts(gate, up, learnable, w3_grad_blocks256="auto")._w3_grad_blocks256(learnable) is False
    with pytest.raises(ValueError, match="learnable"):
        moe.FluteExperts(gate, up, learnable, w3_grad_blocks256=True)._w3_grad_blocks256(gate, learnable)
