"""flute_qgemm_grouped_input_grad, its Python wrapper and the autograd entry of the grouped ops without a GPU: the
exports, every refusal of the C ABI (returned before anything is enqueued, on null or host pointers), the wrapper's
validation on meta tensors, and the raise that replaces a silently detached result."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from flute_amd.ops import _validate_grouped_input_grad
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind


def igrad(dtype=0, bits=4, g=64, E=4, R=8, N=1024, K=512, P=None, tid=0, ptrs=(None,) * 11, num_sms=256):
    """ptrs: dY, offsets, Q, S, QM2, row_weight, dY2, Q2, S2, QM22, dX"""
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_input_grad(dtype, bits, g, E, R, N, K, P, tid, *ptrs, num_sms, None)


def test_symbol_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_input_grad", "flute_qgemm_grouped_input_grad_row_block"):
        assert name in _lib.SYMBOLS
        assert "int %s(" % name in text
        getattr(_lib.get(), name)
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_grouped_input_grad is flute_amd.ops.qgemm_grouped_input_grad
    rb = flute_amd.ops.GROUPED_INPUT_GRAD_ROW_BLOCK
    assert rb == _lib.get().flute_qgemm_grouped_input_grad_row_block()
    assert "#define FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK %d\n" % rb in text
    assert rb >= 64 and rb % 16 == 0            # one dequantized tile feeds several 16-row MFMA tiles


def test_layer_and_shape_refusals_with_null_pointers():
    assert igrad(dtype=2) == ERR_DTYPE
    assert igrad(bits=5) == ERR_NUM_BITS
    for g in (0, 16, 48, 512):
        assert igrad(g=g) == ERR_GROUP_SIZE, g
    assert igrad(tid=10 ** 6) == ERR_TEMPLATE_ID
    assert igrad(bits=3, tid=first_template(3, 64), N=512) == ERR_TEMPLATE_ID       # 3 bits: TileP 32 only
    assert igrad(dtype=2, bits=5) == ERR_DTYPE                                # the order: dtype first
    assert igrad(N=1000) == ERR_SHAPE
    assert igrad(tid=first_template(4, 64), N=128) == ERR_SHAPE                     # TileP 64: the column block is 256
    assert igrad(K=480) == ERR_SHAPE
    assert igrad(K=384, g=256) == ERR_SHAPE
    assert igrad(P=255) == ERR_SHAPE
    assert igrad(E=-1) == ERR_SHAPE
    assert igrad(R=-1) == ERR_SHAPE


def test_pair_form_nothing_to_do_and_nulls():
    single = [FAKE] * 5 + [None] * 5 + [FAKE]
    pair = [FAKE] * 5 + [None] + [FAKE] * 5
    # a row weight together with any pointer of the pair form is refused - before "nothing to do" and before the nulls
    for i in range(6, 10):
        ptrs = [FAKE] * 6 + [None] * 4 + [FAKE]
        ptrs[i] = FAKE
        assert igrad(ptrs=ptrs) == ERR_SHAPE, i
        assert igrad(R=0, ptrs=ptrs) == ERR_SHAPE, i
    assert igrad(R=0) == OK                       # no launch: the null pointers are never looked at
    assert igrad(R=0, ptrs=single) == OK
    assert igrad() == ERR_NULL
    assert igrad(E=0) == ERR_NULL                 # E == 0 still writes dX (zeros): a null dX is refused
    for i in (0, 1, 2, 3, 4, 10):
        ptrs = list(single)
        ptrs[i] = None
        assert igrad(ptrs=ptrs) == ERR_NULL, i
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):     # the pair form given in part
        ptrs = list(pair)
        ptrs[i] = None
        assert igrad(ptrs=ptrs) == ERR_NULL, i


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def stack(E=4, K=512, N=1024, bits=4, g=64, dtype=torch.float16):
    return (meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g, dtype=dtype),
            meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))


def validate(dy, off, w, rw=None, dy2=None, w2=(None, None, None), bits=4, g=64):
    _validate_grouped_input_grad(dy, off, *w, bits, g, rw, dy2, *w2)


def test_validate_grouped_input_grad():
    dy, off, w = meta(8, 1024), meta(5, dtype=torch.int32), stack()
    rw = meta(8, dtype=torch.float32)
    validate(dy, off, w)
    validate(dy, off, w, rw=rw)
    validate(dy, off, w, dy2=meta(8, 1024), w2=stack())
    V, T = ValueError, TypeError
    bad = [
        (T, dict(dy=dy.float())),                                     # wrong dtypes
        (T, dict(dy=dy.bfloat16())),                                  # ... not the scales'
        (T, dict(w=(w[0].to(torch.int32), w[1], w[2]))),
        (T, dict(w=(w[0], w[1], w[2].half()))),
        (T, dict(off=off.long())),                                    # offsets: int32
        (V, dict(off=meta(4, dtype=torch.int32))),                    # ... of E + 1 entries
        (V, dict(off=meta(6, dtype=torch.int32))),
        (V, dict(dy=meta(8, 512))),                                   # grad_output.shape[1] != N
        (V, dict(dy=meta(8, 1024, 1))),
        (V, dict(bits=5)),
        (V, dict(g=48)),
        (V, dict(dy2=meta(8, 1024), w2=stack(N=2048))),               # a second stack of another shape
        (V, dict(dy2=meta(8, 1024), w2=stack(E=3))),
        (V, dict(dy2=meta(8, 1024), w2=stack(K=1024))),
        (V, dict(dy2=meta(8, 1024), w2=stack(g=128))),
        (V, dict(dy2=meta(7, 1024), w2=stack())),
        (T, dict(dy2=meta(8, 1024, dtype=torch.bfloat16), w2=stack())),
        (T, dict(dy2=meta(8, 1024), w2=stack(dtype=torch.bfloat16))),
        (V, dict(dy2=meta(8, 1024))),                                 # the pair form in part
        (V, dict(w2=stack())),
        (V, dict(rw=rw, dy2=meta(8, 1024), w2=stack())),              # row_weight together with the pair form
        (T, dict(rw=rw.half())),
        (V, dict(rw=meta(7, dtype=torch.float32))),
        (V, dict(rw=meta(8, 1, dtype=torch.float32))),
    ]
    for exc, kw in bad:
        args = dict(dy=dy, off=off, w=w)
        args.update(kw)
        with pytest.raises(exc):
            validate(**args)
    # the public function validates before any device call, then refuses tensors that are not on a GPU
    with pytest.raises(V):
        flute_amd.qgemm_grouped_input_grad(meta(8, 512), off, *w, 4, 64, 0)
    with pytest.raises(V):
        flute_amd.qgemm_grouped_input_grad(dy, off, *w, 4, 64, 0, row_weight=rw, grad_output2=dy, weight2=w[0], scales2=w[1],
                                           table22=w[2])
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.qgemm_grouped_input_grad(dy, off, *w, 4, 64, 0)


def test_no_silently_detached_result():
    """An op of the expert path backpropagates or raises.  Without a GPU: the stacks' scales / tables requiring grad raise
    the documented message before any device call, and the input-gradient op refuses to be differentiated itself."""
    cpu = lambda *shape, dtype=torch.float16: torch.zeros(shape, dtype=dtype)
    E, K, N, bits, g = 2, 64, 128, 4, 64
    w = (cpu(E, bits * N // 16, K, dtype=torch.int16), cpu(E, N, K // g), cpu(E, 16, 16, 1, dtype=torch.float32))
    x, off, rw = cpu(4, K), cpu(E + 1, dtype=torch.int32), cpu(4, dtype=torch.float32)
    msg = "gradients with respect to scales, table or table2 are not supported"
    learn = (w[0], w[1].clone().requires_grad_(), w[2])
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped: " + msg):
        flute_amd.qgemm_grouped(x, off, *learn, bits, g, 0)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_weighted: " + msg):
        flute_amd.qgemm_grouped_weighted(x, off, *learn, rw, bits, g, 0)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_glu: " + msg):
        flute_amd.qgemm_grouped_glu(x, off, *w, w[0], w[1], w[2].clone().requires_grad_(), bits, g, 0)
    with pytest.raises(RuntimeError, match="once-differentiable"):
        flute_amd.qgemm_grouped_input_grad(cpu(4, N).requires_grad_(), off, *w, bits, g, 0)
    with torch.no_grad():                                  # grad mode off: the plain path, which refuses CPU tensors as always
        with pytest.raises(RuntimeError, match="GPU"):
            flute_amd.qgemm_grouped(x, off, *learn, bits, g, 0)
