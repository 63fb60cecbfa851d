"""flute_qgemm_scale_grad and flute_amd.qgemm_scale_grad without a GPU: the C ABI's refusals (each returned before
anything is enqueued), the wrapper's validation on meta tensors, and the suite's fp64 formula against the
reference's absmax gradient recorded by tests/golden/make_scale_grad_golden.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flute_amd
from flute_amd import _lib
from tests import scale_grad_ref as SR
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: every call below is refused before a launch
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "scale_grad", "manual_nf4_absmax_grad.npz")


def call(dtype=0, bits=4, g=64, M=8, N=1024, K=512, P=None, tid=0, ptrs=(FAKE,) * 5, scratch=None, nbytes=0,
         num_sms=256):
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_scale_grad(dtype, bits, g, M, N, K, P, tid, *ptrs, scratch, nbytes, num_sms, None)


def test_symbol_exported_abi_unchanged():
    assert "flute_qgemm_scale_grad" in _lib.SYMBOLS
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_scale_grad is flute_amd.ops.qgemm_scale_grad
    assert not hasattr(torch.ops.flute_amd, "qgemm_scale_grad")


@pytest.mark.parametrize("i", range(5))
def test_null_pointers_refused(i):
    ptrs = [FAKE] * 5
    ptrs[i] = None
    assert call(ptrs=ptrs) == ERR_NULL
    assert call(ptrs=ptrs, bits=5, M=0) == ERR_NULL          # before any other check


def test_layer_refusals():
    assert call(dtype=2) == ERR_DTYPE
    assert call(bits=5) == ERR_NUM_BITS
    assert call(bits=1) == ERR_NUM_BITS
    for g in (0, 16, 48, 512):
        assert call(g=g) == ERR_GROUP_SIZE, g
    assert call(tid=10 ** 6) == ERR_TEMPLATE_ID
    assert call(bits=3, N=512, tid=first_template(3, 64)) == ERR_TEMPLATE_ID      # 3 bits: TileP 32 only


def test_shape_refusals():
    assert call(N=1000) == ERR_SHAPE             # N % (J * TileP)
    assert call(N=0) == ERR_SHAPE
    assert call(bits=3, N=256, tid=first_template(3, 32)) == ERR_SHAPE      # 3 bits: N % 512
    assert call(K=480) == ERR_SHAPE              # K % 64
    assert call(K=384, g=256) == ERR_SHAPE       # K % g
    assert call(K=0) == ERR_SHAPE
    assert call(P=255) == ERR_SHAPE
    assert call(M=0) == ERR_SHAPE
    assert call(M=-1) == ERR_SHAPE


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def args(M=8, K=512, N=1024, bits=4, dtype=torch.float16):
    return (meta(M, N, dtype=dtype), meta(M, K, dtype=dtype), meta(bits * N // 16, K, dtype=torch.int16),
            meta(2 ** bits, 2 ** bits, 1, dtype=torch.float32))


def test_wrapper_validation_before_launch():
    dy, x, w, t2 = args()
    f = flute_amd.qgemm_scale_grad
    with pytest.raises(TypeError):
        f(dy.float(), x.float(), w, t2, 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x.to(torch.bfloat16), w, t2, 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x, w.to(torch.int32), t2, 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x, w, t2.half(), 4, 64, 0)
    with pytest.raises(ValueError):
        f(dy, x[0], w, t2, 4, 64, 0)                          # 1-d input
    with pytest.raises(ValueError):
        f(dy[:4], x, w, t2, 4, 64, 0)                         # rows differ
    with pytest.raises(ValueError):
        f(dy, x[:, :448], w, t2, 4, 64, 0)                    # K != weight's
    with pytest.raises(ValueError):
        f(dy[:, :512], x, w, t2, 4, 64, 0)                    # P != b N / 16
    with pytest.raises(ValueError):
        f(dy, x, w, t2, 4, 48, 0)                             # group size
    with pytest.raises(ValueError):
        f(dy, x, w, t2, 5, 64, 0)                             # bits
    with pytest.raises(ValueError):
        f(dy, x, w, t2[:8], 4, 64, 0)                         # table2 shape
    with pytest.raises(RuntimeError, match="GPU"):
        f(dy, x, w, t2, 4, 64, 0)                             # valid, but not on a GPU


def test_scratch_bound_covers_every_split():
    """The wrapper's scratch is the most the launch can use: blocks of 256 x 128 below two per CU."""
    from flute_amd.ops import _scale_grad_scratch_bytes as nbytes
    assert nbytes(28672, 8192, 64, 256) == 0                   # 7168 blocks: never split
    assert nbytes(1024, 1024, 64, 256) == 16 * 1024 * 16 * 4   # 32 blocks: up to 16 splits
    assert nbytes(128, 256, 32, 256) == 512 * 128 * 8 * 4


def test_fp64_formula_matches_reference_absmax_grad():
    z = np.load(GOLDEN)
    g = int(z["group_size"])
    codes = torch.from_numpy(z["codes"]).long()                # [N, K], the codes manual_nf4 chose
    values = torch.from_numpy(z["values"])
    assert z["values"].dtype == np.float64 and z["grad"].dtype == np.float64
    n = values.numel()
    pairs = torch.stack([values[:, None].expand(n, n), values[None, :].expand(n, n)], -1).reshape(n * n, 2)
    L = SR.lut_of_codes(codes.T, pairs, 4)                     # [K, N]
    assert torch.equal(L, values[codes].T)
    X, dY = torch.from_numpy(z["X"]), torch.from_numpy(z["dY"])
    got = SR.scale_grad(dY, X, L, g)
    ref = torch.from_numpy(z["grad"])
    scale = SR.scale_grad(dY, X, L, g, absolute=True)
    assert got.shape == ref.shape
    assert torch.all((got - ref).abs() <= 1e-13 * scale + 1e-300), float((got - ref).abs().max())
    # the codes are what the pivots give for W / absmax: recomputing them is not possible without W, but every code
    # must be a valid 4-bit index and the fixture's scales positive
    assert codes.min() >= 0 and codes.max() < 16 and (torch.from_numpy(z["absmax"]) > 0).all()
