"""flute_dequantize and the torch surface around it, without a GPU: the C ABI's refusals (every one returned before
anything is enqueued), the fake impl of flute_amd::dequantize, and the Autograd kernels of both flute:: ops."""
import ctypes

import pytest
import torch

import flute_amd
from flute_amd import _lib

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: every call below is refused before a launch


def call(dtype=0, bits=4, g=64, N=1024, K=512, P=None, k_begin=0, k_count=None, ptrs=(FAKE,) * 4, tid=0):
    P = bits * N // 16 if P is None else P
    k_count = K if k_count is None else k_count
    return _lib.get().flute_dequantize(dtype, bits, g, N, K, P, k_begin, k_count, *ptrs, tid, None)


def test_abi_version_and_symbol():
    lib = _lib.get()
    assert lib.flute_abi_version() == 9
    assert "flute_dequantize" in _lib.SYMBOLS


@pytest.mark.parametrize("i", range(4))
def test_null_pointers_refused(i):
    ptrs = [FAKE] * 4
    ptrs[i] = None
    assert call(ptrs=ptrs) == ERR_NULL
    assert call(ptrs=ptrs, bits=5) == ERR_NULL          # before any other check


def test_layer_refusals():
    assert call(bits=5) == ERR_NUM_BITS
    assert call(bits=1) == ERR_NUM_BITS
    assert call(g=48) == ERR_GROUP_SIZE
    assert call(g=512) == ERR_GROUP_SIZE
    assert call(tid=10 ** 6) == ERR_TEMPLATE_ID
    assert call(tid=-1) == ERR_TEMPLATE_ID
    assert call(dtype=2) == ERR_DTYPE
    assert call(N=1000) == ERR_SHAPE                   # N % (J * TileP)
    tid3 = next(t for (b, t), c in sorted(flute_amd.TEMPLATE_CONFIGS.items()) if b == 3 and c["TileP"] == 32)
    tid3_64 = [t for (b, t), c in sorted(flute_amd.TEMPLATE_CONFIGS.items()) if b == 3 and c["TileP"] == 64]
    assert call(bits=3, N=256, tid=tid3) == ERR_SHAPE   # 3 bits: N % 512
    for t in tid3_64[:1]:
        assert call(bits=3, N=512, tid=t) == ERR_TEMPLATE_ID   # 3 bits: TileP 32 only
    assert call(K=576, g=128) == ERR_SHAPE             # group size does not divide K
    assert call(K=96, g=32) == ERR_SHAPE               # K % 64


def test_k_range_and_p_refusals():
    assert call(P=4 * 1024 // 16 + 1) == ERR_SHAPE
    assert call(P=0) == ERR_SHAPE
    assert call(k_begin=32, k_count=64) == ERR_SHAPE
    assert call(k_begin=0, k_count=96) == ERR_SHAPE
    assert call(k_begin=-64, k_count=64) == ERR_SHAPE
    assert call(k_begin=0, k_count=-64) == ERR_SHAPE
    assert call(k_begin=448, k_count=128) == ERR_SHAPE   # past K
    assert call(k_begin=576, k_count=0) == ERR_SHAPE     # starts past K
    assert call(k_begin=128, k_count=0) == OK            # empty range: nothing to do, no launch
    assert call(k_begin=512, k_count=0) == OK


def meta_args(bits=4, N=1024, K=512, g=64, dtype=torch.float16):
    m = "meta"
    W = torch.empty(bits * N // 16, K, dtype=torch.int16, device=m)
    S = torch.empty(N, K // g, dtype=dtype, device=m)
    T2 = torch.empty(2 ** bits, 2 ** bits, 1, dtype=torch.float32, device=m)
    return W, S, T2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("bits,N,K,g", [(4, 1024, 512, 64), (3, 512, 256, 128), (2, 2048, 4096, 32)])
def test_fake_impl_shape_and_dtype(dtype, bits, N, K, g):
    W, S, T2 = meta_args(bits, N, K, g, dtype)
    out = flute_amd.dequantize(W, S, T2, bits, g, 0)
    assert out.shape == (N, K) and out.dtype == dtype and out.device.type == "meta"


def test_fake_impl_rejects_inconsistent_shapes():
    W, S, T2 = meta_args()
    with pytest.raises(ValueError):
        flute_amd.dequantize(W[:-1], S, T2, 4, 64, 0)                       # P != bits * N / 16
    with pytest.raises(ValueError):
        flute_amd.dequantize(W, S[:, :-1], T2, 4, 64, 0)                    # K != G * group_size
    with pytest.raises(ValueError):
        flute_amd.dequantize(W, S, T2[:8], 4, 64, 0)                        # table2 not 2^b x 2^b
    with pytest.raises(ValueError):
        flute_amd.dequantize(W[0], S, T2, 4, 64, 0)                         # rank
    with pytest.raises(TypeError):
        flute_amd.dequantize(W, S.float(), T2, 4, 64, 0)                    # fp32 scales
    with pytest.raises(TypeError):
        flute_amd.dequantize(W.int(), S, T2, 4, 64, 0)                      # int32 codes


def test_flute_amd_namespace_holds_only_dequantize():
    assert hasattr(torch.ops.flute_amd, "dequantize")
    # the reference's two schemas stay the only ops of `flute`
    names = torch._C._dispatch_get_all_op_names()
    assert sorted(n for n in names if n.startswith("flute::")) == ["flute::qgemm_raw_simple", "flute::qgemm_raw_simple_hadamard"]
    assert sorted(n for n in names if n.startswith("flute_amd::")) == ["flute_amd::dequantize"]


@pytest.mark.parametrize("op", ["flute::qgemm_raw_simple", "flute::qgemm_raw_simple_hadamard"])
def test_autograd_kernel_registered(op):
    table = torch._C._dispatch_dump_table(op)
    lines = {l.split(":")[0]: l for l in table.splitlines() if l.strip()}
    for key in ("AutogradCUDA", "AutogradCPU", "AutogradOther"):
        assert key in lines and "torch_binding.cpp" in lines[key] and "autograd kernel" in lines[key], lines.get(key)


def test_autograd_graph_only_when_needed():
    """On meta tensors: a grad-requiring input gets a grad_fn, a graph without one (or no_grad) gets none."""
    m = "meta"
    W, S, T2 = meta_args()
    T = torch.empty(16, dtype=torch.float16, device=m)
    ws = torch.empty(1024, dtype=torch.uint8, device=m)
    x = torch.empty(3, 5, 512, dtype=torch.float16, device=m, requires_grad=True)
    y = flute_amd.qgemm(x, W, S, T, T2, ws, 4, 64, 0, 256)
    assert y.shape == (3, 5, 1024) and y.requires_grad and y.grad_fn is not None
    yh = flute_amd.qgemm_hadamard(x, W, S, T, T2, ws, 4, 64, 128, 0, 256)
    assert yh.requires_grad and yh.grad_fn is not None
    with torch.no_grad():
        assert flute_amd.qgemm(x, W, S, T, T2, ws, 4, 64, 0, 256).grad_fn is None
    y2 = flute_amd.qgemm(x.detach(), W, S, T, T2, ws, 4, 64, 0, 256)
    assert not y2.requires_grad and y2.grad_fn is None
