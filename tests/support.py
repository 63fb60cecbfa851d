"""What every GPU test needs: the one `Env` and its module-scoped fixture, the lowest template id of a layout, bit views,
row offsets, integer draws and the two error measures.  Importable without a GPU: the package is imported inside the
functions that need it."""
import contextlib

import pytest
import torch


class Env:
    """The package's modules, the device and its workspace.  `lib_mod` is the module flute_amd._lib, `lib` the loaded
    library handle `_lib.get()`; `cache` and `layers` are per-module stores that start empty."""


def make_env():
    import flute_amd
    import flute_amd.nf_utils  # noqa: F401
    from flute_amd import _lib, dev, utils
    from flute_amd.integrations import learnable, moe
    from flute_amd.integrations.base import FluteLinear
    from flute_amd.ops import _stream_ptr
    from oracle import flute_oracle as O

    e = Env()
    e.fa, e.utils, e.O, e.moe, e.ln, e.FluteLinear, e.dev_mod = flute_amd, utils, O, moe, learnable, FluteLinear, dev
    e.lib_mod, e.lib = _lib, _lib.get()
    e.check, e.stream_ptr = _lib.check, _stream_ptr
    e.dev = torch.device("cuda:0")
    e.num_sms = utils.get_device_num_sms(e.dev)
    e.ws = utils.get_workspace_streamk(e.dev)
    e.cache, e.layers = {}, {}
    return e


@pytest.fixture(scope="module")
def env():
    """One Env per test module: the module's caches go with it."""
    return make_env()


def first_template(bits, tile_p):
    """The lowest template id of a bit width with this TileP."""
    import flute_amd
    return min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == tile_p)


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


def bits_by_size(t):
    """A copy of `t` as integers of its element size."""
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()]).clone()


def offsets_of(counts, device=None):
    off = torch.zeros(len(counts) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(counts), 0)
    return off if device is None else off.to(device)


def ints(M, K, amp, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, (M, K), generator=gen).to(dtype)


@contextlib.contextmanager
def fp32_blas_reduction():
    """hipBLASLt may reduce fp16 / bf16 GEMMs in reduced precision by default; the exact cases need fp32 partial sums."""
    m = torch.backends.cuda.matmul
    old = (m.allow_fp16_reduced_precision_reduction, m.allow_bf16_reduced_precision_reduction)
    m.allow_fp16_reduced_precision_reduction = False
    m.allow_bf16_reduced_precision_reduction = False
    try:
        yield
    finally:
        m.allow_fp16_reduced_precision_reduction, m.allow_bf16_reduced_precision_reduction = old


def norm_rel_err(out, ref):
    """|out - ref|_2 / |ref|_2 in fp32, where the tensors are."""
    out, ref = out.float(), ref.float()
    return ((out - ref).norm() / ref.norm()).item()


def max_rel_err(a, ref):
    """max |a - ref| / max |ref|, `ref` in fp64."""
    return float((a.double() - ref).abs().max() / ref.abs().max())
