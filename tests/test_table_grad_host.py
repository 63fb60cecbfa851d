"""flute_qgemm_table_grad and flute_amd.qgemm_table_grad without a GPU: the C ABI's refusals (each returned before
anything is enqueued), the scratch query, the wrapper's validation on meta tensors, and the suite's fp64 formula
against torch autograd and against the reference's values / absmax gradients recorded by
tests/golden/make_table_grad_golden.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flute_amd
from flute_amd import _lib
from tests import scale_grad_ref as SR
from tests import table_grad_ref as TR
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_WORKSPACE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -5, -7, -9
FAKE = ctypes.c_void_p(0x1000)      # never dereferenced: every call below is refused before a launch
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "table_grad", "manual_nf4_values_grad.npz")
# dY, X, Q, S, QM2, dT2, dS, scratch
NAMES = ("dY", "X", "Q", "S", "QM2", "dT2", "dS", "scratch")


def query(bits=4, g=64, M=8, N=1024, K=512, want_dS=1, num_sms=256):
    return _lib.get().flute_qgemm_table_grad_scratch_bytes(bits, g, M, N, K, want_dS, num_sms)


def call(dtype=0, bits=4, g=64, M=8, N=1024, K=512, P=None, tid=0, ptrs=(FAKE,) * 8, nbytes=1 << 40, num_sms=256):
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_table_grad(dtype, bits, g, M, N, K, P, tid, *ptrs, nbytes, num_sms, None)


def test_symbols_exported_abi_unchanged():
    assert "flute_qgemm_table_grad" in _lib.SYMBOLS and "flute_qgemm_table_grad_scratch_bytes" in _lib.SYMBOLS
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_table_grad is flute_amd.ops.qgemm_table_grad
    assert flute_amd.pair_grad_to_table_grad is flute_amd.ops.pair_grad_to_table_grad
    assert not hasattr(torch.ops.flute_amd, "qgemm_table_grad")


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers_refused(name):
    i = NAMES.index(name)
    ptrs = [FAKE] * 8
    ptrs[i] = None
    if name == "dS":                                            # table only: allowed, and then QM2 may be null too
        ptrs[4] = None
        assert call(ptrs=ptrs, nbytes=0) == ERR_WORKSPACE       # passed every check up to the scratch size
        return
    assert call(ptrs=ptrs) == ERR_NULL
    assert call(ptrs=ptrs, bits=5, M=0) == ERR_NULL             # before any other check


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


def test_too_small_scratch_refused():
    for want_dS in (0, 1):
        for M in (8, 4099):
            need = query(M=M, want_dS=want_dS)
            assert need > 0
            ptrs = [FAKE] * 8
            if not want_dS:
                ptrs[6] = None
            assert call(M=M, ptrs=ptrs, nbytes=need - 1) == ERR_WORKSPACE
            assert call(M=M, ptrs=ptrs, nbytes=0) == ERR_WORKSPACE
    assert query(M=4099, want_dS=1) > query(M=4099, want_dS=0)         # the split's dS partials
    assert query(M=8, want_dS=1) == query(M=8, want_dS=0)              # too few rows to split: no dS partials


def test_query_refuses_what_the_call_refuses():
    assert query(bits=5) == 0 and query(g=48) == 0 and query(M=0) == 0 and query(N=1000) == 0 and query(K=480) == 0
    assert query(K=384, g=256) == 0


def test_query_covers_the_dispatch():
    """The launch writes one fp32 [4^b][2] partial per workgroup - blocks of 256 (k) x 128 (n) x splits of M - and, with
    dS and a split, fp32 [splits][N][K / g].  The split follows scale_grad's rule: never more than fill two workgroups
    per CU, never fewer than 4 steps of 32 rows each.  The query must hold the most that rule allows."""
    for bits in (2, 3, 4):
        for N, K in ((512, 1024), (1024, 3584), (4096, 4096), (28672, 8192), (512, 64)):
            for g in (32, 64, 256):
                if K % max(64, g):
                    continue
                for M in (1, 31, 129, 600, 4099, 70000):
                    for sms in (256, 64, 0):
                        blocks = (N // 128) * -(-K // 256)
                        steps = -(-M // 32)
                        target = 2 * (sms if sms >= 1 else 256)
                        splits = max(1, min(-(-target // blocks), steps // 4, 1024))
                        bins = 2 * 4 ** bits * 4
                        got0 = query(bits, g, M, N, K, 0, sms)
                        got1 = query(bits, g, M, N, K, 1, sms)
                        assert got0 >= blocks * bins and got0 % bins == 0
                        wgs = got0 // bins
                        assert wgs % blocks == 0 and 1 <= wgs // blocks <= splits, (bits, N, K, g, M, sms)
                        used = wgs // blocks
                        assert got1 == got0 + (used * N * (K // g) * 4 if used > 1 else 0)


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def args(M=8, K=512, N=1024, bits=4, g=64, dtype=torch.float16):
    return (meta(M, N, dtype=dtype), meta(M, K, dtype=dtype), meta(bits * N // 16, K, dtype=torch.int16),
            meta(N, K // g, dtype=dtype))


def test_wrapper_validation_before_launch():
    dy, x, w, s = args()
    t2 = meta(16, 16, 1, dtype=torch.float32)
    f = flute_amd.qgemm_table_grad
    with pytest.raises(TypeError):
        f(dy.float(), x.float(), w, s, 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x.to(torch.bfloat16), w, s, 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x, w.to(torch.int32), s, 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x, w, s.float(), 4, 64, 0)
    with pytest.raises(TypeError):
        f(dy, x, w, s, 4, 64, 0, table2=t2.half(), with_scale_grad=True)
    with pytest.raises(ValueError):
        f(dy, x[0], w, s, 4, 64, 0)                           # 1-d input
    with pytest.raises(ValueError):
        f(dy[:4], x, w, s, 4, 64, 0)                          # rows differ
    with pytest.raises(ValueError):
        f(dy, x[:, :448], w, s, 4, 64, 0)                     # K != weight's
    with pytest.raises(ValueError):
        f(dy[:, :512], x, w, s, 4, 64, 0)                     # P != b N / 16
    with pytest.raises(ValueError):
        f(dy, x, w, s[:, :4], 4, 64, 0)                       # scales shape
    with pytest.raises(ValueError):
        f(dy, x, w, s, 4, 48, 0)                              # group size
    with pytest.raises(ValueError):
        f(dy, x, w, s, 5, 64, 0)                              # bits
    with pytest.raises(ValueError):
        f(dy, x, w, s, 4, 64, 0, with_scale_grad=True)        # the scale gradient needs the table
    with pytest.raises(ValueError):
        f(dy, x, w, s, 4, 64, 0, table2=t2[:8], with_scale_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        f(dy, x, w, s, 4, 64, 0)                              # valid, but not on a GPU
    with pytest.raises(RuntimeError, match="GPU"):
        f(dy, x, w, s, 4, 64, 0, table2=t2, with_scale_grad=True)


def test_pair_grad_to_table_grad_is_the_adjoint():
    for bits in (2, 3, 4):
        n = 2 ** bits
        gen = torch.Generator().manual_seed(bits)
        t = torch.randn(n, dtype=torch.float64, generator=gen, requires_grad=True)
        d = torch.randn(n, n, 2, dtype=torch.float64, generator=gen)
        pairs = torch.stack([t[:, None].expand(n, n), t[None, :].expand(n, n)], -1)      # make_qmap2_from_qmap
        (pairs * d).sum().backward()
        got = flute_amd.pair_grad_to_table_grad(d)
        assert torch.allclose(got, t.grad, rtol=0, atol=1e-13)
        assert torch.equal(got, TR.to_scalar(d.reshape(n * n, 2), bits))
    with pytest.raises(ValueError):
        flute_amd.pair_grad_to_table_grad(torch.zeros(16, 2))


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("pair", [False, True])
def test_fp64_formula_matches_autograd(bits, pair):
    """A differentiable restatement of lookup x scale: W_hat[k, n] = pairs[idx(k / 2, n), k % 2] * S[n, k / g]."""
    gen = torch.Generator().manual_seed(10 * bits + pair)
    M, K, N, g = 5, 128, 48, 32
    n = 2 ** bits
    codes = torch.randint(0, n, (K, N), generator=gen)
    S = torch.randn(N, K // g, dtype=torch.float64, generator=gen)
    X = torch.randn(M, K, dtype=torch.float64, generator=gen)
    dY = torch.randn(M, N, dtype=torch.float64, generator=gen)
    if pair:
        leaf = torch.randn(n * n, 2, dtype=torch.float64, generator=gen, requires_grad=True)
        pairs = leaf
    else:
        leaf = torch.randn(n, dtype=torch.float64, generator=gen, requires_grad=True)
        pairs = torch.stack([leaf[:, None].expand(n, n), leaf[None, :].expand(n, n)], -1).reshape(n * n, 2)
    idx = TR.pair_index(codes, bits)                                           # [K / 2, N]
    L = pairs[idx].permute(0, 2, 1).reshape(K, N)
    assert torch.equal(L.detach(), SR.lut_of_codes(codes, pairs.detach(), bits))
    What = L * S.repeat_interleave(g, dim=1).T                                 # [K, N]
    ((X @ What) * dY).sum().backward()
    got = TR.table_grad(dY, X, codes, S, bits, g)
    A = TR.table_grad(dY, X, codes, S, bits, g, absolute=True)
    assert (A >= got.abs() - 1e-12).all()
    if not pair:
        got, A = TR.to_scalar(got, bits), TR.to_scalar(A, bits)
    assert got.shape == leaf.grad.shape
    assert torch.all((got - leaf.grad).abs() <= 1e-13 * A + 1e-300), float((got - leaf.grad).abs().max())


def test_fp64_formula_matches_reference_values_grad():
    z = np.load(GOLDEN)
    g = int(z["group_size"])
    codes = torch.from_numpy(z["codes"]).long()                # [N, K], the codes manual_nf4 chose
    assert z["values"].dtype == np.float64 and z["values_grad"].dtype == np.float64
    X, dY, S = torch.from_numpy(z["X"]), torch.from_numpy(z["dY"]), torch.from_numpy(z["absmax"])
    got = TR.to_scalar(TR.table_grad(dY, X, codes.T, S, 4, g), 4)
    scale = TR.to_scalar(TR.table_grad(dY, X, codes.T, S, 4, g, absolute=True), 4)
    ref = torch.from_numpy(z["values_grad"])
    assert got.shape == ref.shape == (16,)
    assert torch.all((got - ref).abs() <= 1e-13 * scale + 1e-300), float((got - ref).abs().max())
    # the same record carries the absmax gradient: the scale formula still agrees with it
    values = torch.from_numpy(z["values"])
    ds = SR.scale_grad(dY, X, values[codes].T, g)
    ds_scale = SR.scale_grad(dY, X, values[codes].T, g, absolute=True)
    assert torch.all((ds - torch.from_numpy(z["absmax_grad"])).abs() <= 1e-13 * ds_scale + 1e-300)
    assert codes.min() >= 0 and codes.max() < 16 and (S > 0).all()


def test_chain_depth_condition():
    for M in (1, 32, 33, 4099, 1 << 20):
        assert M + 2058 <= TR.chain_depth(M) <= M + 2 + 32768
