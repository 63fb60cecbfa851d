"""The scale gradient of packed layers on the GPU: flute_amd.qgemm_scale_grad (param_grad.hip) bit for bit on exactly
representable data, within the componentwise bound on random data, deterministic across M splits, repeated calls
and graph replay, past 2^31 activation elements; qgemm_learnable_scales / LearnableScalesFluteLinear through
autograd, against dense fake quantization and the reference's recorded absmax gradient, and a short training run."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import exact_cases as XC
from tests import scale_grad_ref as SR
from tests.support import env, first_template, ints  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 1e-3, BF16: 4e-3}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "scale_grad", "manual_nf4_absmax_grad.npz")


def exact_layer(env, lay):
    tid = first_template(lay.bits, lay.tile_p)
    Q = env.utils.pack(lay.W.to(env.dev), lay.bits, [tid], env.num_sms)
    return Q, lay.table2.to(env.dev), tid, SR.lut_of_codes(lay.W.to(env.dev), lay.pairs, lay.bits)


def exact_reference(dY, X, L, g, dtype):
    R = SR.scale_grad(dY, X, L, g)
    A = SR.scale_grad(dY, X, L, g, absolute=True)
    assert float(A.max()) < 2.0 ** 24, "every partial sum an integer below 2^24: exact in fp32 in any order"
    assert torch.isfinite(R.to(dtype)).all()
    return R


def abi(env, dY, X, Q, table2, bits, g, tid, scratch=None, num_sms=None):
    """The C ABI directly: the scratch (and so the split of M) is the caller's."""
    M, N = dY.shape
    K = X.shape[1]
    out = torch.empty(N, K // g, dtype=X.dtype, device=env.dev)
    nbytes = scratch.numel() if scratch is not None else 0
    rc = env.fa._lib.get().flute_qgemm_scale_grad(
        0 if X.dtype == F16 else 1, bits, g, M, N, K, Q.shape[0], tid, dY.data_ptr(), X.data_ptr(), Q.data_ptr(),
        table2.data_ptr(), out.data_ptr(), scratch.data_ptr() if scratch is not None else None, nbytes,
        env.num_sms if num_sms is None else num_sms, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return out


# (bits, K, N, g, dtype, TileP, pair codebook): K with an odd number of groups and K past a 256-column block
EXACT = [
    (4, 1024, 512, 64, F16, 32, False), (4, 768, 256, 256, BF16, 64, False), (4, 320, 128, 64, F16, 32, True),
    (4, 1152, 256, 128, BF16, 32, False), (4, 448, 256, 32, BF16, 64, True),
    (3, 1152, 512, 128, BF16, 32, False), (3, 576, 512, 64, F16, 32, True),
    (2, 1280, 512, 256, F16, 64, False), (2, 448, 256, 32, BF16, 32, False), (2, 960, 512, 64, F16, 64, True),
]
MS = [1, 5, 31, 32, 33, 257, 4096]


@pytest.mark.parametrize("bits,K,N,g,dtype,tile_p,pair", EXACT)
def test_exact(env, bits, K, N, g, dtype, tile_p, pair):
    lay = XC.Layer(bits, K, N, g, dtype, seed=bits * 131 + K + N + g, tile_p=tile_p, pair=pair)
    Q, table2, tid, L = exact_layer(env, lay)
    for M in MS:
        amp = 4 if M <= 257 else 1
        dY = ints(M, N, amp, M + N, dtype).to(env.dev)
        X = ints(M, K, amp, M + K + 1, dtype).to(env.dev)
        R = exact_reference(dY, X, L, g, dtype)
        got = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)
        assert got.shape == (N, K // g) and got.dtype == dtype
        assert XC.exact_equal(got, R, dtype), (M, float((got.double() - R).abs().max()))


@pytest.mark.parametrize("bits,K,N,g,dtype,tile_p,M", [
    (4, 4096, 1024, 64, F16, 32, 600), (4, 2048, 2048, 128, BF16, 64, 77), (3, 2048, 1024, 64, BF16, 32, 1000),
    (2, 1024, 2048, 32, F16, 64, 3), (4, 1024, 1024, 256, BF16, 32, 4096)])
def test_random_within_componentwise_bound(env, bits, K, N, g, dtype, tile_p, M):
    """|dS - exact| <= gamma(M g) sum |dY X L| + u_T |exact|: fp32 products and sums in any order, one rounding."""
    d = env.dev
    gen = torch.Generator().manual_seed(K + N + M)
    codes = torch.randint(0, 2 ** bits, (K, N), generator=gen, dtype=torch.uint8)
    table = torch.tensor(env.fa.nf_utils.NF4_VALUES, dtype=dtype)
    table = table[:: 16 // 2 ** bits][: 2 ** bits]
    n = 2 ** bits
    pairs = torch.stack([table[:, None].expand(n, n), table[None, :].expand(n, n)], -1).reshape(n * n, 2).double()
    tid = first_template(bits, tile_p)
    Q = env.utils.pack(codes.to(d), bits, [tid], env.num_sms)
    table2 = env.utils.make_qmap2_from_qmap(table).to(d)
    L = SR.lut_of_codes(codes.to(d), pairs, bits)
    dY = torch.randn(M, N, generator=gen).to(dtype).to(d)
    X = torch.randn(M, K, generator=gen).to(dtype).to(d)
    got = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid).double()
    R = SR.scale_grad(dY, X, L, g)
    A = SR.scale_grad(dY, X, L, g, absolute=True)
    bound = XC.gamma(M * g + 2) * A + XC.U_T[dtype] * R.abs()
    assert torch.all((got - R).abs() <= bound), float(((got - R).abs() - bound).max())


def test_split_and_unsplit_agree_and_repeat(env):
    """A small layer splits M across workgroups when the scratch allows it; on exact data every split gives the
    unsplit bits, and each plan repeats itself bit for bit."""
    d = env.dev
    for bits, K, N, g, dtype, tile_p in ((4, 1024, 512, 64, F16, 32), (3, 1152, 512, 128, BF16, 32),
                                         (2, 448, 256, 32, BF16, 32)):
        lay = XC.Layer(bits, K, N, g, dtype, seed=K + N, tile_p=tile_p)
        Q, table2, tid, L = exact_layer(env, lay)
        M = 4099
        dY = ints(M, N, 1, 5, dtype).to(d)
        X = ints(M, K, 1, 6, dtype).to(d)
        R = exact_reference(dY, X, L, g, dtype)
        base = abi(env, dY, X, Q, table2, bits, g, tid)
        assert XC.exact_equal(base, R, dtype)
        for nbytes, sms in ((1 << 20, 256), (1 << 24, 256), (1 << 24, 1024), (4 * N * (K // g) * 2, 256)):
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=d)
            a = abi(env, dY, X, Q, table2, bits, g, tid, scratch, sms)
            b = abi(env, dY, X, Q, table2, bits, g, tid, scratch, sms)
            assert torch.equal(a.view(torch.int16), base.view(torch.int16)), (bits, nbytes, sms)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        r1 = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)
        r2 = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)
        assert torch.equal(r1.view(torch.int16), r2.view(torch.int16))


def test_random_repeat_and_graph_replay(env):
    d = env.dev
    bits, K, N, g, dtype = 4, 1024, 512, 64, BF16
    gen = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 16, (K, N), generator=gen, dtype=torch.uint8)
    tid = first_template(bits, 32)
    Q = env.utils.pack(codes.to(d), bits, [tid], env.num_sms)
    table2 = env.utils.make_qmap2_from_qmap(torch.tensor(env.fa.nf_utils.NF4_VALUES, dtype=dtype)).to(d)
    dY = torch.randn(2, 300, N, generator=gen).to(dtype).to(d)
    X = torch.randn(2, 300, K, generator=gen).to(dtype).to(d)
    eager = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)
    for _ in range(3):
        assert torch.equal(env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid).view(torch.int16),
                           eager.view(torch.int16))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)           # warm up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
    empty = env.fa.qgemm_scale_grad(dY[:, :0], X[:, :0], Q, table2, bits, g, tid)
    assert empty.shape == (N, K // g) and not empty.any()


def test_activations_past_2_31_elements(env):
    """M = 65 600, K = 32 768: X holds 2.15e9 elements; rows from 65 536 on start past 2^31.  Sparse exact rows."""
    d = env.dev
    bits, K, N, g, dtype, tile_p = 4, 32768, 128, 64, F16, 32
    M = 65600
    lay = XC.Layer(bits, K, N, g, dtype, seed=77, tile_p=tile_p)
    Q, table2, tid, L = exact_layer(env, lay)
    rows = torch.tensor([0, 1, 31, 65535, 65536, 65537, 65567, 65599], device=d)
    X = torch.zeros(M, K, dtype=dtype, device=d)
    X[rows] = ints(rows.numel(), K, 4, 11, dtype).to(d)
    dY = ints(M, N, 4, 12, dtype).to(d)
    R = exact_reference(dY[rows], X[rows], L, g, dtype)
    for scratch in (None, torch.empty(64 << 20, dtype=torch.uint8, device=d)):
        got = abi(env, dY, X, Q, table2, bits, g, tid, scratch)
        assert XC.exact_equal(got, R, dtype)
    got = env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid)
    assert XC.exact_equal(got, R, dtype)
    del X
    torch.cuda.empty_cache()


def nf4_layer(env, bits, K, N, g, dtype, tile_p, seed):
    d = env.dev
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 2 ** bits, (K, N), generator=gen, dtype=torch.uint8)
    table = torch.tensor(env.fa.nf_utils.NF4_VALUES, dtype=dtype)[:: 16 // 2 ** bits][: 2 ** bits]
    S = (torch.randn(N, K // g, generator=gen) / 8).to(dtype)
    tid = first_template(bits, tile_p)
    Q = env.utils.pack(codes.to(d), bits, [tid], env.num_sms)
    return Q, S.to(d), table.to(d), env.utils.make_qmap2_from_qmap(table).to(d), tid


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_learnable_scales_autograd(env, dtype):
    d = env.dev
    bits, K, N, g = 4, 2048, 1024, 64
    Q, S, table, table2, tid = nf4_layer(env, bits, K, N, g, dtype, 32, seed=5)
    x = torch.randn(3, 40, K, dtype=dtype, device=d)
    dY = torch.randn(3, 40, N, dtype=dtype, device=d)
    for h in (0, 128):
        x0 = x.clone().requires_grad_()
        if h:
            y0 = env.fa.qgemm_hadamard(x0, Q, S, table, table2, env.ws, bits, g, h, tid, env.num_sms)
        else:
            y0 = env.fa.qgemm(x0, Q, S, table, table2, env.ws, bits, g, tid, env.num_sms)
        y0.backward(dY)
        x1 = x.clone().requires_grad_()
        S1 = torch.nn.Parameter(S.clone())
        y1 = env.ln.qgemm_learnable_scales(x1, Q, S1, table, table2, env.ws, bits, g, tid, env.num_sms, h)
        assert torch.equal(y1.detach().view(torch.int16), y0.detach().view(torch.int16))
        y1.add_(1.0)                                                       # the output allows in-place ops
        y1.backward(dY)
        assert torch.equal(x1.grad.view(torch.int16), x0.grad.view(torch.int16)), h
        xs = env.fa.hadamard_transform(x, h) if h else x
        ref = env.fa.qgemm_scale_grad(dY, xs, Q, table2, bits, g, tid, env.num_sms)
        assert torch.equal(S1.grad.view(torch.int16), ref.view(torch.int16)), h
    # scales alone (an input without grad) and refused table gradients
    S2 = torch.nn.Parameter(S.clone())
    env.ln.qgemm_learnable_scales(x, Q, S2, table, table2, env.ws, bits, g, tid, env.num_sms).backward(dY)
    assert torch.equal(S2.grad.view(torch.int16), env.fa.qgemm_scale_grad(dY, x, Q, table2, bits, g, tid).view(torch.int16))
    for t, t2, name in ((table.clone().requires_grad_(), table2, "table"), (table, table2.clone().requires_grad_(), "table2")):
        with pytest.raises(RuntimeError, match=name):
            env.ln.qgemm_learnable_scales(x, Q, S2, t, t2, env.ws, bits, g, tid, env.num_sms)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_matches_dense_fake_quantization(env, dtype):
    """The reference's learnable layer, densely: codes from nf_quantize, scales a Parameter, W_hat = values[codes] *
    scales differentiated by fp64 autograd.  The kernel's gradient agrees within the fp16 / bf16 tolerances."""
    d = env.dev
    bits, K, N, g, M = 4, 1024, 512, 64, 96
    gen = torch.Generator().manual_seed(8)
    Wd = torch.randn(N, K, generator=gen)
    _, idx, absmax, values = env.fa.nf_utils.nf_quantize(Wd, bits, g)
    S = absmax.reshape(N, K // g).to(dtype)
    table = values.to(dtype)
    codes = idx.reshape(N, K).T.contiguous().to(torch.uint8)
    tid = first_template(bits, 32)
    Q = env.utils.pack(codes.to(d), bits, [tid], env.num_sms)
    X = torch.randn(M, K, generator=gen).to(dtype)
    dY = torch.randn(M, N, generator=gen).to(dtype)
    # dense: fp64 autograd through values[codes] * scales (values as the layer holds them, in T)
    Sp = torch.nn.Parameter(S.double())
    What = table.double()[idx.reshape(N, K)] * Sp.repeat_interleave(g, dim=1)
    ((X.double() @ What.T) * dY.double()).sum().backward()
    layer = env.fa.integrations.base.FluteLinear.from_codes(codes.to(d), S.to(d), table.to(d), bits, g, tid)
    holder = torch.nn.Sequential(layer)
    (p,) = env.ln.make_scales_learnable(holder)
    holder(X.to(d)).backward(dY.to(d))
    err = ((p.grad.double().cpu() - Sp.grad).norm() / Sp.grad.norm()).item()
    assert err < TOL[dtype], err


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_reproduces_reference_absmax_grad(env, dtype):
    """The recorded reference gradient (fp64, NF4 values in fp64): the kernel differs only by the table held in T,
    the fp32 arithmetic and the one rounding."""
    d = env.dev
    z = np.load(GOLDEN)
    g = int(z["group_size"])
    codes = torch.from_numpy(z["codes"]).T.contiguous()            # [K, N]
    K, N = codes.shape
    values = torch.from_numpy(z["values"])
    table = values.to(dtype)
    X, dY = torch.from_numpy(z["X"]), torch.from_numpy(z["dY"])
    assert torch.equal(X.to(dtype).double(), X) and torch.equal(dY.to(dtype).double(), dY)
    tid = first_template(4, 32)
    Q = env.utils.pack(codes.to(d), 4, [tid], env.num_sms)
    table2 = env.utils.make_qmap2_from_qmap(table).to(d)
    got = env.fa.qgemm_scale_grad(dY.to(dtype).to(d), X.to(dtype).to(d), Q, table2, 4, g, tid).double().cpu()
    ref = torch.from_numpy(z["grad"])
    n = 16
    pairs = torch.stack([values[:, None].expand(n, n), values[None, :].expand(n, n)], -1).reshape(n * n, 2)
    A = SR.scale_grad(dY, X, SR.lut_of_codes(codes, pairs, 4), g, absolute=True)
    u = XC.U_T[dtype]
    bound = (u + XC.gamma(X.shape[0] * g + 2)) * A * (1 + u) + u * ref.abs()
    assert torch.all((got - ref).abs() <= bound), float(((got - ref).abs() - bound).max())


def test_train_stacked_layers(env):
    """Three stacked FluteLinear layers (bias) learn their scales against a dense teacher: the loss falls, weights
    and tables stay untouched, and the frozen model is plain FluteLinear running flute.qgemm with the learned scales."""
    from flute_amd.integrations.base import FluteLinear
    d = env.dev
    torch.manual_seed(0)
    dtype, bits, g = BF16, 4, 64
    dims = (1024, 1024, 512, 256)
    student, teacher = [], []
    for i in range(3):
        K, N = dims[i], dims[i + 1]
        codes = torch.randint(0, 16, (K, N), dtype=torch.uint8)
        S = (torch.rand(N, K // g) / 16 + 1 / 32).to(dtype).to(d)
        table = torch.tensor(env.fa.nf_utils.NF4_VALUES).to(dtype).to(d)
        bias = (torch.randn(N) / 8).to(dtype).to(d)
        layer = FluteLinear.from_codes(codes, S, table, bits, g, template_id=0, bias=bias)
        layer.requires_grad_(False)
        dense = torch.nn.Linear(K, N, bias=True, device=d, dtype=torch.float32)
        with torch.no_grad():
            S_true = S.float() * (1 + torch.randn_like(S.float()) / 8)
            dense.weight.copy_(env.fa.dequantize(layer.weight, S_true.to(dtype), layer.tables2, bits, g, 0).float())
            dense.bias.copy_(bias.float())
        student.append(layer)
        teacher += [dense]
    model = torch.nn.Sequential(student[0], torch.nn.SiLU(), student[1], torch.nn.SiLU(), student[2])
    dense_model = torch.nn.Sequential(teacher[0], torch.nn.SiLU(), teacher[1], torch.nn.SiLU(), teacher[2])
    keys = set(model.state_dict())
    before = {k: v.clone() for k, v in model.state_dict().items() if not k.endswith("scales") and torch.is_tensor(v)}
    params = env.ln.make_scales_learnable(model)
    assert len(params) == 3 and all(isinstance(m, env.ln.LearnableScalesFluteLinear) for m in model[::2])
    assert model[0].weight is student[0].weight and model[0].tables2 is student[0].tables2
    assert set(model.state_dict()) == keys
    opt = torch.optim.Adam(params, lr=2e-3)
    gen = torch.Generator(d).manual_seed(1)
    losses = []
    for _ in range(12):
        x = torch.randn(256, dims[0], device=d, generator=gen)
        with torch.no_grad():
            target = dense_model(x)
        loss = (model(x.to(dtype)).float() - target).square().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.8 * losses[0], losses
    for k, v in model.state_dict().items():
        if k in before:
            assert torch.equal(v, before[k]), k
    learned = [p.detach().clone() for p in params]
    state = model.state_dict()
    env.ln.freeze_scales(model)
    assert all(type(m) is FluteLinear for m in model[::2])
    assert all(torch.equal(m.scales, s) for m, s in zip(model[::2], learned))
    x = torch.randn(7, dims[0], device=d, dtype=dtype)
    h = x
    for i, m in enumerate(model[::2]):
        h = env.fa.qgemm(h, m.weight, learned[i], m.tables, m.tables2, env.ws, bits, g, 0, env.num_sms) + m.bias
        if i < 2:
            h = torch.nn.functional.silu(h)
    assert torch.equal(model(x).view(torch.int16), h.view(torch.int16))
    plain = torch.nn.Sequential(FluteLinear(dims[0], dims[1], bits, g, 0, bias=True, device=d, dtype=dtype), torch.nn.SiLU(),
                                FluteLinear(dims[1], dims[2], bits, g, 0, bias=True, device=d, dtype=dtype), torch.nn.SiLU(),
                                FluteLinear(dims[2], dims[3], bits, g, 0, bias=True, device=d, dtype=dtype))
    plain.load_state_dict(state)
    assert torch.equal(plain(x).view(torch.int16), h.view(torch.int16))
    again = env.ln.make_scales_learnable(plain)
    plain.load_state_dict(model.state_dict())                 # and back into learnable layers
    assert all(torch.equal(p, s) for p, s in zip(again, learned))
