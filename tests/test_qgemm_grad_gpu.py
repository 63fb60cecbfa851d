"""Backpropagation through flute::qgemm_raw_simple[_hadamard]: the input gradient dX = dY @ dequantize(...) (then the
rotation), exact on exactly representable data, within the forward's tolerances on random data, through stacked
FluteLinear layers with LoRA adapters, with the forward unchanged and scale gradients refused."""
import pytest
import torch

from tests import exact_cases as XC
from tests.support import env, first_template, fp32_blas_reduction  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 1e-3, BF16: 4e-3}


def norm_rel_err64(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


EXACT = [
    (4, 4096, 1024, 64, F16, 32, False, (7,)), (4, 2048, 2048, 128, BF16, 64, True, (3, 5)),
    (3, 2048, 1024, 64, F16, 32, True, (9,)), (3, 1024, 512, 32, BF16, 32, False, (2, 4)),
    (2, 2048, 1024, 256, F16, 64, False, (2, 33)), (2, 1024, 512, 64, BF16, 32, True, (17,)),
    (4, 1024, 512, 64, BF16, 32, False, (70,)), (2, 4096, 2048, 128, BF16, 32, False, (5,)),
    (4, 8192, 28672, 64, F16, 32, False, (8,)),            # 470 MB dense: four K chunks of the 128 MiB scratch
]


@pytest.mark.parametrize("bits,K,N,g,dtype,tile_p,pair,shape", EXACT)
def test_exact_input_grad(env, bits, K, N, g, dtype, tile_p, pair, shape):
    """Integer dY in [-4, 4] against exact weights: x.grad must be round_T(dY @ W_exact^T) bit for bit."""
    d = env.dev
    lay = XC.Layer(bits, K, N, g, dtype, seed=bits * 7919 + K + N + g, tile_p=tile_p, pair=pair)
    tid = first_template(bits, tile_p)
    Q = env.utils.pack(lay.W.to(d), bits, [tid], env.num_sms)
    S, table, table2 = lay.S.to(d), lay.table.to(d), lay.table2.to(d)
    M = 1
    for s in shape:
        M *= s
    dY = XC.make_x(M, N, seed=K + M, dtype=dtype, witness=False).to(d)
    x = XC.make_x(M, K, seed=N + M, dtype=dtype, witness=False).to(d).reshape(*shape, K).requires_grad_()
    # premise of the N reduction: integer dY times multiples of 2^-3, every partial sum below 2^21
    R = torch.empty(M, K, dtype=torch.float64, device=d)
    A = torch.empty(M, K, dtype=torch.float64, device=d)
    dy64 = dY.double()
    for n0 in range(0, N, 4096):
        n1 = min(N, n0 + 4096)
        W = lay.w_exact(n0, n1, device=d)                       # [K, n] fp64, exact
        if n0 == 0:
            assert torch.equal(W.to(dtype).double(), W) and torch.equal(W * 8, (W * 8).round())
            R.copy_(dy64[:, n0:n1] @ W.T)
            A.copy_(dy64[:, n0:n1].abs() @ W.abs().T)
        else:
            R += dy64[:, n0:n1] @ W.T
            A += dy64[:, n0:n1].abs() @ W.abs().T
        del W
    assert float(A.max()) < XC.EXACT_SUM_LIMIT
    assert torch.isfinite(R.to(dtype)).all()
    with fp32_blas_reduction():
        y = env.fa.qgemm(x, Q, S, table, table2, env.ws, bits, g, tid, env.num_sms)
        assert y.shape == (*shape, N)
        y.backward(dY.reshape(*shape, N))
    assert x.grad.shape == x.shape and x.grad.dtype == dtype
    assert XC.exact_equal(x.grad.reshape(M, K), R, dtype)
    del Q, x, y, R, A
    torch.cuda.empty_cache()


def random_layer(env, bits, K, N, g, dtype, tile_p, seed):
    from oracle import flute_oracle as O
    gen = torch.Generator().manual_seed(seed)
    W = torch.randint(0, 2 ** bits, (K, N), generator=gen, dtype=torch.uint8)
    S = (torch.randn(N, K // g, generator=gen) / 8).to(dtype)
    table = torch.tensor(O.NF4_VALUES, dtype=dtype)[:: 16 // 2 ** bits][: 2 ** bits]
    table2 = O.make_qmap2_from_qmap(table)
    Q = torch.from_numpy(O.pack(W.numpy(), bits, tile_p))
    What = O.dequantize(Q.numpy(), S, table2, bits, g, tile_p)      # [K, N] in T: the weight the kernels use
    return Q, S, table, table2, What


@pytest.mark.parametrize("bits,K,N,g,dtype,tile_p,M", [
    (4, 4096, 2048, 64, F16, 32, 40), (4, 2048, 1024, 128, BF16, 64, 3), (3, 2048, 1024, 64, BF16, 32, 129),
    (2, 1024, 2048, 32, F16, 64, 8)])
def test_random_input_grad(env, bits, K, N, g, dtype, tile_p, M):
    d = env.dev
    Q, S, table, table2, What = random_layer(env, bits, K, N, g, dtype, tile_p, seed=K + N + M)
    tid = first_template(bits, tile_p)
    x = torch.randn(M, K, dtype=dtype, device=d).requires_grad_()
    dY = torch.randn(M, N, dtype=dtype)
    y = env.fa.qgemm(x, Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, tid, env.num_sms)
    y.backward(dY.to(d))
    ref = dY.double() @ What.double().T
    assert norm_rel_err64(x.grad, ref) < TOL[dtype]


@pytest.mark.parametrize("h", [64, 128, 512])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_random_input_grad_hadamard(env, h, dtype):
    d = env.dev
    bits, K, N, g, tile_p = 4, 2048, 1024, 64, 32
    Q, S, table, table2, What = random_layer(env, bits, K, N, g, dtype, tile_p, seed=h)
    tid = first_template(bits, tile_p)
    for shape in ((1,), (6,), (2, 70)):
        x = torch.randn(*shape, K, dtype=dtype, device=d).requires_grad_()
        dY = torch.randn(*shape, N, dtype=dtype)
        y = env.fa.qgemm_hadamard(x, Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, h, tid, env.num_sms)
        y.backward(dY.to(d))
        ref = env.O.hadamard_transform((dY.double().reshape(-1, N) @ What.double().T), h).reshape(*shape, K)
        assert x.grad.shape == x.shape
        assert norm_rel_err64(x.grad, ref) < TOL[dtype], (shape, norm_rel_err64(x.grad, ref))


def test_non_contiguous_grad_output(env):
    d = env.dev
    bits, K, N, g, dtype, tile_p = 4, 1024, 512, 64, F16, 32
    Q, S, table, table2, What = random_layer(env, bits, K, N, g, dtype, tile_p, seed=4)
    tid = first_template(bits, tile_p)
    x = torch.randn(5, K, dtype=dtype, device=d).requires_grad_()
    y = env.fa.qgemm(x, Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, tid, env.num_sms)
    dY = torch.randn(N, 5, dtype=dtype, device=d).T               # transposed: non-contiguous
    y.backward(dY)
    assert norm_rel_err64(x.grad, dY.cpu().double() @ What.double().T) < TOL[dtype]
    x.grad = None
    y = env.fa.qgemm(x, Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, tid, env.num_sms)
    y.sum().backward()                                            # an expanded (stride 0) gradient
    assert norm_rel_err64(x.grad, torch.ones(5, N).double() @ What.double().T) < TOL[dtype]


def test_lora_adapters_on_stacked_flute_linear(env):
    """Two FluteLinear layers (bias) with trainable LoRA adapters against dense nn.Linear layers holding
    dequantize(...): every adapter's gradient (the lower layer's needs the gradient through the upper quantized layer)."""
    from flute_amd.integrations.base import FluteLinear
    d = env.dev
    torch.manual_seed(0)
    dtype, bits, g, r = F16, 4, 64, 8
    dims = (1024, 2048, 512)
    bases, denses = [], []
    for i in range(2):
        K, N = dims[i], dims[i + 1]
        codes = torch.randint(0, 16, (K, N), dtype=torch.uint8)
        S = (torch.randn(N, K // g) / 16).to(dtype).to(d)
        table = torch.tensor(env.O.NF4_VALUES).to(dtype).to(d)
        bias = torch.randn(N).to(dtype).to(d)
        base = FluteLinear.from_codes(codes, S, table, bits, g, template_id=0, bias=bias)
        base.requires_grad_(False)
        dense = torch.nn.Linear(K, N, bias=True, device=d, dtype=dtype)
        with torch.no_grad():
            dense.weight.copy_(env.fa.dequantize(base.weight, base.scales, base.tables2, bits, g, base.template_id))
            dense.bias.copy_(base.bias)
        dense.requires_grad_(False)
        bases.append(base)
        denses.append(dense)
    lora = [(torch.randn(r, dims[i], device=d, dtype=dtype) / 32, torch.randn(dims[i + 1], r, device=d, dtype=dtype) / 8)
            for i in range(2)]

    def run(layers):
        params = [(a.clone().requires_grad_(), b.clone().requires_grad_()) for a, b in lora]
        h = torch.randn(6, 3, dims[0], device=d, dtype=dtype, generator=torch.Generator(d).manual_seed(1))
        for layer, (A, B) in zip(layers, params):
            h = layer(h) + (h @ A.T) @ B.T
            h = torch.nn.functional.silu(h)
        h.float().square().mean().backward()
        return [p.grad for ab in params for p in ab]

    got, ref = run(bases), run(denses)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a is not None and norm_rel_err64(a, b) < 1e-2, (i, norm_rel_err64(a, b))


@pytest.mark.parametrize("M", [1, 4, 33, 600])
def test_forward_unchanged_by_requires_grad(env, M):
    d = env.dev
    bits, K, N, g, dtype, tile_p = 4, 2048, 2048, 64, BF16, 32
    Q, S, table, table2, _ = random_layer(env, bits, K, N, g, dtype, tile_p, seed=M)
    args = (Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, first_template(bits, tile_p), env.num_sms)
    x = torch.randn(M, K, dtype=dtype, device=d)
    with torch.no_grad():
        y0 = env.fa.qgemm(x, *args)
    y1 = env.fa.qgemm(x.clone().requires_grad_(), *args)
    assert y1.requires_grad and torch.equal(y0.view(torch.int16), y1.detach().view(torch.int16))
    hargs = args[:7] + (128,) + args[7:]
    with torch.no_grad():
        h0 = env.fa.qgemm_hadamard(x, *hargs)
    h1 = env.fa.qgemm_hadamard(x.clone().requires_grad_(), *hargs)
    assert torch.equal(h0.view(torch.int16), h1.detach().view(torch.int16))


def test_scale_and_table_gradients_refused(env):
    d = env.dev
    bits, K, N, g, dtype, tile_p = 4, 1024, 512, 64, F16, 32
    Q, S, table, table2, _ = random_layer(env, bits, K, N, g, dtype, tile_p, seed=9)
    tid = first_template(bits, tile_p)
    Sd = S.to(d).requires_grad_()
    x = torch.randn(3, K, dtype=dtype, device=d)
    y = env.fa.qgemm(x, Q.to(d), Sd, table.to(d), table2.to(d), env.ws, bits, g, tid, env.num_sms)
    with pytest.raises(RuntimeError, match="scales"):
        y.sum().backward()
    assert Sd.grad is None
    xg = x.clone().requires_grad_()
    t2 = table2.to(d).requires_grad_()
    y = env.fa.qgemm_hadamard(xg, Q.to(d), S.to(d), table.to(d), t2, env.ws, bits, g, 64, tid, env.num_sms)
    with pytest.raises(RuntimeError, match="table2"):
        y.sum().backward()
    assert t2.grad is None
