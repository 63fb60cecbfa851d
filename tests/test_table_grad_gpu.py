"""The lookup-table gradient of packed layers on the GPU: flute_amd.qgemm_table_grad (param_grad.hip) bit for bit on
exactly representable data, within the componentwise bound gamma(d) on random data, its fused scale gradient equal to
qgemm_scale_grad's, reproducible over repeated calls and graph replay, past 2^31 activation elements;
qgemm_learnable / LearnableFluteLinear through autograd against a dense fp64 model and the reference's recorded
values gradient, a short training run, and freeze."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import exact_cases as XC
from tests import scale_grad_ref as SR
from tests import table_grad_ref as TR
from tests.grouped_cases import exact_inputs, exact_premise, exact_scales
from tests.support import env, first_template  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "table_grad", "manual_nf4_values_grad.npz")
# ---------------------------------------------------------------------------
# exactly representable data
# ---------------------------------------------------------------------------

def exact_shape(bits, g, tile_p):
    """(K, N) of a case.  N: the smallest the layout packs (3 bits: 512), or three column blocks of it.  K by group size;
    a workgroup owns 256 k, so K % 256 != 0 leaves a last block whose columns past K are the zero-filled tail:
      g = 32:  448  = 256 + 192   tail block, 14 groups
      g = 64:  3584 = 14 x 256    whole blocks only, no tail; at 2 bits 320 = 256 + 64: tail block, 5 groups
      g = 128: 1152 = 4 x 256 + 128   tail block, 9 groups
      g = 256: 768  = 3 x 256     whole blocks only (g = 256 allows no tail), 3 groups"""
    K = {32: 448, 64: 3584 if bits != 2 else 320, 128: 1152, 256: 768}[g]
    N = XC.cols_per_block(bits, tile_p) * (3 if bits == 4 and tile_p == 32 else 1)
    return K, N


EXACT = [(b, g, dt, tp, pair) for b, g, dt, tp, pair in
         itertools.product((2, 3, 4), (32, 64, 128, 256), (F16, BF16), (32, 64), (False, True)) if not (b == 3 and tp == 64)]
EXACT_MS = (5, 77, 300)          # 300 rows: 10 steps of 32, which these small layers split in two


def exact_case(bits, g, dtype, tile_p, pair):
    K, N = exact_shape(bits, g, tile_p)
    lay = XC.Layer(bits, K, N, g, dtype, seed=bits * 131 + K + N + g + tile_p, tile_p=tile_p, pair=pair)
    S = exact_scales(N, K // g, dtype, seed=K + N)
    return lay, S


@pytest.mark.parametrize("bits,g,dtype,tile_p,pair", EXACT)
def test_exact(env, bits, g, dtype, tile_p, pair):
    d = env.dev
    lay, S = exact_case(bits, g, dtype, tile_p, pair)
    K, N = lay.K, lay.N
    tid = first_template(bits, tile_p)
    codes = lay.W.to(d)
    Q = env.utils.pack(codes, bits, [tid], env.num_sms)
    table2 = lay.table2.to(d)
    L = SR.lut_of_codes(codes, lay.pairs, bits)
    S = S.to(d)
    n = 2 ** bits
    for M in EXACT_MS:
        X, dY = (t.to(d) for t in exact_inputs(M, K, N, dtype, seed=M + K))
        R, Rs = exact_premise(X, dY, S, codes, L, bits, g, dtype)
        got = env.fa.qgemm_table_grad(dY, X, Q, S, bits, g, tid)
        assert got.shape == (n, n, 2) and got.dtype == torch.float32
        assert torch.equal(got.double().reshape(-1, 2), R), (M, float((got.double().reshape(-1, 2) - R).abs().max()))
        got2, dS = env.fa.qgemm_table_grad(dY, X, Q, S, bits, g, tid, table2=table2, with_scale_grad=True)
        assert torch.equal(got2, got)
        assert dS.shape == (N, K // g) and dS.dtype == dtype
        assert XC.exact_equal(dS, Rs, dtype), M
        assert torch.equal(dS.view(torch.int16), env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid).view(torch.int16))
        if not pair:
            folded = env.fa.pair_grad_to_table_grad(got.double())             # in fp64: 2^(b + 1) bins may pass 2^24 quanta
            assert torch.equal(folded, TR.to_scalar(R, bits))


# ---------------------------------------------------------------------------
# random data
# ---------------------------------------------------------------------------

def random_layer(env, bits, K, N, g, dtype, tile_p, seed):
    d = env.dev
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 2 ** bits, (K, N), generator=gen, dtype=torch.uint8)
    table = torch.tensor(env.fa.nf_utils.NF4_VALUES, dtype=dtype)[:: 16 // 2 ** bits][: 2 ** bits]
    S = (torch.randn(N, K // g, generator=gen) / 8).to(dtype)
    tid = first_template(bits, tile_p)
    Q = env.utils.pack(codes.to(d), bits, [tid], env.num_sms)
    return codes.to(d), Q, S.to(d), table.to(d), env.utils.make_qmap2_from_qmap(table).to(d), tid


RANDOM = [(4, 4096, 1024, 64, F16, 32, 600), (4, 2048, 2048, 128, BF16, 64, 77), (3, 2048, 1024, 64, BF16, 32, 1000),
          (2, 1024, 2048, 32, F16, 64, 3), (4, 1024, 1024, 256, BF16, 32, 4096), (2, 3584, 512, 64, BF16, 32, 2100)]


@pytest.mark.parametrize("bits,K,N,g,dtype,tile_p,M", RANDOM)
def test_random_within_componentwise_bound(env, bits, K, N, g, dtype, tile_p, M):
    """|dT2 - exact| <= gamma_fp32(d) sum |dY X S|, bin by bin: d = table_grad_ref.chain_depth(M) is the longest chain
    of fp32 roundings one term passes through (param_grad.hip's header), well inside M + 2 + 32768.  The fused scale
    gradient equals qgemm_scale_grad's bit for bit on the same data."""
    d = env.dev
    codes, Q, S, table, table2, tid = random_layer(env, bits, K, N, g, dtype, tile_p, seed=K + N + M)
    gen = torch.Generator().manual_seed(M)
    dY = torch.randn(M, N, generator=gen).to(dtype).to(d)
    X = torch.randn(M, K, generator=gen).to(dtype).to(d)
    depth = TR.chain_depth(M)
    assert depth <= M + 2 + 32768
    got, dS = env.fa.qgemm_table_grad(dY, X, Q, S, bits, g, tid, table2=table2, with_scale_grad=True)
    R = TR.table_grad(dY, X, codes, S, bits, g)
    A = TR.table_grad(dY, X, codes, S, bits, g, absolute=True)
    err = (got.double().reshape(-1, 2) - R).abs()
    bound = XC.gamma(depth) * A
    print("table grad", (bits, K, N, g, M), "max err / bound", float((err / bound.clamp_min(1e-300)).max()))
    assert torch.all(err <= bound), float((err - bound).max())
    assert torch.equal(env.fa.qgemm_table_grad(dY, X, Q, S, bits, g, tid), got)        # table only: the same bits
    assert torch.equal(dS.view(torch.int16), env.fa.qgemm_scale_grad(dY, X, Q, table2, bits, g, tid).view(torch.int16))


REPRO = [(2, 1024, 512, 64, BF16, 32, 600),        # 16 pair indices: most lanes of a wave meet on a bin
         (4, 1024, 512, 64, F16, 32, 600), (3, 1152, 512, 128, BF16, 32, 77)]


@pytest.mark.parametrize("bits,K,N,g,dtype,tile_p,M", REPRO)
def test_reproducible(env, bits, K, N, g, dtype, tile_p, M):
    """The same arguments 20 times, eagerly and in a replayed graph: the same bits every time.  This is the gate for
    adding into the wave's LDS bins with ds_add_f32 (lanes of one instruction that meet on a bin)."""
    d = env.dev
    codes, Q, S, table, table2, tid = random_layer(env, bits, K, N, g, dtype, tile_p, seed=bits)
    gen = torch.Generator().manual_seed(M + bits)
    dY = torch.randn(M, N, generator=gen).to(dtype).to(d)
    X = torch.randn(M, K, generator=gen).to(dtype).to(d)

    def run():
        return env.fa.qgemm_table_grad(dY, X, Q, S, bits, g, tid, table2=table2, with_scale_grad=True)
    first, first_s = run()
    for _ in range(19):
        t, s = run()
        assert torch.equal(t, first) and torch.equal(s.view(torch.int16), first_s.view(torch.int16))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                              # warm up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t, s = run()
    for _ in range(20):
        t.zero_()
        s.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(t, first) and torch.equal(s.view(torch.int16), first_s.view(torch.int16))
    empty, empty_s = env.fa.qgemm_table_grad(dY[:0], X[:0], Q, S, bits, g, tid, table2=table2, with_scale_grad=True)
    assert empty.shape == first.shape and not empty.any() and empty_s.shape == first_s.shape and not empty_s.any()


def test_activations_past_2_31_elements(env):
    """M = 65 600, K = 32 768: X holds 2.15e9 elements; rows from 65 536 on start past 2^31.  Sparse exact rows."""
    d = env.dev
    bits, K, N, g, dtype, tile_p = 4, 32768, 128, 64, F16, 32
    M = 65600
    lay = XC.Layer(bits, K, N, g, dtype, seed=77, tile_p=tile_p)
    tid = first_template(bits, tile_p)
    codes = lay.W.to(d)
    Q = env.utils.pack(codes, bits, [tid], env.num_sms)
    L = SR.lut_of_codes(codes, lay.pairs, bits)
    S = exact_scales(N, K // g, dtype, seed=3).to(d)
    rows = torch.tensor([0, 1, 31, 65535, 65536, 65537, 65567, 65599], device=d)
    Xr, dYr = (t.to(d) for t in exact_inputs(rows.numel(), K, N, dtype, seed=11))
    X = torch.zeros(M, K, dtype=dtype, device=d)
    X[rows] = Xr
    dY = (torch.randint(-4, 5, (M, N), generator=torch.Generator().manual_seed(12)).double() / 4).to(dtype).to(d)
    R, Rs = exact_premise(X[rows], dY[rows], S, codes, L, bits, g, dtype)
    got, dS = env.fa.qgemm_table_grad(dY, X, Q, S, bits, g, tid, table2=lay.table2.to(d), with_scale_grad=True)
    assert torch.equal(got.double().reshape(-1, 2), R)
    assert XC.exact_equal(dS, Rs, dtype)
    del X
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# autograd: qgemm_learnable, LearnableFluteLinear, freeze
# ---------------------------------------------------------------------------

def rel(got, ref):
    return ((got.double().cpu() - ref.double().cpu()).norm() / ref.double().norm()).item()


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("form,h", [("scalar", 0), ("pair", 0), ("scalar", 128)])
def test_learnable_matches_dense_autograd(env, dtype, form, h):
    """qgemm_learnable against fp64 autograd through W_hat = pairs[idx] * scales on the values the layer holds (table
    and scales in T).  Norm-wise, to first order, each rounding to T of a whole operand or result costs at most u_T:
    dS passes two (the rotated input under a Hadamard size, its own output), the codebook gradient at most that, dX
    four (the dequantized weight, the product, the rotation in and out)."""
    d = env.dev
    bits, K, N, g, M = 4, 1024, 512, 64, 96
    n = 2 ** bits
    u = XC.U_T[dtype]
    codes, Q, S, table, table2, tid = random_layer(env, bits, K, N, g, dtype, 32, seed=8)
    gen = torch.Generator().manual_seed(9)
    if form == "pair":
        master = (torch.randn(n, n, 2, generator=gen) / 2).to(dtype).float().to(d)     # values T holds
    else:
        master = table.float()
    x = torch.randn(M, K, generator=gen).to(dtype).to(d)
    dY = torch.randn(M, N, generator=gen).to(dtype).to(d)
    # dense
    leaf = master.double().clone().requires_grad_()
    Sp = S.double().clone().requires_grad_()
    xp = x.double().clone().requires_grad_()
    pairs = leaf.reshape(n * n, 2) if form == "pair" else \
        torch.stack([leaf[:, None].expand(n, n), leaf[None, :].expand(n, n)], -1).reshape(n * n, 2)
    Lk = pairs[TR.pair_index(codes, bits)].permute(0, 2, 1).reshape(K, N)
    What = Lk * Sp.repeat_interleave(g, dim=1).T
    xr = xp
    if h:
        H = torch.ones(1, 1, dtype=torch.float64, device=d)
        while H.shape[0] < h:
            H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
        xr = (xp.reshape(-1, h) @ (H / h ** 0.5)).reshape(M, K)
    ((xr @ What) * dY.double()).sum().backward()
    # the layer
    x1 = x.clone().requires_grad_()
    S1 = torch.nn.Parameter(S.clone())
    cb = torch.nn.Parameter(master.clone())
    y = env.ln.qgemm_learnable(x1, Q, S1, cb, env.ws, bits, g, tid, env.num_sms, h)
    t1, t2 = env.ln._codebook_tables(cb, bits, dtype)
    x0 = x.clone().requires_grad_()
    y0 = env.fa.qgemm_hadamard(x0, Q, S, t1, t2, env.ws, bits, g, h, tid, env.num_sms) if h else \
        env.fa.qgemm(x0, Q, S, t1, t2, env.ws, bits, g, tid, env.num_sms)
    assert torch.equal(y.detach().view(torch.int16), y0.detach().view(torch.int16))
    y.add_(1.0)                                                            # the output allows in-place ops
    y.backward(dY)
    y0.backward(dY)
    assert torch.equal(x1.grad.view(torch.int16), x0.grad.view(torch.int16))           # the op's own Autograd kernel
    assert cb.grad.dtype == torch.float32 and cb.grad.shape == master.shape and S1.grad.dtype == dtype
    errs = rel(x1.grad, xp.grad), rel(S1.grad, Sp.grad), rel(cb.grad, leaf.grad)
    print("learnable", form, h, str(dtype), "rel errors dX dS dcodebook", errs, "u_T", u)
    assert errs[0] < 4 * u and errs[1] < 2 * u and errs[2] < 2 * u, errs
    # one fused call gave both; each alone gives the same bits
    xs = env.fa.hadamard_transform(x, h) if h else x
    assert torch.equal(S1.grad.view(torch.int16), env.fa.qgemm_scale_grad(dY, xs, Q, t2, bits, g, tid, env.num_sms).view(torch.int16))
    dT2 = env.fa.qgemm_table_grad(dY, xs, Q, S, bits, g, tid, env.num_sms)
    assert torch.equal(cb.grad, dT2 if form == "pair" else env.fa.pair_grad_to_table_grad(dT2))
    # scales alone, codebook alone
    S2 = torch.nn.Parameter(S.clone())
    env.ln.qgemm_learnable(x, Q, S2, master, env.ws, bits, g, tid, env.num_sms, h).backward(dY)
    assert torch.equal(S2.grad.view(torch.int16), S1.grad.view(torch.int16))
    cb2 = torch.nn.Parameter(master.clone())
    env.ln.qgemm_learnable(x, Q, S, cb2, env.ws, bits, g, tid, env.num_sms, h).backward(dY)
    assert torch.equal(cb2.grad, cb.grad)


def test_learnable_refusals(env):
    d = env.dev
    bits, K, N, g = 4, 512, 256, 64
    codes, Q, S, table, table2, tid = random_layer(env, bits, K, N, g, F16, 32, seed=1)
    x = torch.randn(4, K, dtype=F16, device=d)
    with pytest.raises(TypeError, match="fp32"):
        env.ln.qgemm_learnable(x, Q, S, table, env.ws, bits, g, tid, env.num_sms)          # a codebook in T
    for shape in ((8,), (16, 16), (16, 16, 1), (4, 4, 2)):
        with pytest.raises(ValueError, match="codebook"):
            env.ln.qgemm_learnable(x, Q, S, torch.zeros(shape, device=d), env.ws, bits, g, tid, env.num_sms)
    from flute_amd.integrations.base import FluteLinear
    layer = FluteLinear.from_codes(codes, S, table, bits, g, tid)
    with pytest.raises(ValueError, match="table"):
        env.ln.LearnableFluteLinear(layer, table="vector")
    layer.tables2.copy_(layer.tables2.flip(0))                              # no longer the pair table of `tables`
    with pytest.raises(ValueError, match="pair"):
        env.ln.LearnableFluteLinear(layer, table="scalar")
    assert env.ln.LearnableFluteLinear(layer, table="pair").codebook.shape == (16, 16, 2)
    # the scales-only surface keeps refusing table gradients
    with pytest.raises(RuntimeError, match="table2"):
        env.ln.qgemm_learnable_scales(x, Q, S, table, table2.clone().requires_grad_(), env.ws, bits, g, tid, env.num_sms)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_reproduces_reference_values_grad(env, dtype):
    """The recorded reference gradient of `values` (fp64, absmax in fp64): the kernel differs by the scales held in T
    (u_T on every term), its fp32 arithmetic (gamma(d)) and the fold onto the scalar table (2^5 fp32 additions)."""
    d = env.dev
    z = np.load(GOLDEN)
    g = int(z["group_size"])
    codes = torch.from_numpy(z["codes"]).T.contiguous()            # [K, N]
    K, N = codes.shape
    X, dY, absmax = torch.from_numpy(z["X"]), torch.from_numpy(z["dY"]), torch.from_numpy(z["absmax"])
    assert torch.equal(X.to(dtype).double(), X) and torch.equal(dY.to(dtype).double(), dY)
    tid = first_template(4, 32)
    Q = env.utils.pack(codes.to(d), 4, [tid], env.num_sms)
    dT2 = env.fa.qgemm_table_grad(dY.to(dtype).to(d), X.to(dtype).to(d), Q, absmax.to(dtype).to(d), 4, g, tid)
    got = env.fa.pair_grad_to_table_grad(dT2).double().cpu()
    ref = torch.from_numpy(z["values_grad"])
    A = TR.to_scalar(TR.table_grad(dY, X, codes, absmax, 4, g, absolute=True), 4)
    u = XC.U_T[dtype]
    bound = (u + XC.gamma(TR.chain_depth(X.shape[0]) + 32)) * A * (1 + u)
    assert got.shape == ref.shape
    assert torch.all((got - ref).abs() <= bound), float(((got - ref).abs() - bound).max())


def test_train_stacked_layers_and_freeze(env):
    """Three stacked FluteLinear layers (bias) learn scales and tables against a dense teacher whose table and scales
    differ: the loss falls, the packed weights stay untouched, and freeze leaves plain FluteLinears whose output is
    the learnable layers' last forward bit for bit, with FluteLinear's state-dict keys."""
    from flute_amd.integrations.base import FluteLinear
    d = env.dev
    torch.manual_seed(0)
    dtype, bits, g = BF16, 4, 64
    dims = (1024, 1024, 512, 256)
    student, teacher = [], []
    nf4 = torch.tensor(env.fa.nf_utils.NF4_VALUES)
    for i in range(3):
        K, N = dims[i], dims[i + 1]
        codes = torch.randint(0, 16, (K, N), dtype=torch.uint8)
        S = (torch.rand(N, K // g) / 16 + 1 / 32).to(dtype).to(d)
        bias = (torch.randn(N) / 8).to(dtype).to(d)
        layer = FluteLinear.from_codes(codes, S, nf4.to(dtype).to(d), bits, g, template_id=0, bias=bias)
        layer.requires_grad_(False)
        dense = torch.nn.Linear(K, N, bias=True, device=d, dtype=torch.float32)
        with torch.no_grad():
            S_true = S.float() * (1 + torch.randn_like(S.float()) / 8)
            t_true = (nf4 * (1 + torch.randn(16) / 8) + torch.randn(16) / 32).to(dtype).to(d)
            dense.weight.copy_(env.fa.dequantize(layer.weight, S_true.to(dtype), env.utils.make_qmap2_from_qmap(t_true), bits, g, 0).float())
            dense.bias.copy_(bias.float())
        student.append(layer)
        teacher.append(dense)
    model = torch.nn.Sequential(student[0], torch.nn.SiLU(), student[1], torch.nn.SiLU(), student[2])
    dense_model = torch.nn.Sequential(teacher[0], torch.nn.SiLU(), teacher[1], torch.nn.SiLU(), teacher[2])
    keys = set(model.state_dict())
    weights = [m.weight.clone() for m in student]
    tables0 = [m.tables.clone() for m in student]
    params = env.ln.make_learnable(model, scales=True, table="scalar")
    assert len(params) == 6 and all(isinstance(m, env.ln.LearnableFluteLinear) for m in model[::2])
    assert [p.dtype for p in params] == [dtype, torch.float32] * 3 and [p.ndim for p in params] == [2, 1] * 3
    assert model[0].weight is student[0].weight
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
    assert all(torch.equal(m.weight, w) for m, w in zip(model[::2], weights))
    assert all(not torch.equal(m.codebook.detach().to(dtype), t) for m, t in zip(model[::2], tables0))     # the tables moved
    x = torch.randn(7, dims[0], device=d, dtype=dtype)
    with torch.no_grad():
        last = model(x)
    learned = [(m.scales.detach().clone(), m.codebook.detach().clone()) for m in model[::2]]
    env.ln.freeze(model)
    assert all(type(m) is FluteLinear for m in model[::2])
    assert set(model.state_dict()) == keys
    for m, (s, c), t0 in zip(model[::2], learned, tables0):
        assert torch.equal(m.scales, s) and m.scales.dtype == dtype
        assert torch.equal(m.tables, c.to(dtype)) and torch.equal(m.tables2, env.utils.make_qmap2_from_qmap(c.to(dtype)))
    assert all(torch.equal(s.tables, t0) for s, t0 in zip(student, tables0))                # the source layers' buffers were not written
    assert torch.equal(model(x).view(torch.int16), last.view(torch.int16))
    plain = torch.nn.Sequential(FluteLinear(dims[0], dims[1], bits, g, 0, bias=True, device=d, dtype=dtype), torch.nn.SiLU(),
                                FluteLinear(dims[1], dims[2], bits, g, 0, bias=True, device=d, dtype=dtype), torch.nn.SiLU(),
                                FluteLinear(dims[2], dims[3], bits, g, 0, bias=True, device=d, dtype=dtype))
    plain.load_state_dict(model.state_dict())
    assert torch.equal(plain(x).view(torch.int16), last.view(torch.int16))
    # a pair codebook trains and freezes the same way; table=None trains the scales alone
    holder = torch.nn.Sequential(plain[0])
    (cb,) = env.ln.make_learnable(holder, scales=False, table="pair")
    assert cb.shape == (16, 16, 2) and cb.dtype == torch.float32
    holder(x).float().square().mean().backward()
    assert cb.grad is not None and cb.grad.abs().sum() > 0 and holder[0].scales.grad is None
    with torch.no_grad():
        cb.add_(cb.grad.sign() / 64)
        moved = holder(x)
    env.ln.freeze(holder)
    assert type(holder[0]) is FluteLinear and torch.equal(holder(x).view(torch.int16), moved.view(torch.int16))
    assert torch.equal(holder[0].tables2, cb.detach().to(dtype).contiguous().view(torch.float32))
    (sc,) = env.ln.make_learnable(holder, scales=True, table=None)
    assert sc.dtype == dtype and "0.codebook" not in holder.state_dict()
    holder(x).float().square().mean().backward()
    assert sc.grad is not None and [k for k, _ in holder.named_parameters()] == ["0.scales", "0.bias"]
