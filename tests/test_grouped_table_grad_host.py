"""flute_qgemm_grouped_table_grad, its scratch query, its Python wrapper, the learnable grouped entry points with a
codebook and the expert modules without a GPU: the export, every refusal of the C ABI in its documented order (returned
before anything is enqueued, on null or host pointers), the scratch formula, every branch of the wrapper's validator on
meta tensors, the refusals around autograd, the batched table2 builder against make_qmap2_from_qmap, and
make_experts_learnable(table=...) / freeze_experts on modules built on the CPU."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind


def header_value(name):
    with open(HEADER) as f:
        for line in f:
            parts = line.replace(",", " ").replace("=", " ").split()
            if name in parts:
                return int(parts[parts.index(name) + 1])
    raise KeyError(name)


ERR_WORKSPACE = header_value("FLUTE_ERR_WORKSPACE")


def query(bits=4, g=64, E=4, N=1024, K=512):
    return _lib.get().flute_qgemm_grouped_table_grad_scratch_bytes(bits, g, E, N, K)


def tgrad(dtype=0, bits=4, g=64, E=4, R=8, N=1024, K=512, P=None, tid=0, ptrs=(None,) * 10, nbytes=None, num_sms=256):
    """ptrs: dY, X, offsets, Q, S, QM2, row_weight, dT2, dS, scratch"""
    P = bits * N // 16 if P is None else P
    nbytes = max(query(bits, g, E, N, K), 1) if nbytes is None else nbytes
    return _lib.get().flute_qgemm_grouped_table_grad(dtype, bits, g, E, R, N, K, P, tid, *ptrs, nbytes, num_sms, None)


def test_symbols_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    for name in ("flute_qgemm_grouped_table_grad", "flute_qgemm_grouped_table_grad_scratch_bytes"):
        assert name in _lib.SYMBOLS
        getattr(_lib.get(), name)
    assert "int flute_qgemm_grouped_table_grad(" in text
    assert "size_t flute_qgemm_grouped_table_grad_scratch_bytes(int num_bits, int group_size, int E, int N, int K);" in text
    assert "flute_qgemm_grouped_table_grad and its scratch query" in text          # the "9:" history
    assert "235 MB" in text                                                        # what the scratch costs at a large stack
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_grouped_table_grad is flute_amd.ops.qgemm_grouped_table_grad
    assert flute_amd.grouped_pair_grad_to_table_grad is flute_amd.ops.grouped_pair_grad_to_table_grad


def test_layer_and_shape_refusals_with_null_and_host_pointers():
    for ptrs in ((None,) * 10, (FAKE,) * 10):                      # refused before any pointer is looked at or behind
        kw = dict(ptrs=ptrs)
        assert tgrad(dtype=2, **kw) == ERR_DTYPE
        assert tgrad(bits=5, **kw) == ERR_NUM_BITS
        for g in (0, 16, 48, 512):
            assert tgrad(g=g, **kw) == ERR_GROUP_SIZE, g
        assert tgrad(tid=10 ** 6, **kw) == ERR_TEMPLATE_ID
        assert tgrad(bits=3, tid=first_template(3, 64), N=512, **kw) == ERR_TEMPLATE_ID   # 3 bits: TileP 32 only
        assert tgrad(dtype=2, bits=5, **kw) == ERR_DTYPE                          # the order: dtype first
        assert tgrad(N=1000, **kw) == ERR_SHAPE
        assert tgrad(N=64, **kw) == ERR_SHAPE                                      # N % 128
        assert tgrad(tid=first_template(4, 64), N=128, **kw) == ERR_SHAPE                # TileP 64: the column block is 256
        assert tgrad(K=480, **kw) == ERR_SHAPE                                     # K % 64
        assert tgrad(K=384, g=256, **kw) == ERR_SHAPE                              # K % g
        assert tgrad(K=96, g=32, **kw) == ERR_SHAPE                                # K % max(64, g)
        assert tgrad(P=255, **kw) == ERR_SHAPE
        assert tgrad(E=-1, **kw) == ERR_SHAPE
        assert tgrad(R=-1, **kw) == ERR_SHAPE
        assert tgrad(E=65536, **kw) == ERR_SHAPE                                   # the expert is a grid dimension
        assert tgrad(E=65536, nbytes=0, **kw) == ERR_SHAPE                         # ... before the scratch is weighed


def test_nothing_to_do_nulls_and_workspace_in_order():
    #        dY    X     off   Q     S     QM2   rw    dT2   dS    scratch
    full = [FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, None, FAKE]
    assert tgrad(E=0) == OK                       # dT2 has no element: no pointer is looked at
    assert tgrad(E=0, R=0) == OK
    assert tgrad(E=0, nbytes=0) == OK
    assert tgrad() == ERR_NULL
    need = query()
    for i in (7, 9):                              # a null dT2 or scratch: before the scratch is weighed, and at R == 0 too
        ptrs = list(full)
        ptrs[i] = None
        assert tgrad(ptrs=ptrs) == ERR_NULL, i
        assert tgrad(ptrs=ptrs, nbytes=0) == ERR_NULL, i
        assert tgrad(ptrs=ptrs, R=0) == ERR_NULL, i
    with_ds = list(full)
    with_ds[8] = FAKE                             # a dS needs QM2 - and only a dS does
    assert tgrad(ptrs=with_ds) == ERR_NULL
    assert tgrad(ptrs=with_ds, nbytes=0) == ERR_NULL
    assert tgrad(ptrs=with_ds, R=0) == ERR_NULL
    # one byte too few, with every pointer given: the workspace comes before R == 0's zeros and the operands' nulls
    assert tgrad(ptrs=full, nbytes=need - 1) == ERR_WORKSPACE
    assert tgrad(ptrs=full, nbytes=need - 1, R=0) == ERR_WORKSPACE
    assert tgrad(ptrs=[None] * 7 + [FAKE, None, FAKE], nbytes=need - 1) == ERR_WORKSPACE
    for i in (0, 1, 2, 3, 4):                     # then the operands
        for base in (full, with_ds[:5] + [FAKE] + with_ds[6:]):
            ptrs = list(base)
            ptrs[i] = None
            assert tgrad(ptrs=ptrs) == ERR_NULL, i
            ptrs[6] = FAKE                        # with a row weight just the same
            assert tgrad(ptrs=ptrs) == ERR_NULL, i


def test_scratch_query():
    for bits in (2, 3, 4):
        for E, N, K in ((1, 128, 64), (4, 1024, 512), (7, 256, 320), (3, 384, 7168 + 64), (65535, 128, 64)):
            want = E * (N // 128) * -(-K // 256) * 2 * 4 ** bits * 4
            assert query(bits=bits, E=E, N=N, K=K) == want, (bits, E, N, K)
    assert query(bits=4, g=128, E=256, N=2048, K=7168) == 256 * 16 * 28 * 2048 == 234881024   # the header's 235 MB
    assert query(g=32) == query(g=256, K=512) == query()            # the group size does not enter
    for kw in (dict(bits=1), dict(bits=5), dict(g=0), dict(g=48), dict(g=512), dict(E=0), dict(E=-1), dict(E=65536),
               dict(N=0), dict(N=64), dict(N=1000), dict(K=0), dict(K=480), dict(K=384, g=256), dict(K=96, g=32)):
        assert query(**kw) == 0, kw


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def stack(E=4, K=512, N=1024, bits=4, g=64):
    """(weight, scales, table2)"""
    return (meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, N, K // g),
            meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))


def validate(dy, x, off, w, rw=None, bits=4, g=64, with_ds=False, t2=True):
    flute_amd.ops._validate_grouped_table_grad(dy, x, off, w[0], w[1], w[2] if t2 else None, bits, g, with_ds, rw)


def test_validate_grouped_table_grad():
    dy, x, off, w = meta(8, 1024), meta(8, 512), meta(5, dtype=torch.int32), stack()
    rw = meta(8, dtype=torch.float32)
    validate(dy, x, off, w)
    validate(dy, x, off, w, t2=False)
    validate(dy, x, off, w, rw=rw, with_ds=True)
    bf = lambda t: t.bfloat16()
    validate(bf(dy), bf(x), off, (w[0], bf(w[1]), w[2]))
    V, T = ValueError, TypeError
    bad = [
        (V, dict(dy=meta(8, 1024, 1))),                               # ranks
        (V, dict(x=meta(512))),
        (V, dict(off=meta(5, 1, dtype=torch.int32))),
        (V, dict(w=(meta(4 * 256, 512, dtype=torch.int16), w[1], w[2]))),
        (V, dict(w=(w[0], meta(4 * 1024, 8), w[2]))),
        (V, dict(w=(w[0], w[1], meta(4, 16, 16, dtype=torch.float32)))),
        (T, dict(x=x.float(), dy=dy.float())),                        # dtypes
        (T, dict(dy=dy.bfloat16())),                                  # ... grad_output not the input's
        (T, dict(w=(w[0], w[1].bfloat16(), w[2]))),                   # ... scales not the input's
        (T, dict(w=(w[0].to(torch.int32), w[1], w[2]))),
        (T, dict(w=(w[0], w[1], w[2].half()))),
        (T, dict(off=off.long())),                                    # offsets: int32
        (V, dict(bits=5)),
        (V, dict(g=48)),
        (V, dict(dy=meta(7, 1024))),                                  # rows of grad_output and input differ
        (V, dict(x=meta(8, 256))),                                    # input.shape[1] != K
        (V, dict(x=meta(8, 480), w=stack(K=480))),                    # K % 64
        (V, dict(x=meta(8, 384), w=stack(K=384, g=128), g=256)),      # K % g
        (V, dict(dy=meta(8, 1088), w=stack(N=1088))),                 # N % 128
        (V, dict(dy=meta(8, 512))),                                   # P != bits * N / 16
        (V, dict(w=(w[0], meta(3, 1024, 8), w[2]))),                  # scales of another E
        (V, dict(w=(w[0], meta(4, 1024, 4), w[2]))),                  # ... of another group count
        (V, dict(w=(w[0], meta(4, 512, 8), w[2]))),                   # ... of another N
        (V, dict(w=(w[0], w[1], meta(3, 16, 16, 1, dtype=torch.float32)))),  # table2 of another E
        (V, dict(w=(w[0], w[1], meta(4, 4, 4, 1, dtype=torch.float32)))),    # ... of another bit width
        (V, dict(off=meta(4, dtype=torch.int32))),                    # offsets of E + 1 entries
        (V, dict(off=meta(6, dtype=torch.int32))),
        (V, dict(with_ds=True, t2=False)),                            # the scale gradient reads the tables
        (T, dict(rw=rw.half())),
        (V, dict(rw=meta(7, dtype=torch.float32))),
        (V, dict(rw=meta(8, 1, dtype=torch.float32))),
    ]
    for exc, kw in bad:
        args = dict(dy=dy, x=x, off=off, w=w)
        args.update(kw)
        with pytest.raises(exc):
            validate(**args)
    with pytest.raises(V, match="with_scale_grad needs table2"):
        validate(dy, x, off, w, with_ds=True, t2=False)
    # the public function validates before any device call, then refuses tensors that are not on a GPU
    f = flute_amd.qgemm_grouped_table_grad
    with pytest.raises(V):
        f(meta(8, 512), x, off, w[0], w[1], 4, 64, 0)
    with pytest.raises(T):
        f(dy, x, off, w[0], w[1], 4, 64, 0, row_weight=rw.half())
    with pytest.raises(V):
        f(dy, x, off, w[0], w[1], 4, 64, 0, with_scale_grad=True)
    with pytest.raises(RuntimeError, match="GPU"):
        f(dy, x, off, w[0], w[1], 4, 64, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        f(dy, x, off, w[0], w[1], 4, 64, 0, table2=w[2], with_scale_grad=True, row_weight=rw)


def test_fold_per_expert():
    g = torch.Generator().manual_seed(5)
    dT2 = torch.randn(3, 8, 8, 2, generator=g)
    got = flute_amd.grouped_pair_grad_to_table_grad(dT2)
    assert got.shape == (3, 8)
    for e in range(3):
        want = dT2[e, :, :, 0].double().sum(1) + dT2[e, :, :, 1].double().sum(0)
        assert torch.allclose(got[e].double(), want, rtol=0, atol=1e-5)
    for bad in (dT2[0], dT2[:, :, :, :1], dT2[:, :4]):
        with pytest.raises(ValueError):
            flute_amd.grouped_pair_grad_to_table_grad(bad)
    with pytest.raises(ValueError):                # pair_grad_to_table_grad keeps its contract: one expert's [n, n, 2] only
        flute_amd.pair_grad_to_table_grad(dT2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_batched_table2_builder(bits, dtype):
    """The table2 of a stack's codebook against the per-expert make_qmap2_from_qmap, bit for bit, and the pair form
    against the rounded pairs viewed as words; the values need rounding, and include a negative zero and an overflow."""
    build = flute_amd.ops._grouped_codebook_table2
    n, E = 2 ** bits, 5
    g = torch.Generator().manual_seed(bits)
    cb = torch.randn(E, n, generator=g) * 3 + 1e-3
    cb[0, 0], cb[1, 1], cb[2, 0] = -0.0, 1e6, 1e-7
    got = build(cb, bits, dtype)
    want = torch.stack([flute_amd.utils.make_qmap2_from_qmap(cb[e].to(dtype)) for e in range(E)])
    assert got.shape == (E, n, n, 1) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    pair = torch.randn(E, n, n, 2, generator=g)
    got = build(pair, bits, dtype)
    assert got.shape == (E, n, n, 1) and got.dtype == torch.float32
    assert torch.equal(got.view(dtype).view(E, n, n, 2), pair.to(dtype))
    assert not got.requires_grad and not build(cb.clone().requires_grad_(), bits, dtype).requires_grad
    with pytest.raises(TypeError):
        build(cb.to(dtype), bits, dtype)           # the master is fp32
    for bad in (cb[0], cb[:, :n - 1], pair[0], pair[..., :1], torch.zeros(E, n, 2 * n, 2)):
        with pytest.raises(ValueError):
            build(bad, bits, dtype)


def cpu(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def test_refusals_around_autograd():
    """The op refuses to be differentiated itself; the public grouped ops and the ..._learnable_scales entry points keep
    refusing tables that require grad; the codebook entry points validate as their ops do and refuse CPU tensors - all
    before any device call."""
    from flute_amd.integrations import learnable as ln
    E, K, N, bits, g = 2, 64, 128, 4, 64
    w = (cpu(E, bits * N // 16, K, dtype=torch.int16), cpu(E, N, K // g), cpu(E, 16, 16, 1, dtype=torch.float32))
    x, dy, off, rw = cpu(4, K), cpu(4, N), cpu(E + 1, dtype=torch.int32), cpu(4, dtype=torch.float32)
    grad = lambda t: t.clone().requires_grad_()
    for kw in (dict(dy=grad(dy)), dict(x=grad(x)), dict(rw=grad(rw)), dict(s=grad(w[1])), dict(t2=grad(w[2]))):
        a = dict(dy=dy, x=x, rw=None, s=w[1], t2=w[2])
        a.update(kw)
        with pytest.raises(RuntimeError, match="once-differentiable"):
            flute_amd.qgemm_grouped_table_grad(a["dy"], a["x"], off, w[0], a["s"], bits, g, 0, table2=a["t2"],
                                               row_weight=a["rw"])
    with torch.no_grad():                                  # grad mode off: nothing to record, CPU tensors refused as always
        with pytest.raises(RuntimeError, match="GPU"):
            flute_amd.qgemm_grouped_table_grad(grad(dy), x, off, w[0], w[1], bits, g, 0)
    # existing behaviour stays
    msg = "gradients with respect to scales, table or table2 are not supported"
    tab = (w[0], w[1], grad(w[2]))
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped: " + msg):
        flute_amd.qgemm_grouped(x, off, *tab, bits, g, 0)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_weighted: " + msg):
        flute_amd.qgemm_grouped_weighted(x, off, *tab, rw, bits, g, 0)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_glu: " + msg):
        flute_amd.qgemm_grouped_glu(x, off, *w, *tab, bits, g, 0)
    with pytest.raises(RuntimeError, match="qgemm_grouped_learnable_scales: no gradient for table2"):
        ln.qgemm_grouped_learnable_scales(x, off, *tab, bits, g, 0)
    with pytest.raises(RuntimeError, match="qgemm_grouped_weighted_learnable_scales: no gradient for table2"):
        ln.qgemm_grouped_weighted_learnable_scales(x, off, *tab, rw, bits, g, 0)
    with pytest.raises(RuntimeError, match="qgemm_grouped_glu_learnable_scales: no gradient for table2"):
        ln.qgemm_grouped_glu_learnable_scales(x, off, *w, *tab, bits, g, 0)
    # the codebook entry points: the codebook is an fp32 master of the stack's E, in either form
    scalar, pair = torch.zeros(E, 16).requires_grad_(), torch.zeros(E, 16, 16, 2).requires_grad_()
    ws = w[:2]
    for cb in (scalar, pair):
        with pytest.raises(TypeError, match="fp32 master"):
            ln.qgemm_grouped_learnable(x, off, *ws, cb.detach().half(), bits, g, 0)
        with pytest.raises(TypeError, match="fp32 master"):
            ln.qgemm_grouped_glu_learnable(x, off, *ws, cb, *ws, cb.detach().half(), bits, g, 0)
        with pytest.raises(ValueError):
            ln.qgemm_grouped_learnable(x, off, *ws, cb.detach()[:1], bits, g, 0)          # another E
        with pytest.raises(ValueError):
            ln.qgemm_grouped_weighted_learnable(x, off, *ws, cb.detach()[0], rw, bits, g, 0)   # no expert axis
        with pytest.raises(ValueError):
            ln.qgemm_grouped_learnable(x, off, *ws, cb, 2, g, 0)                          # another bit width
        with pytest.raises(ValueError):
            ln.qgemm_grouped_learnable(cpu(4, 128), off, *ws, cb, bits, g, 0)
        with pytest.raises(TypeError):
            ln.qgemm_grouped_weighted_learnable(x, off, *ws, cb, rw.half(), bits, g, 0)
        with pytest.raises(TypeError):
            ln.qgemm_grouped_glu_learnable(x, off, *ws, cb, *ws, cb, bits, g, 0, rows=torch.zeros(4, dtype=torch.int64))
        # their launches refuse CPU tensors, with and without a graph to record: no fall-back
        for c in (cb, cb.detach()):
            with pytest.raises(RuntimeError, match="GPU"):
                ln.qgemm_grouped_learnable(x, off, *ws, c, bits, g, 0)
            with pytest.raises(RuntimeError, match="GPU"):
                ln.qgemm_grouped_weighted_learnable(x, off, *ws, c, rw, bits, g, 0)
            with pytest.raises(RuntimeError, match="GPU"):
                ln.qgemm_grouped_glu_learnable(x, off, *ws, c, *ws, c, bits, g, 0)


def build_model(E=3, K=128, F=256, bits=4, g=64):
    from flute_amd.integrations import moe
    from flute_amd.integrations.base import FluteLinear
    cpu_dev = torch.device("cpu")
    mk = lambda kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, 0, device=cpu_dev, dtype=torch.bfloat16)
    gate, up, down = mk(K, F), mk(K, F), mk(F, K)
    gen = torch.Generator().manual_seed(3)
    for i, m in enumerate((gate, up, down)):
        m.scales.fill_(0.5 + i)
        tables = (torch.randn(E, 2 ** bits, generator=gen) + i).bfloat16()       # per expert, per stack
        m.tables.copy_(tables)
        m.tables2.copy_(torch.stack([flute_amd.utils.make_qmap2_from_qmap(t) for t in tables]))
    experts = moe.FluteExperts(gate, up, down, fused=True, native_routing=True)
    dense = FluteLinear(K, K, bits, g, 0, workspace_lazy_init=True, device=cpu_dev, dtype=torch.bfloat16)
    model = torch.nn.ModuleDict(dict(attn=dense, block=moe.FluteSparseMoeBlock(torch.zeros(E, K), experts, top_k=2)))
    return model, experts, (gate, up, down)


NAMES = ("gate", "up", "down")


def test_defaults_reproduce_the_scales_only_result():
    from flute_amd.integrations import moe
    model, experts, old = build_model()
    keys = list(model.state_dict())
    params = moe.make_experts_learnable(model)
    stacks = (experts.gate, experts.up, experts.down)
    assert len(params) == 3 and all(p is m.scales for p, m in zip(params, stacks))
    assert all(m.table_mode is None and not hasattr(m, "codebook") for m in stacks)
    assert sorted(model.state_dict()) == sorted(keys)
    assert [n for n, _ in model.named_parameters()] == ["block.experts.%s.scales" % s for s in NAMES]
    assert all(m.tables is o.tables and m.tables2 is o.tables2 and m.weight is o.weight for m, o in zip(stacks, old))
    assert experts._fused_ops() == (moe.qgemm_grouped_glu_learnable_scales, moe.qgemm_grouped_weighted_learnable_scales)
    moe.freeze_experts(model)
    stacks = (experts.gate, experts.up, experts.down)
    assert all(type(m) is moe.GroupedFluteLinear for m in stacks) and list(model.state_dict()) == keys
    assert all(m.tables is o.tables and m.tables2 is o.tables2 for m, o in zip(stacks, old))
    assert experts._fused_ops() == (flute_amd.qgemm_grouped_glu, flute_amd.qgemm_grouped_weighted)
    # the explicit single-stack form: scales only, and nothing at all
    one = moe.LearnableGroupedFluteLinear(old[0])
    assert [n for n, _ in one.named_parameters()] == ["scales"] and one.table_mode is None
    none = moe.LearnableGroupedFluteLinear(old[0], scales=False)
    assert not list(none.parameters()) and none.scales is old[0].scales


@pytest.mark.parametrize("scales", [True, False])
@pytest.mark.parametrize("table", ["scalar", "pair"])
def test_make_experts_learnable_with_a_codebook_and_freeze(table, scales):
    from flute_amd.integrations import moe
    model, experts, old = build_model()
    E, n = 3, 16
    keys = list(model.state_dict())
    before = [(o.tables.clone(), o.tables2.clone()) for o in old]
    params = moe.make_experts_learnable(model, scales=scales, table=table)
    stacks = (experts.gate, experts.up, experts.down)
    assert all(type(m) is moe.LearnableGroupedFluteLinear and m.table_mode == table for m in stacks)
    # scales then codebook per stack, in module order
    want = [p for m in stacks for p in ((m.scales, m.codebook) if scales else (m.codebook,))]
    assert len(params) == len(want) and all(a is b for a, b in zip(params, want))
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in params)
    names = [("block.experts.%s." % s) + leaf for s in NAMES for leaf in (("scales", "codebook") if scales else ("codebook",))]
    assert [nm for nm, _ in model.named_parameters()] == names
    assert sorted(model.state_dict()) == sorted(keys + ["block.experts.%s.codebook" % s for s in NAMES])
    for m, o in zip(stacks, old):
        assert m.codebook.dtype == torch.float32 and m.codebook.shape == ((E, n) if table == "scalar" else (E, n, n, 2))
        assert m.weight is o.weight and m.tables is o.tables and m.tables2 is o.tables2
        assert (m.scales is not o.scales) if scales else (m.scales is o.scales)
        if table == "scalar":
            assert torch.equal(m.codebook.detach(), o.tables.float())
        else:
            assert torch.equal(m.codebook.detach().bfloat16().contiguous().view(torch.float32), o.tables2)
        assert torch.equal(flute_amd.ops._grouped_codebook_table2(m.codebook, 4, torch.bfloat16), o.tables2)
    assert experts._fused_ops() == (moe.qgemm_grouped_glu_learnable, moe.qgemm_grouped_weighted_learnable)
    assert moe.make_experts_learnable(model, scales=scales, table=table) == params      # already learnable: nothing swapped
    # ... and other arguments on an already learnable module are refused, not ignored: nothing changes
    for other in (dict(scales=scales, table=None), dict(scales=not scales, table=table),
                  dict(scales=scales, table="pair" if table == "scalar" else "scalar")):
        with pytest.raises(ValueError, match="learnable already"):
            moe.make_experts_learnable(model, **other)
    assert all(m is n for m, n in zip(stacks, (experts.gate, experts.up, experts.down)))

    with torch.no_grad():
        for m in stacks:
            m.codebook.add_(0.3337)                       # not a bf16 value: freeze rounds
    learned = [m.codebook.detach().clone() for m in stacks]
    moe.freeze_experts(model)
    stacks = (experts.gate, experts.up, experts.down)
    assert all(type(m) is moe.GroupedFluteLinear for m in stacks)
    assert list(model.state_dict()) == keys and not list(model.parameters())
    for m, o, cb, (t0, t20) in zip(stacks, old, learned, before):
        assert m.weight is o.weight
        assert m.tables2 is not o.tables2 and m.tables2.dtype == torch.float32 and m.tables2.shape == o.tables2.shape
        assert torch.equal(o.tables, t0) and torch.equal(o.tables2, t20)       # the source stack's buffers are not written
        if table == "scalar":
            assert m.tables is not o.tables and torch.equal(m.tables, cb.bfloat16())
            want2 = torch.stack([flute_amd.utils.make_qmap2_from_qmap(t) for t in cb.bfloat16()])
        else:
            assert m.tables is o.tables
            want2 = cb.bfloat16().contiguous().view(torch.float32)
        assert torch.equal(m.tables2.view(torch.int32), want2.view(torch.int32))
        assert not torch.equal(m.tables2.view(torch.int32), t20.view(torch.int32))


def test_module_refusals():
    from flute_amd.integrations import moe
    model, experts, old = build_model()
    with pytest.raises(ValueError, match="table is"):
        moe.make_experts_learnable(model, table="vector")
    assert type(experts.gate) is moe.GroupedFluteLinear           # nothing was swapped by the refused call
    with pytest.raises(ValueError):
        moe.make_experts_learnable(old[0], table="scalar")
    with pytest.raises(TypeError):
        moe.LearnableGroupedFluteLinear(model["attn"], table="scalar")
    # the scalar form refuses a stack whose tables2 is not the pair table of its tables, as the dense layer does
    old[1].tables2[2, 3, 4, 0] += 1.0
    with pytest.raises(ValueError, match="table='scalar'"):
        moe.LearnableGroupedFluteLinear(old[1], table="scalar")
    pair = moe.LearnableGroupedFluteLinear(old[1], table="pair")
    assert torch.equal(flute_amd.ops._grouped_codebook_table2(pair.codebook, 4, torch.bfloat16), old[1].tables2)
    # gate and up of a fused block take one entry point: both with or both without a codebook
    mixed = moe.FluteExperts(moe.LearnableGroupedFluteLinear(old[0], table="scalar"), old[1], old[2], fused=True)
    with pytest.raises(ValueError, match="both with or both without"):
        mixed._fused_ops()
