"""flute_qgemm_grouped_scale_grad, its Python wrapper, the learnable grouped entry points and the expert modules without
a GPU: the export, every refusal of the C ABI (returned before anything is enqueued, on null or host pointers), every
branch of the wrapper's validator on meta tensors, the refusals around autograd, and make_experts_learnable /
freeze_experts on modules built on the CPU."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
FAKE = 0x1000            # a host address no refusal may look behind


def sgrad(dtype=0, bits=4, g=64, E=4, R=8, N=1024, K=512, P=None, tid=0, ptrs=(None,) * 7, num_sms=256):
    """ptrs: dY, X, offsets, Q, QM2, row_weight, dS"""
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped_scale_grad(dtype, bits, g, E, R, N, K, P, tid, *ptrs, num_sms, None)


def test_symbol_declared_abi_unchanged():
    with open(HEADER) as f:
        text = f.read()
    assert "flute_qgemm_grouped_scale_grad" in _lib.SYMBOLS
    assert "int flute_qgemm_grouped_scale_grad(" in text
    getattr(_lib.get(), "flute_qgemm_grouped_scale_grad")
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_grouped_scale_grad is flute_amd.ops.qgemm_grouped_scale_grad


def test_layer_and_shape_refusals_with_null_and_host_pointers():
    for ptrs in ((None,) * 7, (FAKE,) * 7):                       # refused before any pointer is looked at or behind
        kw = dict(ptrs=ptrs)
        assert sgrad(dtype=2, **kw) == ERR_DTYPE
        assert sgrad(bits=5, **kw) == ERR_NUM_BITS
        for g in (0, 16, 48, 512):
            assert sgrad(g=g, **kw) == ERR_GROUP_SIZE, g
        assert sgrad(tid=10 ** 6, **kw) == ERR_TEMPLATE_ID
        assert sgrad(bits=3, tid=first_template(3, 64), N=512, **kw) == ERR_TEMPLATE_ID   # 3 bits: TileP 32 only
        assert sgrad(dtype=2, bits=5, **kw) == ERR_DTYPE                          # the order: dtype first
        assert sgrad(N=1000, **kw) == ERR_SHAPE
        assert sgrad(N=64, **kw) == ERR_SHAPE                                      # N % 128
        assert sgrad(tid=first_template(4, 64), N=128, **kw) == ERR_SHAPE                # TileP 64: the column block is 256
        assert sgrad(K=480, **kw) == ERR_SHAPE                                     # K % 64
        assert sgrad(K=384, g=256, **kw) == ERR_SHAPE                              # K % g
        assert sgrad(K=96, g=32, **kw) == ERR_SHAPE                                # K % max(64, g)
        assert sgrad(P=255, **kw) == ERR_SHAPE
        assert sgrad(E=-1, **kw) == ERR_SHAPE
        assert sgrad(R=-1, **kw) == ERR_SHAPE
        assert sgrad(E=65536, **kw) == ERR_SHAPE                                   # the expert is the grid's z


def test_nothing_to_do_and_nulls():
    full = [FAKE] * 5 + [None, FAKE]
    assert sgrad(E=0) == OK                       # dS has no element: no pointer is looked at
    assert sgrad(E=0, R=0) == OK
    assert sgrad() == ERR_NULL
    assert sgrad(R=0) == ERR_NULL                 # R == 0 still writes dS (zeros): a null dS is refused
    for i in (0, 1, 2, 3, 4, 6):
        ptrs = list(full)
        ptrs[i] = None
        assert sgrad(ptrs=ptrs) == ERR_NULL, i
        ptrs[5] = FAKE                            # with a row weight just the same
        assert sgrad(ptrs=ptrs) == ERR_NULL, i


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def stack(E=4, K=512, N=1024, bits=4):
    return meta(E, bits * N // 16, K, dtype=torch.int16), meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32)


def validate(dy, x, off, w, rw=None, bits=4, g=64):
    flute_amd.ops._validate_grouped_scale_grad(dy, x, off, *w, bits, g, rw)


def test_validate_grouped_scale_grad():
    dy, x, off, w = meta(8, 1024), meta(8, 512), meta(5, dtype=torch.int32), stack()
    rw = meta(8, dtype=torch.float32)
    validate(dy, x, off, w)
    validate(dy, x, off, w, rw=rw)
    validate(dy.bfloat16(), x.bfloat16(), off, w)
    V, T = ValueError, TypeError
    bad = [
        (V, dict(dy=meta(8, 1024, 1))),                               # ranks
        (V, dict(x=meta(512))),
        (V, dict(off=meta(5, 1, dtype=torch.int32))),
        (V, dict(w=(meta(4 * 256, 512, dtype=torch.int16), w[1]))),
        (V, dict(w=(w[0], meta(4, 16, 16, dtype=torch.float32)))),
        (T, dict(x=x.float(), dy=dy.float())),                        # dtypes
        (T, dict(dy=dy.bfloat16())),                                  # ... grad_output not the input's
        (T, dict(w=(w[0].to(torch.int32), w[1]))),
        (T, dict(w=(w[0], w[1].half()))),
        (T, dict(off=off.long())),                                    # offsets: int32
        (V, dict(bits=5)),
        (V, dict(g=48)),
        (V, dict(dy=meta(7, 1024))),                                  # rows of grad_output and input differ
        (V, dict(x=meta(8, 256))),                                    # input.shape[1] != K
        (V, dict(x=meta(8, 480), w=stack(K=480))),                    # K % 64
        (V, dict(x=meta(8, 384), w=stack(K=384), g=256)),             # K % g
        (V, dict(dy=meta(8, 1088), w=stack(N=1088))),                 # N % 128
        (V, dict(dy=meta(8, 512))),                                   # P != bits * N / 16
        (V, dict(w=(w[0], meta(3, 16, 16, 1, dtype=torch.float32)))),  # table2 of another E
        (V, dict(w=(w[0], meta(4, 4, 4, 1, dtype=torch.float32)))),   # ... of another bit width
        (V, dict(off=meta(4, dtype=torch.int32))),                    # offsets of E + 1 entries
        (V, dict(off=meta(6, dtype=torch.int32))),
        (T, dict(rw=rw.half())),
        (V, dict(rw=meta(7, dtype=torch.float32))),
        (V, dict(rw=meta(8, 1, dtype=torch.float32))),
    ]
    for exc, kw in bad:
        args = dict(dy=dy, x=x, off=off, w=w)
        args.update(kw)
        with pytest.raises(exc):
            validate(**args)
    # the public function validates before any device call, then refuses tensors that are not on a GPU
    with pytest.raises(V):
        flute_amd.qgemm_grouped_scale_grad(meta(8, 512), x, off, *w, 4, 64, 0)
    with pytest.raises(T):
        flute_amd.qgemm_grouped_scale_grad(dy, x, off, *w, 4, 64, 0, row_weight=rw.half())
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.qgemm_grouped_scale_grad(dy, x, off, *w, 4, 64, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.qgemm_grouped_scale_grad(dy, x, off, *w, 4, 64, 0, row_weight=rw)


def cpu(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def test_refusals_around_autograd():
    """The op refuses to be differentiated itself; the public grouped ops still raise on scales that require grad; the
    learnable entry points refuse a table that requires grad - all before any device call."""
    from flute_amd.integrations import learnable as ln
    E, K, N, bits, g = 2, 64, 128, 4, 64
    w = (cpu(E, bits * N // 16, K, dtype=torch.int16), cpu(E, N, K // g), cpu(E, 16, 16, 1, dtype=torch.float32))
    x, dy, off, rw = cpu(4, K), cpu(4, N), cpu(E + 1, dtype=torch.int32), cpu(4, dtype=torch.float32)
    for kw in (dict(dy=dy.clone().requires_grad_()), dict(x=x.clone().requires_grad_()), dict(rw=rw.clone().requires_grad_())):
        a = dict(dy=dy, x=x, rw=None)
        a.update(kw)
        with pytest.raises(RuntimeError, match="once-differentiable"):
            flute_amd.qgemm_grouped_scale_grad(a["dy"], a["x"], off, w[0], w[2], bits, g, 0, row_weight=a["rw"])
    with torch.no_grad():                                  # grad mode off: nothing to record, CPU tensors refused as always
        with pytest.raises(RuntimeError, match="GPU"):
            flute_amd.qgemm_grouped_scale_grad(dy.clone().requires_grad_(), x, off, w[0], w[2], bits, g, 0)
    msg = "gradients with respect to scales, table or table2 are not supported"
    learn = (w[0], w[1].clone().requires_grad_(), w[2])
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped: " + msg):
        flute_amd.qgemm_grouped(x, off, *learn, bits, g, 0)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_weighted: " + msg):
        flute_amd.qgemm_grouped_weighted(x, off, *learn, rw, bits, g, 0)
    with pytest.raises(RuntimeError, match="flute_amd.qgemm_grouped_glu: " + msg):
        flute_amd.qgemm_grouped_glu(x, off, *w, *learn, bits, g, 0)
    tab = (w[0], w[1], w[2].clone().requires_grad_())
    with pytest.raises(RuntimeError, match="qgemm_grouped_learnable_scales: no gradient for table2"):
        ln.qgemm_grouped_learnable_scales(x, off, *tab, bits, g, 0)
    with pytest.raises(RuntimeError, match="qgemm_grouped_weighted_learnable_scales: no gradient for table2"):
        ln.qgemm_grouped_weighted_learnable_scales(x, off, *tab, rw, bits, g, 0)
    with pytest.raises(RuntimeError, match="qgemm_grouped_glu_learnable_scales: no gradient for table2"):
        ln.qgemm_grouped_glu_learnable_scales(x, off, *w, *tab, bits, g, 0)
    # the entry points validate as their ops do, and their launches refuse CPU tensors: no fall-back
    with pytest.raises(ValueError):
        ln.qgemm_grouped_learnable_scales(cpu(4, 128), off, *learn, bits, g, 0)
    with pytest.raises(TypeError):
        ln.qgemm_grouped_weighted_learnable_scales(x, off, *learn, rw.half(), bits, g, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ln.qgemm_grouped_learnable_scales(x, off, *learn, bits, g, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ln.qgemm_grouped_weighted_learnable_scales(x, off, *learn, rw, bits, g, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ln.qgemm_grouped_glu_learnable_scales(x, off, *learn, *w, bits, g, 0)


def test_make_experts_learnable_and_freeze_on_cpu_modules():
    from flute_amd.integrations import learnable as ln
    from flute_amd.integrations import moe
    from flute_amd.integrations.base import FluteLinear
    cpu_dev = torch.device("cpu")
    E, K, F, bits, g = 3, 128, 256, 4, 64
    mk = lambda kk, nn: moe.GroupedFluteLinear(E, kk, nn, bits, g, 0, device=cpu_dev, dtype=torch.bfloat16)
    gate, up, down = mk(K, F), mk(K, F), mk(F, K)
    for i, m in enumerate((gate, up, down)):
        m.scales.fill_(0.5 + i)
    experts = moe.FluteExperts(gate, up, down, fused=True, native_routing=True)
    dense = FluteLinear(K, K, bits, g, 0, workspace_lazy_init=True, device=cpu_dev, dtype=torch.bfloat16)
    model = torch.nn.ModuleDict(dict(attn=dense, block=moe.FluteSparseMoeBlock(torch.zeros(E, K), experts, top_k=2)))
    keys = list(model.state_dict())
    # the dense helpers keep ignoring grouped stacks
    assert ln.make_scales_learnable(model) == [model["attn"].scales] and type(experts.gate) is moe.GroupedFluteLinear
    ln.freeze_scales(model)
    assert type(model["attn"]) is FluteLinear

    params = moe.make_experts_learnable(model)
    stacks = (experts.gate, experts.up, experts.down)
    assert all(type(m) is moe.LearnableGroupedFluteLinear for m in stacks) and type(model["attn"]) is FluteLinear
    assert len(params) == 3 and all(p is m.scales for p, m in zip(params, stacks))          # module order: gate, up, down
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in params)
    assert [float(p.detach()[0, 0, 0]) for p in params] == [0.5, 1.5, 2.5]
    for new, old in zip(stacks, (gate, up, down)):
        assert new.weight is old.weight and new.tables is old.tables and new.tables2 is old.tables2
        assert new.scales is not old.scales and new.scales.data_ptr() != old.scales.data_ptr()
        assert torch.equal(new.scales.detach(), old.scales)
        assert (new.num_experts, new.in_features, new.out_features, new.num_bits, new.group_size, new.template_id) == \
            (old.num_experts, old.in_features, old.out_features, old.num_bits, old.group_size, old.template_id)
    assert sorted(model.state_dict()) == sorted(keys)
    assert [n for n, _ in model.named_parameters()] == ["block.experts.%s.scales" % s for s in ("gate", "up", "down")]
    assert moe.make_experts_learnable(model) == params                                      # already learnable: nothing swapped
    with pytest.raises(ValueError):
        moe.make_experts_learnable(gate)
    with pytest.raises(ValueError):
        moe.freeze_experts(experts.gate)
    with pytest.raises(TypeError):
        moe.LearnableGroupedFluteLinear(dense)

    with torch.no_grad():
        params[1].mul_(2)
    learned = [p.detach().clone() for p in params]
    state = {k: v.clone() for k, v in model.state_dict().items() if torch.is_tensor(v)}
    moe.freeze_experts(model)
    stacks = (experts.gate, experts.up, experts.down)
    assert all(type(m) is moe.GroupedFluteLinear for m in stacks)
    assert all(torch.equal(m.scales, s) and not m.scales.requires_grad for m, s in zip(stacks, learned))
    assert all(m.weight is o.weight and m.tables2 is o.tables2 for m, o in zip(stacks, (gate, up, down)))
    assert list(model.state_dict()) == keys and not list(model.parameters())
    fresh = moe.FluteExperts(mk(K, F), mk(K, F), mk(F, K))
    fresh.load_state_dict({k[len("block.experts."):]: v for k, v in state.items() if k.startswith("block.experts.")})
    assert torch.equal(fresh.up.scales, learned[1])
