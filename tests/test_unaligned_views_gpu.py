"""The Python and torch entry points realign their operands (include/flute_amd.h: the C ABI wants 16-B aligned pointers).

A contiguous view such as buf[1:1 + n].view(M, K) is contiguous and 2 bytes off; the kernels load 16 bytes at a time and
address through buffer descriptors.  Every call here hands such a view - at element offsets 1 and 4 of a larger buffer -
to an entry point and must return the bits of the same call on aligned clones.  The C ABI itself is never given a
misaligned pointer: the entry points copy first (ops._abi_tensor, torch_binding.cpp abi_tensor)."""
import pytest
import torch

from tests import exact_cases as E

pytestmark = pytest.mark.gpu

OFFSETS = (1, 4)
BITS, K, N, G = 4, 512, 256, 64
COUNTS = (5, 0, 12)


def off_view(t, off):
    """t's values in a contiguous view that starts `off` elements into a larger buffer."""
    flat = torch.zeros(off + t.numel() + 8, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == flat.data_ptr() + off * t.element_size()
    return v


def bits_of(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def case(request):
    import flute_amd
    from flute_amd import utils
    T = request.param
    d = torch.device("cuda:0")
    c = dict(fa=flute_amd, T=T, d=d, num_sms=utils.get_device_num_sms(d), ws=utils.get_workspace_streamk(d))
    c["tid"] = min(t for (b, t), cfg in flute_amd.TEMPLATE_CONFIGS.items() if b == BITS and cfg["TileP"] == 32)
    lays = [E.Layer(BITS, K, N, G, T, 90 + e) for e in range(len(COUNTS))]
    c["Q"] = torch.stack([utils.pack(l.W.to(d), BITS, [c["tid"]], c["num_sms"]) for l in lays])
    c["S"] = torch.stack([l.S for l in lays]).to(d)
    c["table"] = lays[0].table.to(d)
    c["t2"] = torch.stack([l.table2 for l in lays]).to(d)
    R = sum(COUNTS)
    gen = torch.Generator().manual_seed(7)
    c["X"] = torch.randint(-4, 5, (R, K), generator=gen).to(T).to(d)
    c["dY"] = torch.randint(-4, 5, (R, N), generator=gen).to(T).to(d)
    off = [0]
    for n in COUNTS:
        off.append(off[-1] + n)
    c["off"] = torch.tensor(off, dtype=torch.int32, device=d)
    return c


def check(call, operands, which):
    """call(**operands) with each operand named in `which` replaced, one at a time and then all together, by a view at each
    offset: the bits of the call on the aligned operands."""
    assert all(t.data_ptr() % 16 == 0 for t in operands.values())
    want = call(**operands)
    want = want if isinstance(want, tuple) else (want,)
    for off in OFFSETS:
        for names in [(n,) for n in which] + [tuple(which)]:
            got = call(**dict(operands, **{n: off_view(operands[n], off) for n in names}))
            got = got if isinstance(got, tuple) else (got,)
            for a, b in zip(want, got):
                assert torch.equal(bits_of(a), bits_of(b)), (names, off)


@pytest.mark.parametrize("M", [2, 17])
def test_qgemm(case, M):
    c = case
    call = lambda input, weight, scales, table, table2: c["fa"].qgemm(input, weight, scales, table, table2, c["ws"], BITS, G, c["tid"], c["num_sms"])
    check(call, dict(input=c["X"][:M].clone(), weight=c["Q"][0].clone(), scales=c["S"][0].clone(), table=c["table"], table2=c["t2"][0].clone()),
          ("input", "scales", "table", "table2", "weight"))


def test_qgemm_hadamard_dequantize_and_backward(case):
    c = case
    fa = c["fa"]
    ops = dict(input=c["X"][:3].clone(), weight=c["Q"][0].clone(), scales=c["S"][0].clone(), table2=c["t2"][0].clone())
    check(lambda input, weight, scales, table2: fa.qgemm_hadamard(input, weight, scales, c["table"], table2, c["ws"], BITS, G, 64, c["tid"], c["num_sms"]),
          ops, ("input", "weight", "scales", "table2"))
    check(lambda input, weight, scales, table2: fa.dequantize(weight, scales, table2, BITS, G, c["tid"]), ops, ("weight", "scales", "table2"))
    check(lambda input, weight, scales, table2: fa.utils.unpack_codes(weight, BITS, c["tid"]).to(torch.int16), ops, ("weight",))

    def backward(input, weight, scales, table2):
        x = input.clone().requires_grad_(True)
        fa.qgemm(x, weight, scales, c["table"], table2, c["ws"], BITS, G, c["tid"], c["num_sms"]).backward(c["dY"][:3])
        return x.grad
    check(backward, ops, ("weight", "scales", "table2"))


def test_grouped(case):
    c = case
    fa, lay = c["fa"], (BITS, G, c["tid"])
    check(lambda input: fa.qgemm_grouped(input, c["off"], c["Q"], c["S"], c["t2"], *lay), dict(input=c["X"]), ("input",))
    check(lambda grad_output: fa.qgemm_grouped_input_grad(grad_output, c["off"], c["Q"], c["S"], c["t2"], *lay), dict(grad_output=c["dY"]),
          ("grad_output",))
    both = dict(grad_output=c["dY"], input=c["X"])
    check(lambda grad_output, input: fa.qgemm_grouped_scale_grad(grad_output, input, c["off"], c["Q"], c["t2"], *lay), both, ("input", "grad_output"))
    check(lambda grad_output, input: fa.qgemm_scale_grad(grad_output, input, c["Q"][0], c["t2"][0], *lay), both, ("input", "grad_output"))


def test_moe_gate_and_combine(case):
    c = case
    fa, d = c["fa"], c["d"]
    gen = torch.Generator().manual_seed(11)
    for dt in (c["T"], torch.float32):
        logits = torch.randn(9, 40, generator=gen).to(dt).to(d)
        check(lambda logits: fa.moe_gate(logits, 4, renormalize=True), dict(logits=logits), ("logits",))
    T, k, NE = 6, 3, 8
    ids = torch.stack([torch.randperm(NE, generator=gen)[:k] for _ in range(T)]).to(d)
    offsets, rows, row_weight, pos, perm = fa.moe_route(ids, None, NE)
    y = torch.randn(T * k, 64, generator=gen).to(c["T"]).to(d)
    check(lambda y: fa.moe_combine(y, pos, offsets), dict(y=y), ("y",))
