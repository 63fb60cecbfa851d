"""The Python and torch entry points realign their operands (include/flute_amd.h: the C ABI wants 16-B aligned pointers).

A contiguous view such as buf[1:1 + n].view(M, K) is contiguous and 2 bytes off; the kernels load 16 bytes at a time and
address through buffer descriptors.  Every call here hands such a view - at two element offsets of a larger buffer, chosen
per element size so that the pointer is off a 16-B boundary - to an entry point and must return the bits of the same call on
aligned clones.  The C ABI itself is never given a
misaligned pointer: the entry points copy first (ops._abi_tensor, torch_binding.cpp abi_tensor)."""
import pytest
import torch

from tests import exact_cases as E

pytestmark = pytest.mark.gpu

OFFSETS = {2: (1, 4), 4: (1, 3), 8: (1, 3)}      # by element size, in elements: none is a multiple of 16 bytes
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
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


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
    for off in range(2):
        for names in [(n,) for n in which] + [tuple(which)]:
            views = {n: off_view(operands[n], OFFSETS[operands[n].element_size()][off]) for n in names}
            assert all(v.data_ptr() % 16 != 0 for v in views.values())
            got = call(**dict(operands, **views))
            got = got if isinstance(got, tuple) else (got,)
            assert len(got) == len(want)
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


# ---- the ops behind ops._abi_call and the grouped launches not covered above: every tensor operand of each

RT, RK, RE, RF = 17, 2, 4, 8                 # the routing ops: 17 tokens, top-2 of 4 experts; the row streams: 8 columns


@pytest.fixture(scope="module")
def routed(case):
    """One routing of RT tokens, shared and left unchanged: ids, weights and what `moe_route` made of them."""
    c, gen = case, torch.Generator().manual_seed(13)
    ids = torch.stack([torch.randperm(RE, generator=gen)[:RK] for _ in range(RT)]).to(torch.int32).to(c["d"])
    weights = torch.rand(RT, RK, generator=gen).to(c["d"])
    offsets, rows, row_weight, pos, perm = c["fa"].moe_route(ids, weights, RE)
    rnd = lambda *shape: torch.randint(-4, 5, shape, generator=gen).to(c["T"]).to(c["d"])
    return dict(ids=ids, weights=weights, offsets=offsets, rows=rows, row_weight=row_weight, pos=pos, rnd=rnd, gen=gen)


def test_hadamard_transform(case):
    check(lambda input: case["fa"].hadamard_transform(input, 64), dict(input=case["X"]), ("input",))


def test_table_grads(case):
    c = case
    fa, lay = c["fa"], (BITS, G, c["tid"])
    row_weight = torch.rand(sum(COUNTS), generator=torch.Generator().manual_seed(5)).to(c["d"])
    dense = dict(grad_output=c["dY"], input=c["X"], weight=c["Q"][0].clone(), scales=c["S"][0].clone(), table2=c["t2"][0].clone())
    check(lambda grad_output, input, weight, scales, table2: fa.qgemm_table_grad(
        grad_output, input, weight, scales, *lay, table2=table2, with_scale_grad=True), dense, tuple(dense))
    stack = dict(grad_output=c["dY"], input=c["X"], offsets=c["off"], weight=c["Q"], scales=c["S"], table2=c["t2"], row_weight=row_weight)
    check(lambda grad_output, input, offsets, weight, scales, table2, row_weight: fa.qgemm_grouped_table_grad(
        grad_output, input, offsets, weight, scales, *lay, table2=table2, with_scale_grad=True, row_weight=row_weight),
        stack, tuple(stack))


def test_grouped_glu_and_weighted(case):
    c = case
    fa, lay = c["fa"], (BITS, G, c["tid"])
    gen = torch.Generator().manual_seed(3)
    R = sum(COUNTS)
    glu = dict(input=c["X"], rows=torch.randint(0, R, (R,), generator=gen).to(torch.int32).to(c["d"]), offsets=c["off"],
               gate_weight=c["Q"], gate_scales=c["S"], gate_table2=c["t2"], up_weight=c["Q"].flip(0).contiguous(),
               up_scales=c["S"].flip(0).contiguous(), up_table2=c["t2"].flip(0).contiguous())
    check(lambda input, rows, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2: fa.qgemm_grouped_glu(
        input, offsets, gate_weight, gate_scales, gate_table2, up_weight, up_scales, up_table2, *lay, rows=rows), glu, tuple(glu))
    weighted = dict(input=c["X"], offsets=c["off"], weight=c["Q"], scales=c["S"], table2=c["t2"],
                    row_weight=torch.rand(R, generator=gen).to(c["d"]))
    check(lambda input, offsets, weight, scales, table2, row_weight: fa.qgemm_grouped_weighted(
        input, offsets, weight, scales, table2, row_weight, *lay), weighted, tuple(weighted))


@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_moe_route_and_wide(case, routed, id_dtype):
    fa = case["fa"]
    for weights in (routed["weights"], routed["weights"].to(case["T"])):
        operands = dict(topk_ids=routed["ids"].to(id_dtype), topk_weights=weights)
        check(lambda topk_ids, topk_weights: fa.moe_route(topk_ids, topk_weights, RE), operands, tuple(operands))
        check(lambda topk_ids, topk_weights: fa.moe_route_wide(topk_ids, topk_weights, RE, chunk_tokens=4), operands, tuple(operands))


def test_moe_gate_route_forms(case, routed):
    fa = case["fa"]
    bias = torch.rand(RE, generator=routed["gen"]).to(case["d"])
    for dt in (case["T"], torch.float32):
        operands = dict(logits=torch.randn(RT, RE, generator=routed["gen"]).to(dt).to(case["d"]), bias=bias)
        check(lambda logits, bias: fa.moe_gate_route(logits, RK, RE, "sigmoid", True, bias), operands, tuple(operands))
        check(lambda logits, bias: fa.moe_gate_route_limited(logits, RK, 2, 1, RE, "sigmoid", True, bias), operands, tuple(operands))
        check(lambda logits, bias: fa.moe_gate_route_wide(logits, RK, RE, "sigmoid", True, bias, 1.0, 2, 1, "max", chunk_tokens=4),
              operands, tuple(operands))


def test_moe_combine_and_row_streams(case, routed):
    fa, r = case["fa"], routed
    R = RT * RK
    stream = dict(offsets=r["offsets"], pos=r["pos"], rows=r["rows"], row_weight=r["row_weight"])
    pick = lambda *names, **more: dict({n: stream[n] for n in names}, **more)
    ops = pick("pos", "offsets", y=r["rnd"](R, RF))
    check(lambda y, pos, offsets: fa.moe_combine(y, pos, offsets), ops, tuple(ops))
    ops = pick("offsets", g=r["rnd"](R, RF), u=r["rnd"](R, RF), grad_output=r["rnd"](R, RF))
    check(lambda g, u, grad_output, offsets: fa.swiglu_grad(g, u, grad_output, offsets), ops, tuple(ops))
    ops = pick("rows", "offsets", input=r["rnd"](RT, RF))
    check(lambda input, rows, offsets: fa.moe_gather(input, rows, offsets), ops, tuple(ops))
    ops = pick("row_weight", "offsets", grad_unweighted=r["rnd"](R, RF), input=r["rnd"](R, RF))
    check(lambda grad_unweighted, input, row_weight, offsets: fa.moe_weight_grad(grad_unweighted, input, row_weight, offsets),
          ops, tuple(ops))
    for dt in (case["T"], torch.float32):
        ops = pick("pos", logits=torch.randn(RT, RE, generator=r["gen"]).to(dt).to(case["d"]), ids=r["ids"],
                   grad_weights=torch.randn(RT, RK, generator=r["gen"]).to(case["d"]),
                   grad_row_weight=torch.randn(R, generator=r["gen"]).to(case["d"]))
        check(lambda logits, ids, grad_weights, grad_row_weight, pos: fa.moe_gate_grad(
            logits, ids, grad_weights, "softmax", True, 1.0, grad_row_weight=grad_row_weight, pos=pos), ops, tuple(ops))
