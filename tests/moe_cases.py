"""What the MoE routing and gating tests share: canary-guarded output buffers, the routing contract as a host loop, the
top-3 module case, and the gating tests' draws and direct ABI call."""
import pytest
import torch

from tests.support import first_template

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
I32 = torch.int32
DTYPE_CODE = {F16: 0, BF16: 1, F32: 2}
SCORING_CODE = {"softmax": 0, "sigmoid": 1}
CANARY = -0x5A5A5A5B
GUARD = 32


# ---- route ---------------------------------------------------------------------------------------------------------------

def host_route(ids, k, E):
    """The contract as a naive loop over the flattened ids (Python ints): offsets, perm, rows, pos."""
    P = len(ids)
    bucket = [v if 0 <= v < E else E for v in ids]
    perm = []
    offsets = []
    for b in range(E + 1):
        offsets.append(len(perm))
        for p in range(P):
            if bucket[p] == b:
                perm.append(p)
    assert len(perm) == P
    pos = [0] * P
    for i, p in enumerate(perm):
        pos[p] = i
    return offsets, perm, [p // k for p in perm], pos


def canary_padded(n, dtype, dev):
    buf = torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.int32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype)


def intact(buf, n):
    return bool(torch.all(buf[:GUARD] == CANARY)) and bool(torch.all(buf[GUARD + n:] == CANARY))


# ---- the module ----------------------------------------------------------------------------------------------------------

def native(env, c, fused):
    return env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused, native_routing=True)


@pytest.fixture(scope="module")
def top3_case(env):
    """E = 4 experts (4-bit, g = 64, K = 256, N_ff = 512), T = 37 tokens, three of the four experts per token."""
    d, dtype = env.dev, F16
    E, K, F, T, k, bits, g = 4, 256, 512, 37, 3, 4, 64
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(33)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, k=k, bits=bits, g=g, tid=tid, dtype=dtype)
    c["gates"], c["ups"], c["downs"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)],
                                        [linear(F, K) for _ in range(E)])
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    c["ids"] = torch.rand(T, E, generator=gen).topk(k, dim=1).indices.to(d)
    weights = torch.rand(T, k, generator=gen)
    c["weights"] = (weights / weights.sum(1, keepdim=True)).to(dtype).to(d)
    return c


# ---- gating: inputs and calls ----------------------------------------------------------------------------------------------

def draw_logits(T, E, dtype, seed, spread=2.0):
    return (torch.randn(T, E, generator=torch.Generator().manual_seed(seed)) * spread).to(dtype)


def draw_bias(E, seed):
    return torch.randn(E, generator=torch.Generator().manual_seed(seed))


def gate_abi(env, logits, k, scoring="softmax", renormalize=False, bias=None, scale=1.0, routed=False):
    """The direct call with every output in the middle of a larger buffer: (ids, weights) or, routed, also (offsets, rows,
    row_weight, pos, perm)."""
    d = env.dev
    T, E = logits.shape
    P = T * k
    sizes = dict(ids=P, weights=P)
    if routed:
        sizes.update(offsets=E + 1, perm=P, rows=P, row_weight=P, pos=P)
    bufs = {n: canary_padded(s, F32 if n in ("weights", "row_weight") else I32, d) for n, s in sizes.items()}
    head = (DTYPE_CODE[logits.dtype], T, E, k, SCORING_CODE[scoring], int(renormalize), float(scale), logits.data_ptr(),
            None if bias is None else bias.data_ptr(), bufs["ids"][1].data_ptr(), bufs["weights"][1].data_ptr())
    lib = env.lib
    with torch.cuda.device(d):
        stream = torch.cuda.current_stream(d).cuda_stream
        if routed:
            rc = lib.flute_moe_gate_route(*head, *(bufs[n][1].data_ptr() for n in ("offsets", "perm", "rows", "row_weight", "pos")),
                                          stream)
        else:
            rc = lib.flute_moe_gate(*head, stream)
    assert rc == 0
    torch.cuda.synchronize()
    for n, s in sizes.items():
        assert intact(bufs[n][0], s), "canary around " + n
    out = {n: bufs[n][1] for n in sizes}
    ids, weights = out["ids"].view(T, k), out["weights"].view(T, k)
    if not routed:
        return ids, weights
    return ids, weights, out["offsets"], out["rows"], out["row_weight"], out["pos"].view(T, k), out["perm"]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))
