"""What the grouped-qgemm tests share (forward, GLU, blocks, the three gradients, the expert modules): the case
matrices and their seeds, exact and random stacks on the device, the per-expert exact check, the shared expert-module
case, the restated expert block and the gradient tests' inputs."""
import pytest
import torch

from tests import exact_cases as XC
from tests import scale_grad_ref as SR
from tests import table_grad_ref as TR
from tests.support import first_template, offsets_of

F16, BF16 = torch.float16, torch.bfloat16

# ---- the forward -----------------------------------------------------------------------------------------------------

COUNTS = [0, 1, 15, 16, 17, 0, 33, 70]           # an empty first expert, one in the middle, both sides of a 16-row tile

# the first K past one scale-panel chunk of the kernel (56 blocks: 7168 k at 4 bits, 3584 at 2 bits, 1792 at 3 bits, all at
# group size 32) plus one 64-k step: the panel is staged a second time, for a ragged last chunk
K_CHUNK_CASES = [(4, 32, 7168 + 64), (4, 64, 7168 + 64), (2, 32, 3584 + 64), (3, 32, 1792 + 64)]


def random_case(e, bits, tile_p, g, dtype, K, N, seed, pair):
    """Random codes, randn scales, an NF-style table or a random pair codebook (HIGGS vector_size = 2)."""
    gen = torch.Generator().manual_seed(seed)
    n = 2 ** bits
    W = torch.randint(0, n, (K, N), generator=gen, dtype=torch.uint8)
    S = torch.randn(N, K // g, generator=gen).to(dtype)
    if pair:
        table2 = torch.randn(n * n, 2, generator=gen).to(dtype).view(n, n, 2).contiguous().view(torch.float32)
    else:
        table2 = e.O.make_qmap2_from_qmap(torch.randn(n, generator=gen).sort().values.to(dtype))
    Q = torch.from_numpy(e.O.pack(W.numpy(), bits, tile_p))
    return Q, S, table2


def exact_layers(bits, tile_p, g, dtype, K, N, pair, E, seed0):
    return [XC.Layer(bits, K, N, g, dtype, seed=seed0 + e, tile_p=tile_p, pair=pair) for e in range(E)]


def stack_exact(env, layers):
    """The grouped operands of E exact layers: Q [E, P, K], S [E, N, G], table2 [E, n, n, 1] on the device."""
    lay = layers[0]
    tid = first_template(lay.bits, lay.tile_p)
    Q = torch.stack([env.utils.pack(l.W.to(env.dev), l.bits, [tid], env.num_sms) for l in layers])
    S = torch.stack([l.S for l in layers]).to(env.dev)
    t2 = torch.stack([l.table2 for l in layers]).to(env.dev)
    return Q, S, t2, tid


def check_exact(env, layers, counts, X, Y):
    off = offsets_of(counts).tolist()
    T = off[-1]
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        rows = X[r0:r1]
        R, A = XC.exact_product(rows, lay, abs_too=True)
        XC.premise(rows, lay, R, A, witness=(r1 == T))           # the accumulator witness is the last row of X
        assert XC.exact_equal(Y[r0:r1], R, lay.dtype), (e, lay)


def exact_matrix():
    rows = ((32, BF16, 64, 1, False), (64, F16, 1088, 3, False), (128, BF16, 2048, 1, True), (256, F16, 4352, 1, False))
    out = []
    for bits in (4, 3, 2):
        for tile_p in ((32, 64) if bits != 3 else (32,)):
            for g, dtype, K, nblk, pair in rows:
                out.append((bits, tile_p, g, dtype, K, nblk * XC.cols_per_block(bits, tile_p), pair))
    return out


def exact_seed(bits, tile_p, g):
    return 1000 * bits + 10 * tile_p + g


def random_stack(env, bits, tile_p, g, dtype, K, N, E, seed):
    """E random layers (random_case: random codes, randn scales, an NF-style table or a pair codebook) and their exact
    lut * s weights [K, N] in fp64."""
    Qs, Ss, t2s, Ws = [], [], [], []
    for e in range(E):
        Q, S, table2 = random_case(env, bits, tile_p, g, dtype, K, N, seed + e, pair=(e % 2 == 1))
        idx = torch.from_numpy(env.O.pair_index(Q.numpy(), bits, tile_p))                  # [K / 2, N]
        w = env.O.table2_as_pairs(table2, dtype).double()[idx].permute(0, 2, 1).reshape(K, N)
        Ws.append(w * torch.repeat_interleave(S.double(), g, dim=1).T)
        Qs.append(Q), Ss.append(S), t2s.append(table2)
    d = env.dev
    return torch.stack(Qs).to(d), torch.stack(Ss).to(d), torch.stack(t2s).to(d), Ws


# ---- the GLU and the weighted down projection ----------------------------------------------------------------------------

EPS_S = 2.0 ** -21                                   # include/flute_amd.h: silu32 and the fp32 product by u
ETA = {F16: 2.0 ** -24, BF16: 2.0 ** -126}
assert EPS_S <= 2.0 ** -14


def assert_glu(H, E, dtype, what):
    u = XC.U_T[dtype]
    H = H.double().cpu()
    err = (H - E).abs()
    bound = (u + EPS_S * (1 + u)) * E.abs() + ETA[dtype]
    worst = float((err / bound).max())
    print("glu %s: max |H - E| / bound = %.4f, max|E| = %.3e" % (what, worst, float(E.abs().max())))
    assert torch.isfinite(H).all() and bool((err <= bound).all()), (what, worst)


ROW_WEIGHTS = torch.tensor([0.25, 0.5, 0.75, 1.0, 1.5])


def draw_row_weights(T, seed):
    return ROW_WEIGHTS[torch.randint(0, len(ROW_WEIGHTS), (T,), generator=torch.Generator().manual_seed(seed))]


def weighted_expected(layers, counts, X, w):
    """round_T(w R) per row, R the exact product; premise: |R| < 2^19, so w R (w a multiple of 2^-2 below 2) is exact in fp32."""
    off = offsets_of(counts).tolist()
    out = torch.zeros(off[-1], layers[0].N, dtype=torch.float64)
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        R, A = XC.exact_product(X[r0:r1], lay, abs_too=True)
        XC.premise(X[r0:r1], lay, R, A, witness=(r1 == off[-1]))
        assert float(R.abs().max()) < 2.0 ** 19
        out[r0:r1] = R * w[r0:r1].double()[:, None]
    return out


# ---- the expert modules ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def experts_case(env):
    """E = 4 experts from FluteLinear.from_codes (4-bit, g = 64, K = 256, N_ff = 512), T = 37 tokens, top-2 routing among
    experts 0, 1, 3: expert 2 is never chosen."""
    d, dtype = env.dev, F16
    E, K, F, T, k, bits, g = 4, 256, 512, 37, 2, 4, 64
    tid = first_template(bits, 32)
    gen = torch.Generator().manual_seed(21)
    nf4 = torch.tensor(env.O.NF4_VALUES).to(dtype)

    def linear(kk, nn):
        codes = torch.randint(0, 16, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, nf4.to(d), bits, g, tid)

    c = dict(E=E, K=K, F=F, T=T, k=k, bits=bits, g=g, tid=tid, dtype=dtype)
    c["gates"], c["ups"], c["downs"] = ([linear(K, F) for _ in range(E)], [linear(K, F) for _ in range(E)],
                                        [linear(F, K) for _ in range(E)])
    c["experts"] = env.moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"])
    c["hidden"] = torch.randn(T, K, generator=gen).to(dtype).to(d)
    choice = torch.tensor([[0, 1], [1, 3], [3, 0], [0, 3], [3, 1], [1, 0]])
    c["ids"] = choice[torch.randint(0, len(choice), (T,), generator=gen)].to(d)
    c["ids2"] = choice[torch.randint(0, len(choice), (T,), generator=gen)].flip(0).to(d)
    weights = torch.rand(T, k, generator=gen)
    c["weights"] = (weights / weights.sum(1, keepdim=True)).to(dtype).to(d)
    return c


def restated_experts(c, hidden, ids, weights, project):
    """The block restated with torch ops: a loop over the experts on rows selected on the host, `project(e, which, x)` the
    projection `which` (0 gate, 1 up, 2 down) of expert e, silu, the routing weight and index_add_."""
    out = torch.zeros_like(hidden)
    for e in range(c["E"]):
        tok, slot = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        x = hidden[tok]
        h = torch.nn.functional.silu(project(e, 0, x)) * project(e, 1, x)
        out = out.index_add(0, tok, project(e, 2, h) * weights[tok, slot][:, None])
    return out


def gate_formula(logits, ids, scoring, renormalize, scale):
    s = torch.softmax(logits, dim=1) if scoring == "softmax" else torch.sigmoid(logits)
    w = s.gather(1, ids.long())
    if renormalize:
        w = w / w.sum(dim=1, keepdim=True)
    return w * scale


def scale_leaves(c):
    """The three stacks' scales [E, N, K / g] as fp64 leaves."""
    return [torch.stack([m.scales for m in ms]).double().requires_grad_() for ms in c["layers"]]


def dense_project(c, S64):
    """project(e, which, x) = x @ (L * S)^T in fp64, S the leaf of the stack `which`."""
    g = c["g"]
    return lambda e, which, x: x @ (c["lut"][which][e] * S64[which][e].repeat_interleave(g, dim=1)).T


# ---- the gradients ---------------------------------------------------------------------------------------------------

def counts_of(RB):
    """An empty first expert, an empty one in the middle, counts on both sides of the kernel's row block."""
    return [0, 1, RB - 1, RB, RB + 1, 0, 2 * RB + 3, 5]


GRAD_COUNTS = [0, 1, 31, 32, 33, 0, 97, 5]     # an empty first expert, one in the middle, one row, both sides of the 32-row step
PAD = 7                                        # rows past offsets[E]: NaN in dY and X, never read
HALF_SUB = {F16: 2.0 ** -25, BF16: 2.0 ** -134}  # half the spacing of the type's subnormals: the rounding error below its smallest normal
MIN_NORMAL = {F16: 2.0 ** -14, BF16: 2.0 ** -126}
ROWS = ((32, BF16, False), (64, F16, False), (128, BF16, True), (256, F16, False))      # (g, dtype, pair codebook)


def matrix():
    """bits 4 / 3 / 2 x TileP 32 / 64 (3 bits: 32) x ROWS.  N = 256 - two of the kernel's 128-column blocks - or the
    template's own column block where that is larger (512: no smaller N is a legal layer); K = 256 + max(64, g): a
    second, partial k block."""
    out = []
    for bits in (4, 3, 2):
        for tile_p in ((32, 64) if bits != 3 else (32,)):
            for g, dtype, pair in ROWS:
                out.append((bits, tile_p, g, dtype, pair, 256 + max(64, g), max(256, XC.cols_per_block(bits, tile_p))))
    return out


def nan_padded(rows, pad=PAD):
    """rows followed by `pad` rows of NaN"""
    return torch.cat([rows, torch.full((pad, rows.shape[1]), float("nan"), dtype=rows.dtype)])


def random_code_layer(env, bits, tile_p, dtype, K, N, seed, pair):
    """Random codes with an NF-style table or a random pair codebook (random_case's), packed on the device:
    (Q [P, K], table2, the lookups L [K, N] in fp64 from the codes)."""
    gen = torch.Generator().manual_seed(seed)
    n = 2 ** bits
    W = torch.randint(0, n, (K, N), generator=gen, dtype=torch.uint8)
    if pair:
        table2 = torch.randn(n * n, 2, generator=gen).to(dtype).view(n, n, 2).contiguous().view(torch.float32)
    else:
        table2 = env.O.make_qmap2_from_qmap(torch.randn(n, generator=gen).sort().values.to(dtype))
    Q = env.utils.pack(W.to(env.dev), bits, [first_template(bits, tile_p)], env.num_sms)
    pairs = env.O.table2_as_pairs(table2, dtype).double()
    return Q, table2.to(env.dev), SR.lut_of_codes(W.to(env.dev), pairs, bits)


@pytest.fixture(scope="module")
def tiny(env):
    """The smallest legal stacks (4 bits, TileP 32, g = 64, K = 64, N = 128; gate and up) over five rows of three
    experts, the middle one empty: offsets [0, 3, 3, 5], from moe_route at top-1."""
    d, dtype, bits, tile_p, g, K, N, E = env.dev, F16, 4, 32, 64, 64, 128, 3
    gen = torch.Generator().manual_seed(4100)

    def stack(seed):
        parts = [random_code_layer(env, bits, tile_p, dtype, K, N, seed + e, pair=(e == 1)) for e in range(E)]
        S = (torch.randn(E, N, K // g, generator=gen) / 8).to(dtype).to(d)
        return torch.stack([p[0] for p in parts]), S, torch.stack([p[1] for p in parts])

    ids = torch.tensor([[2], [0], [0], [2], [0]], dtype=torch.int32, device=d)
    offsets, rows, _, pos, _ = env.fa.moe_route(ids, None, E)
    assert offsets.tolist() == [0, 3, 3, 5]
    tokens = (torch.randn(5, K, generator=gen) / 4).to(dtype).to(d)
    return dict(gate=stack(4110), up=stack(4120), off=offsets, rows=rows, pos=pos, tokens=tokens,
                x_sorted=tokens.index_select(0, rows.long()), rw=(torch.rand(5, generator=gen) + 0.5).to(d),
                dY=torch.randn(5, N, generator=gen).to(dtype).to(d),
                args=(bits, g, first_template(bits, tile_p), env.num_sms))


QUANTUM = 2.0 ** -5          # x, dy multiples of 1/4, |s| in {1/2, 1, 2}: every term x dy s is a multiple


def exact_inputs(M, K, N, dtype, seed):
    """X and dY multiples of 1/4 in [-1, 1] (from 64 rows on: in [-1/4, 1/4], so that the larger sums stay exact)."""
    gen = torch.Generator().manual_seed(seed)
    amp = 4 if M < 64 else 1
    X = (torch.randint(-amp, amp + 1, (M, K), generator=gen).double() / 4).to(dtype)
    dY = (torch.randint(-amp, amp + 1, (M, N), generator=gen).double() / 4).to(dtype)
    return X, dY


def exact_scales(N, G, dtype, seed):
    """S = +-2^e, e in {-1, 0, 1}."""
    gen = torch.Generator().manual_seed(seed)
    e = torch.randint(-1, 2, (N, G), generator=gen).double()
    sign = torch.randint(0, 2, (N, G), generator=gen).double() * 2 - 1
    return (sign * torch.pow(2.0, e)).to(dtype)


def exact_premise(X, dY, S, codes, L, bits, g, dtype):
    """What makes the fp64 sums the only allowed answers: every term x dy s is a multiple of QUANTUM and every bin's
    sum of |terms| stays below 2^24 quanta, so each partial sum, in any order, is exact in fp32 (and G itself, whose
    terms are multiples of 1/16); the same for the scale gradient's sum of |dY X L| (integers / 16) before its one
    rounding to T.  Returns the references (dT2 [4^b, 2], dS [N, K / g]) in fp64."""
    for t in (X, dY):
        assert torch.equal(t.double() * 4, (t.double() * 4).round()) and t.abs().max() <= 1
    assert torch.equal(S.double().abs().log2(), S.double().abs().log2().round()) and S.abs().max() <= 2 and S.abs().min() >= 0.5
    A = TR.table_grad(dY, X, codes, S, bits, g, absolute=True)
    assert float(A.max()) / QUANTUM < 2.0 ** 24, ("a bin's sum of |terms| reaches 2^24 quanta", float(A.max()))
    As = SR.scale_grad(dY, X, L, g, absolute=True)
    assert float(As.max()) * 16 < 2.0 ** 24
    R = TR.table_grad(dY, X, codes, S, bits, g)
    Rs = SR.scale_grad(dY, X, L, g)
    assert torch.isfinite(Rs.to(dtype)).all()
    return R, Rs
