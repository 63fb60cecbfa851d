"""What the tests of the block form of the fused SwiGLU launch share (flute_amd.qgemm_grouped_glu_blocks; host and GPU): the
case matrix, the row draw, the fp64 reference with every premise of its bound asserted, and two exact stacks on the device.

The reference, the row draw and the case class restate `glu_reference`, `draw_rows` and `GluCase` of
tests/test_grouped_glu_gpu.py under other names: that file is a frozen test module, and test modules are not imported from
(README).  The bound itself is tests/grouped_cases.assert_glu, shared as it is."""
import torch

from tests import exact_cases as XC
from tests.grouped_cases import assert_glu, exact_layers, stack_exact
from tests.support import offsets_of

F16, BF16 = torch.float16, torch.bfloat16
# an empty first and middle expert, both sides of a 128-row block edge, three blocks with a ragged last one
BLOCK_COUNTS = [0, 1, 127, 128, 129, 0, 300]
# (K, g): 4, 8, 12 and 16 K steps - every exit of the ring unrolled by three - with one to three blocks of 8 scale groups
BLOCK_K_CASES = [(256, 32), (512, 32), (768, 32), (1024, 64)]
BLOCK_TSRC = 200                   # source rows: fewer than sorted rows, so `rows` repeats


def glu_blocks_matrix():
    """(bits, tile_p, dtype, K, g, F, pair): bits 4 / 2 x TileP 32 / 64 x fp16 / bf16 x BLOCK_K_CASES; F = 256 / 512 alternate (512
    where the layout's column block is 512 wide); a pair codebook on every fifth case."""
    out = []
    i = 0
    for bits in (4, 2):
        for tile_p in (32, 64):
            for dtype in (F16, BF16):
                for K, g in BLOCK_K_CASES:
                    F = 512 if (XC.cols_per_block(bits, tile_p) == 512 or i % 2) else 256
                    out.append((bits, tile_p, dtype, K, g, F, i % 5 == 3))
                    i += 1
    # 4 bits / TileP 64 / fp16 / K 256 would carry a pair codebook, and no seed of the 50 the search tries gives that stack an
    # accumulator witness (256 terms of a pair table stay exactly representable in fp16); its pair flag moves to K = 512
    moved = {(4, 64, F16, 256): False, (4, 64, F16, 512): True}
    return [c[:6] + (moved.get(c[:4], c[6]),) for c in out]


def glu_blocks_seed0(bits, tile_p, K):
    return 200000 + 1000 * bits + 10 * tile_p + K


def glu_block_rows(R, tsrc, seed):
    """R source rows with repeats; the last one is the accumulator witness (the last row of XC.make_x)."""
    rows = torch.randint(0, tsrc, (R,), generator=torch.Generator().manual_seed(seed))
    rows[-1] = tsrc - 1
    return rows


def _exact_in_fp32(x, lay, A, witness):
    """XC.premise without its demand that the product fits T: g and u stay in fp32 and are never rounded to T."""
    xd = x.double()
    assert torch.equal(xd, xd.round()) and xd.abs().max() <= 4, "activations: integers in [-4, 4]"
    w = lay.w_exact(0, min(lay.N, 256))
    assert torch.equal(w.to(lay.dtype).double(), w) and torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16
    assert float(A.max()) < XC.EXACT_SUM_LIMIT, ("sum |x w| reaches 2^21", float(A.max()))
    if witness:
        XC.assert_witness(xd[-1], w, lay.dtype)


def glu_block_reference(gate, up, segments, R, Xi, rows, need_witness=True):
    """For integer activations Xi [Tsrc, K] read through `rows` [R] and `segments` = [(expert, r0, r1)] - the sorted rows each
    expert serves; rows in no segment are not part of the reference -: the power p, X = Xi 2^-p in T, E [R, F] fp64 and the mask
    of the rows it covers, with every premise of assert_glu's bound asserted: g and u exact in fp32 whatever the summation
    order, |g| <= 88, a quarter of the elements with 0.25 <= |g| <= 8, and the accumulator witness in the segment that ends at R."""
    dtype = gate[0].dtype
    assert rows.shape == (R,) and int(rows[-1]) == Xi.shape[0] - 1
    G = torch.zeros(R, gate[0].N, dtype=torch.float64)
    U = torch.zeros_like(G)
    covered = torch.zeros(R, dtype=torch.bool)
    witnessed = False
    for e, r0, r1 in segments:
        if r1 <= r0:
            continue
        x = Xi[rows[r0:r1]]
        for lay, out in ((gate[e], G), (up[e], U)):
            P, A = XC.exact_product(x, lay, abs_too=True)
            _exact_in_fp32(x, lay, A, witness=(r1 == R))
            out[r0:r1] = P
        covered[r0:r1] = True
        witnessed |= r1 == R
    assert witnessed or not need_witness, "no segment ends at the witness row"
    Gc = G[covered]
    share = lambda p: float(((Gc.abs() * 2.0 ** -p >= 0.25) & (Gc.abs() * 2.0 ** -p <= 8)).double().mean())
    p = max((p for p in range(0, 20) if float(Gc.abs().max()) * 2.0 ** -p <= 88), key=share)     # silu32's eps_s holds for |g| <= 88
    X = (Xi.double() * 2.0 ** -p).to(dtype)
    assert torch.equal(X.double(), Xi.double() * 2.0 ** -p), "X 2^-p is exact in T"
    g, u = G * 2.0 ** -p, U * 2.0 ** -p
    E = g / (1 + torch.exp(-g)) * u
    assert share(p) >= 0.25, ("a quarter of the elements with 0.25 <= |g| <= 8", p, share(p))
    assert float(g.abs().max()) <= 88, float(g.abs().max())
    if dtype == F16:
        assert float(E.abs().max()) < XC.FP16_MAX / 2, float(E.abs().max())
    return dict(p=p, X=X, E=E, share=share(p), covered=covered)


def segments_of(counts):
    off = offsets_of(counts).tolist()
    return [(e, off[e], off[e + 1]) for e in range(len(counts))]


class GluBlockLayers:
    """Two exact stacks (gate: seed, up: seed + 500) on the CPU and the reference over them."""

    def __init__(self, bits, tile_p, g, dtype, K, F, pair, E, seed):
        self.bits, self.tile_p, self.g, self.dtype, self.K, self.F, self.E, self.seed = bits, tile_p, g, dtype, K, F, E, seed
        self.gate = exact_layers(bits, tile_p, g, dtype, K, F, pair, E, seed)
        self.up = exact_layers(bits, tile_p, g, dtype, K, F, pair, E, seed + 500)

    def reference(self, counts, Xi, rows, **kw):
        return glu_block_reference(self.gate, self.up, segments_of(counts), sum(counts), Xi, rows, **kw)


def premised_case(bits, tile_p, g, dtype, K, F, pair, counts, tsrc, seed0, tries=50):
    """(layers, Xi, rows, reference, tries used) from the first seed (seed0, seed0 + 1000, ..) at which every premise of the bound
    holds - at K = 256 not every draw of a table gives an accumulator witness or the share of |g| in [0.25, 8]."""
    last = None
    for i in range(tries):
        seed = seed0 + 1000 * i
        layers = GluBlockLayers(bits, tile_p, g, dtype, K, F, pair, len(counts), seed)
        Xi = XC.make_x(tsrc, K, seed + 77, dtype)
        rows = glu_block_rows(sum(counts), tsrc, seed + 78)
        try:
            return layers, Xi, rows, layers.reference(counts, Xi, rows), i + 1
        except AssertionError as err:
            last = err
    raise AssertionError("no seed in %d meets every premise: %s" % (tries, last))


class GluBlockCase:
    """GluBlockLayers on the device, and the two launches over them."""

    def __init__(self, env, layers):
        self.env, self.lay = env, layers
        self.Qg, self.Sg, self.Tg, self.tid = stack_exact(env, layers.gate)
        self.Qu, self.Su, self.Tu, _ = stack_exact(env, layers.up)

    def ops(self):
        return (self.Qg, self.Sg, self.Tg, self.Qu, self.Su, self.Tu)

    def run(self, X, off, rows, blocks=True):
        op = self.env.fa.qgemm_grouped_glu_blocks if blocks else self.env.fa.qgemm_grouped_glu
        return op(X, off, *self.ops(), self.lay.bits, self.lay.g, self.tid, self.env.num_sms, rows=rows)

    def check(self, counts, ref, rows, what, use_rows=True):
        """The block launch on the reference's X against assert_glu's bound; returns H."""
        d = self.env.dev
        H = self.run(ref["X"].to(d), offsets_of(counts, d), rows.int().to(d) if use_rows else None)
        assert H.shape == (sum(counts), self.lay.F) and H.dtype == self.lay.dtype
        assert_glu(H, ref["E"], self.lay.dtype, (what, "p = %d" % ref["p"], "share %.2f" % ref["share"]))
        return H
