"""Inputs whose exact product every kernel must return bit for bit, and the checkers built on them.

A test helper module (not a conftest): `tests/test_exact_cases.py` checks the checkers on the CPU,
`tests/test_exact_gpu.py` runs them against the kernels.

Exact by construction
---------------------
codes W[K, N] in [0, 2^b); an integer table |t| <= 8 (or an integer 4^b x 2 pair codebook, the HIGGS
vector_size = 2 case); scales +-2^e with e in [-3, 1] per (column, group); activations integers in [-4, 4].
Every weight lut * s is then exact in fp16 and bf16, every product x * w is a multiple of 2^-3 with
|x * w| <= 64, and while sum_k |x_k w_k| < 2^21 every partial sum, in any order, is exact in fp32.  The
kernels' documented arithmetic (include/flute_amd.h: w^ = round_T(lut * s) or the scale applied in fp32 to
an fp32 partial sum; fp32 accumulation; one rounding of the output) then allows exactly one answer,
round_T(X @ W_exact), whatever the family, split or summation order.  `premise()` asserts this for every
case it is given, and that the last row of X (the accumulator witness, every entry 4) has running partial
sums that an accumulator in T could not hold.

Where exactness is impossible (random NF4 data, the 1 / sqrt(512) rotation) `assert_componentwise` checks
a per-element bound that follows from the same documented arithmetic (see its docstring).
"""
import zlib

import torch

U_T = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}       # unit roundoff of the output type
NAN_BITS = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0}
FP16_MAX = 65504.0
EXACT_SUM_LIMIT = 2.0 ** 21        # |partial sum| < 2^21 in multiples of 2^-3: 24 significand bits


def cols_per_block(bits, tile_p):
    return tile_p * (16 if bits == 3 else 16 // bits)


class Layer:
    """One quantized weight matrix, exact by construction, generated from `seed` on the CPU."""

    def __init__(self, bits, K, N, g, dtype, seed, tile_p=32, pair=False, table_div=1, scale_exp=(-3, 1)):
        """`table_div`: the table is k / table_div, integer |k| <= 8; `scale_exp`: scales +-2^e, e in [lo, hi] (both inclusive)."""
        assert K % g == 0 and N % cols_per_block(bits, tile_p) == 0, (bits, K, N, g, tile_p)
        self.bits, self.K, self.N, self.g, self.dtype, self.seed, self.tile_p, self.pair = bits, K, N, g, dtype, seed, tile_p, pair
        self.table_div, self.scale_exp = table_div, tuple(scale_exp)
        gen = torch.Generator().manual_seed(seed)
        n = 2 ** bits
        self.W = torch.randint(0, n, (K, N), generator=gen, dtype=torch.uint8)
        if pair:
            self.pairs = torch.randint(-8, 9, (n * n, 2), generator=gen).double() / table_div
            self.table = self.pairs[:n, 0].to(dtype)                     # not read by the kernels (the reference's contract)
            self.table2 = self.pairs.to(dtype).view(n, n, 2).contiguous().view(torch.float32)
        else:
            t = torch.randint(-8, 9, (n,), generator=gen).double() / table_div
            self.pairs = torch.stack([t[:, None].expand(n, n), t[None, :].expand(n, n)], dim=-1).reshape(n * n, 2)
            self.table = t.to(dtype)
            q = self.table
            self.table2 = torch.stack([q[:, None].expand(n, n), q[None, :].expand(n, n)], dim=-1).contiguous().view(torch.float32)
        e = torch.randint(scale_exp[0], scale_exp[1] + 1, (N, K // g), generator=gen).double()
        sign = torch.randint(0, 2, (N, K // g), generator=gen).double() * 2 - 1
        self.S64 = sign * torch.pow(2.0, e)
        self.S = self.S64.to(dtype)
        assert torch.equal(self.S.double(), self.S64) and torch.equal(self.pairs.to(dtype).double(), self.pairs)

    def key(self):
        return (self.bits, self.K, self.N, self.g, str(self.dtype)[6:], self.seed, self.tile_p, self.pair)

    def __repr__(self):
        return "Layer(b=%d K=%d N=%d g=%d %s seed=%d P=%d%s)" % (
            self.bits, self.K, self.N, self.g, str(self.dtype)[6:], self.seed, self.tile_p, " pair" if self.pair else "")

    def w_exact(self, n0=0, n1=None, device="cpu"):
        """W_exact[:, n0:n1] = lut * scale in fp64, from the codes (no packer): the pair index of rows (2 kappa,
        2 kappa + 1) is W[2 kappa] << b | W[2 kappa + 1] (flute/utils.py:77-84), element e of the pair is row 2 kappa + e."""
        n1 = self.N if n1 is None else n1
        W = self.W[:, n0:n1].to(device).long()
        idx = (W[0::2] << self.bits) | W[1::2]
        w = self.pairs.to(device)[idx]                                   # [K/2, n, 2]
        w = w.permute(0, 2, 1).reshape(self.K, n1 - n0)
        return w * torch.repeat_interleave(self.S64[n0:n1].to(device), self.g, dim=1).T


def make_x(M, K, seed, dtype, witness=True):
    """Integer activations in [-4, 4]; the last row is the accumulator witness (every entry 4)."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.randint(-4, 5, (M, K), generator=gen).double()
    if witness:
        X[-1] = 4
    return X.to(dtype)


def exact_product(X, layer, device="cpu", chunk=4096, abs_too=False, flush_w=False, flush_x=False):
    """R = X @ W_exact in fp64 (and |X| @ |W_exact| with abs_too), over column chunks.  flush_w / flush_x: the product with
    the fp16 subnormal weights / activations replaced by zero (what a kernel that flushes them would return)."""
    Xd = X.to(device).double()
    if flush_x:
        Xd = flush_subnormal_f16(Xd)
    R, A = [], []
    for n0 in range(0, layer.N, chunk):
        Wc = layer.w_exact(n0, min(layer.N, n0 + chunk), device)
        if flush_w:
            Wc = flush_subnormal_f16(Wc)
        R.append(Xd @ Wc)
        if abs_too:
            A.append(Xd.abs() @ Wc.abs())
    R = torch.cat(R, 1)
    return (R, torch.cat(A, 1)) if abs_too else R


def _is_T(v, dtype):
    return torch.equal(v.to(dtype).double(), v)


def premise(X, layer, R, A, witness=True):
    """Assert what makes round_T(R) the only allowed answer; R, A = exact_product(..., abs_too=True)."""
    dtype = layer.dtype
    Xd = X.double().cpu()
    assert _is_T(Xd, dtype) and torch.equal(Xd, Xd.round()) and Xd.abs().max() <= 4, "activations: integers in [-4, 4]"
    w = layer.w_exact(0, min(layer.N, 256))
    assert _is_T(w, dtype) and torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16, "weights: exact, multiples of 2^-3"
    assert float(A.max()) < EXACT_SUM_LIMIT, ("sum |x w| reaches 2^21", float(A.max()))
    assert torch.isfinite(R.to(dtype)).all()
    if dtype == torch.float16:
        assert float(R.abs().max()) <= FP16_MAX, float(R.abs().max())
    if witness:
        assert_witness(Xd[-1], w, dtype)


def assert_witness(x, w, dtype, cols=64):
    """The witness row x against columns w[:, :cols]: summed in order with an accumulator in T (every partial sum
    rounded to T) it ends away from round_T(exact) in some column, so a kernel that accumulates in T fails."""
    w = w[:, :cols]
    exact = (x[None, :] @ w)[0]
    acc = torch.zeros(w.shape[1], dtype=dtype)
    xt, wt = x.to(dtype), w.to(dtype)
    for k in range(w.shape[0]):
        acc = (acc.double() + (xt[k] * wt[k]).double()).to(dtype)
    assert not torch.equal(acc.double(), exact.to(dtype).double()), "witness row does not need an fp32 accumulator"


def exact_equal(D, R, dtype):
    """By value (a kernel may return -0.0 where round_T(R) is +0.0)."""
    return torch.equal(D.double().cpu(), R.to(dtype).double().cpu())


def gamma(n):
    v = n * 2.0 ** -24
    assert v < 0.5
    return v / (1 - v)


def componentwise_excess(D, R, A, K, dtype, extra=0.0):
    """max over elements of |D - R| - bound (<= 0: within the bound).

    D = round_T(C) with C the fp32 result of at most K + 16 operations per element on the weights
    w^ = round_T(lut * s) = W_exact (1 + d), |d| <= u_T (decode kernels: no weight rounding, the scale applied
    in fp32 - inside the same bound).  So |C - R| <= E = (u_T + (1 + u_T) gamma_{K+16}) A with
    A = |X| @ |W_exact|, and |D - C| <= u_T |C| + tiny, hence
        |D - R| <= u_T |R| + (1 + u_T) E + tiny.
    To first order this is u_T |R| + (u_T + (K + 16) 2^-24) A + tiny.  `extra` adds c A for callers whose
    activations are themselves rounded (the Hadamard rotation)."""
    u = U_T[dtype]
    c = (1 + u) * (u + (1 + u) * gamma(K + 16)) + extra
    tiny = 2.0 ** -24
    D = D.double().to(R.device)
    return float(((D - R).abs() - (u * R.abs() + c * A + tiny)).max())


def assert_componentwise(D, X, What_exact, K, dtype, extra=0.0, what=None):
    """|D - R| <= u_T |R| + (u_T + (K + 16) 2^-24) |X| @ |W| + tiny, element by element (componentwise_excess),
    R = X @ What_exact in fp64 with What_exact the exact lut * s weight."""
    Xd = X.double().to(What_exact.device)
    W = What_exact.double()
    R = Xd @ W
    A = Xd.abs() @ W.abs()
    ex = componentwise_excess(D, R, A, K, dtype, extra)
    assert ex <= 0, ("componentwise bound", what, ex)


# ---------------------------------------------------------------------------
# the forced-plan matrix: (layer, M, overrides, what the plan must say)
# ---------------------------------------------------------------------------

F16, BF16 = torch.float16, torch.bfloat16
ONE_SHOT_CODE = {0: 0, 1: 1, 2: 3, 4: 4}        # override one_shot -> flute_plan.one_shot


def _lay(bits, K, N, g, dtype, tile_p=32, pair=False):
    return dict(bits=bits, K=K, N=N, g=g, dtype=dtype, tile_p=tile_p, pair=pair)


def forced_matrix():
    """[(family, layer kwargs, M, overrides, expected plan fields)], one entry per launch.  Shapes sit at the families'
    legal edges: ragged M, N an odd multiple of the column block where the family takes it (the smallest legal N
    included), K not a multiple of 1024, the 28672 x 8192 and 8192 x 28672 layers at M = 4 and 16."""
    out = []

    def add(fam, lay, Ms, ovr, exp):
        for M in Ms:
            out.append((fam, lay, M, dict(ovr), dict(exp, family=fam)))

    # family 0, the decode kernels: ring (one_shot 0), one-shot (1; reported 2 for one row: the pipelined form), persistent
    # one-shot (2 and 3, M <= 2; reported 3), lean (4); rows per pass (m_block) 1 / 2 / 4 - at least the next power of two of M
    for lay in (_lay(4, 4096, 512, 64, F16), _lay(4, 2048, 3 * 1024, 128, BF16, 64), _lay(2, 4416, 3 * 256, 64, F16),
                _lay(3, 3072, 3 * 512, 32, BF16), _lay(4, 8192, 3 * 128, 256, BF16), _lay(4, 3584, 3 * 512, 64, F16, pair=True),
                _lay(2, 2048, 3 * 512, 128, BF16, 64, pair=True)):
        for one in (0, 1, 2, 3, 4):
            if one == 4 and (lay["bits"] != 4 or lay["g"] < 64):
                continue
            # (the one-shot kernels need whole 512-k pieces, 4 bits or group size >= 64; the persistent one needs an even group count)
            if one in (1, 2, 3) and (lay["K"] % 512 or lay["g"] < 64 or lay["bits"] == 2 and lay["tile_p"] == 32):
                continue
            if one in (2, 3) and lay["pair"]:
                continue
            for mb in (1, 2, 4):
                for M in (1, 2, 3, 4):
                    rows = 1 << (M - 1).bit_length()
                    if one in (2, 3) and (M > 2 or mb > 1 or lay["g"] == 256):
                        continue
                    if one == 4 and (mb > 1 or max(rows, 1) * lay["K"] * 2 > 32768):
                        continue
                    code = {0: 0, 1: (1, 2), 2: 3, 3: 3, 4: 4}[one]       # (one_shot 1 at one row: either one-shot form)
                    exp = dict(one_shot=code)
                    if one == 0:
                        exp["m_block"] = max(mb, rows)
                    add(0, lay, (M,), dict(family=0, one_shot=one, m_block=mb), exp)
    # family 2, the per-wave MFMA kernel: 16-row tiles per wave, column slabs per wave, in-workgroup K split, grid K split
    # combined inside the launch (splitk_mode 1) or by the reduce launch (0)
    for lay in (_lay(4, 4096 + 320, 3 * 512, 64, F16), _lay(2, 2048, 3 * 1024, 128, BF16, 64), _lay(3, 2048 + 64, 3 * 512, 64, F16),
                _lay(4, 3584, 1024, 32, BF16)):
        for mt, sl, kw, sk in ((1, 1, 1, 1), (2, 1, 2, 1), (4, 1, 1, 1), (1, 1, 4, 3), (4, 1, 2, 4), (2, 1, 8, 2)):
            if lay["bits"] == 3:
                continue
            add(2, lay, (5, 17, 129, 700), dict(family=2, m_tiles=mt, slabs_per_wave=sl, kw=kw, splitk=sk),
                dict(m_tiles=mt, slabs_per_wave=sl, kw=kw, splitk=sk))
    for mt, sl, kw, sk in ((1, 1, 4, 1), (1, 1, 8, 2), (1, 1, 4, 3)):          # 3 bits: one row tile per wave
        add(2, _lay(3, 2048 + 64, 3 * 512, 64, F16), (5, 17, 129, 700), dict(family=2, m_tiles=mt, slabs_per_wave=sl, kw=kw, splitk=sk),
            dict(m_tiles=mt, slabs_per_wave=sl, kw=kw, splitk=sk))
    add(2, _lay(4, 4096 + 320, 3 * 512, 64, F16), (700,), dict(family=2, m_tiles=4, slabs_per_wave=2, kw=4, splitk=1),
        dict(m_tiles=4, slabs_per_wave=2, kw=4, splitk=1))
    # family 3, the block prefill kernels: 256- / 128-row blocks (m_block 4 / 5), with a grid K split; 3-bit blocks of 1 / 2 / 4 row
    # tiles (m_block 8 + rt) with K slices
    for lay in (_lay(4, 4096, 1536, 64, F16), _lay(2, 2048, 1536, 128, BF16, 64), _lay(4, 1024, 256, 32, BF16)):
        for mt, sk in ((8, 1), (4, 1), (8, 2), (4, 2)):
            add(3, lay, (1, 129, 257, 700), dict(family=3, m_tiles=mt, splitk=sk), dict(m_block=4 if mt == 8 else 5, splitk=sk))
    for lay in (_lay(3, 2048, 1024, 64, BF16), _lay(3, 3072, 512, 128, F16)):
        for mt, sk in ((8, 1), (4, 2)):
            add(3, lay, (13, 257), dict(family=3, m_tiles=mt, splitk=sk), dict(m_block=4 if mt == 8 else 5, splitk=sk))
        for rt, sk in ((1, 1), (2, 2), (4, 2), (1, 2)):
            add(3, lay, (5, 17, 33, 65), dict(family=3, m_block=rt, splitk=sk), dict(m_block=8 + rt, splitk=sk))
    # family 5, the skinny MFMA kernel: 4 / 8 waves (K = 32 x depth x waves)
    for lay, waves in ((_lay(4, 2048, 3 * 128, 64, F16), 4), (_lay(4, 1024, 3 * 256, 32, BF16, 64), 4), (_lay(4, 4096, 3 * 128, 128, BF16), 8),
                       (_lay(4, 1024, 256, 256, F16, 64), 8), (_lay(4, 4096, 1024, 64, F16, pair=True), 8)):
        add(5, lay, (1, 3, 7, 16), dict(family=5, waves=waves), dict(waves=waves))
    # family 6, the split-K block kernel: K slices 1 .. 16 x (row tiles, K parts per workgroup) x block order
    for lay in (_lay(4, 4096, 3 * 256, 64, F16), _lay(2, 3072, 3 * 512, 128, BF16, 64), _lay(4, 2048, 256, 32, BF16)):
        for sk in (1, 2, 3, 4, 6, 8, 16):
            for rt, kp in ((8, 2), (4, 2), (4, 4)):
                # (not every split is legal for every K: qgemm_splitk.h's host contract refuses the others - FLUTE_ERR_SHAPE)
                add(6, lay, (17, 257), dict(family=6, splitk=sk, m_tiles=rt, kw=kp), dict(splitk=sk, m_tiles=rt, kw=kp, may_refuse=True))
        for mb in (2, 4):
            add(6, lay, (257,), dict(family=6, splitk=1, m_tiles=4, kw=2, m_block=mb), dict(splitk=1, m_tiles=4, kw=2))
    # family 7, the lean MFMA decode kernel: 1 .. 3 column groups per workgroup, K = 2048 / 4096
    for lay in (_lay(4, 4096, 11008 // 128 * 128, 64, F16), _lay(4, 2048, 5248, 128, BF16), _lay(4, 4096, 1024, 256, BF16, pair=True)):
        for ng in (1, 2, 3):
            add(7, lay, (5, 13, 16), dict(family=7, slabs_per_wave=ng), dict(slabs_per_wave=ng))
    # family 8, the persistent MFMA decode kernel: 1 .. 3 column groups per set, sets per workgroup (override m_tiles), the activations
    # resident (one_shot 1) or through the rings (0), 2 / 4 bits, group size 64 / 128
    for lay in (_lay(4, 1152, 5248, 64, F16), _lay(2, 3584, 3 * 512, 128, BF16, 64), _lay(4, 8192, 1024, 128, BF16), _lay(2, 1280, 3 * 256, 64, F16, pair=True)):
        for ng in (1, 2, 3):
            for vis in (-1, 1, 3):
                for res in (-1, 0):
                    if vis == 1 and -(-lay["N"] // 16 // ng) > 256:      # one set per workgroup would need more workgroups than CUs
                        continue
                    exp = dict(slabs_per_wave=ng)
                    if vis > 0:
                        exp["visits"] = vis
                    if res == 0:
                        exp["one_shot"] = 0
                    add(8, lay, (3, 7, 16), dict(family=8, slabs_per_wave=ng, m_tiles=vis, one_shot=res), exp)
    # the full-size layers (BASELINE.json configs[2] / [3] shapes) at M = 4 and 16
    for lay in (_lay(4, 8192, 28672, 64, F16), _lay(4, 28672, 8192, 64, BF16)):
        add(8, lay, (4, 16), dict(family=8), dict())
        add(2, lay, (4, 16), dict(family=2), dict())
        add(6, lay, (16,), dict(family=6), dict())
    add(8, _lay(4, 8192, 28672, 64, F16), (4,), dict(family=8, m_tiles=4), dict(visits=4))
    add(0, _lay(4, 8192, 28672, 64, F16), (4,), dict(family=0), dict())
    return out


# the families the planner picks by itself (256 CUs); auto_grid() must reach every one of them
AUTO_FAMILIES = {0, 2, 3, 5, 6, 7, 8}


def auto_grid():
    """[(layer kwargs, M)] for the automatic plans: BASELINE.json configs[0..4] (configs[3]: one TP = 8 shard of
    8192 x 28672, configs[4]: the pair codebook on Gemma-2-9B shapes) and shapes that make the planner pick each family."""
    out = [
        (_lay(4, 4096, 4096, 64, F16), 1),                                                       # configs[0]
        (_lay(4, 4096, 4096, 64, F16), 16), (_lay(4, 4096, 4096, 64, F16), 256),                 # configs[1]
        (_lay(4, 4096, 11008 // 128 * 128, 64, F16), 1), (_lay(4, 4096, 11008 // 128 * 128, 64, F16), 16),
        (_lay(4, 4096, 11008 // 128 * 128, 64, F16), 256),
        (_lay(3, 8192, 8192, 64, BF16), 1), (_lay(3, 8192, 8192, 64, BF16), 64), (_lay(3, 8192, 10240, 64, BF16), 16),   # configs[2]
        (_lay(4, 8192, 28672 // 8, 64, F16), 1), (_lay(4, 8192, 28672 // 8, 64, F16), 16),       # configs[3]
        (_lay(4, 3584, 4096, 64, BF16, pair=True), 1), (_lay(4, 3584, 4096, 64, BF16, pair=True), 16),   # configs[4]
        (_lay(4, 4096, 14336, 64, F16), 16),                                                     # skinny MFMA kernel
        (_lay(4, 8192, 8192, 64, F16), 4),                                                       # persistent MFMA decode
        (_lay(4, 4096, 4096, 64, BF16), 2048),                                                   # block prefill
        (_lay(2, 8192, 28672, 64, F16), 16),                                                     # per-wave MFMA kernel
        (_lay(2, 4096, 4096, 64, F16), 2), (_lay(4, 4096, 4096, 64, F16), 7), (_lay(4, 4096, 4096, 64, F16), 700),
    ]
    return out


# ---------------------------------------------------------------------------
# the fp16 range edges and non-finite rows (tests/test_value_edges_gpu.py)
# ---------------------------------------------------------------------------
#
# Three kinds of exact case outside the region above, each still with ONE allowed answer round_T(X @ W_exact) under both
# documented forms of the arithmetic (the weight rounded to T; the scale applied in fp32 to an fp32 partial sum):
#   "subw"      fp16 weights below 2^-14: table k / 64, scales +-2^e with e in [-12, -10] (table and scales are normal
#               numbers, most products lut * s are subnormal, all are exact), integer activations in [-4, 4]
#   "subx"      fp16 activations j 2^-20, integer j in [-4, 4] (all subnormal), on an ordinary exact layer
#   "overflow"  an ordinary exact layer; rows of X are +-a sign(w[:, n]): the exact result passes 65520 in both
#               directions, so round_T(R) holds +inf and -inf (IEEE round to nearest, not 65504), and one row stays
#               finite above 2^15
# and "nonfinite": one NaN and one +Inf in X (fp16 and bf16), the expectation built by rule (nonfinite_expected).
# `premise_edge` asserts for each what makes the answer unique.

MIN_NORMAL_F16 = 2.0 ** -14
SUBW = dict(table_div=64, scale_exp=(-12, -10))
OVERFLOW_K = 4096                      # 4 sum |w| over one column must pass 65520: K = 4096 with scales +-1, +-2
OVERFLOW = dict(scale_exp=(0, 1))      # (weights still multiples of 2^-3 with |w| <= 16: premise() holds unchanged)
EDGE_KINDS = ("subw", "subx", "overflow", "nonfinite")


def is_subnormal_f16(v):
    return (v != 0) & (v.abs() < MIN_NORMAL_F16)


def flush_subnormal_f16(v):
    """v with its fp16 subnormals replaced by zero: what an instruction that flushes such operands multiplies."""
    return torch.where(is_subnormal_f16(v), torch.zeros_like(v), v)


def make_x_subnormal(M, K, seed):
    """fp16 activations j 2^-20, j integer in [-4, 4]; the last row is the witness (every j 4)."""
    return (make_x(M, K, seed, torch.float16).double() * 2.0 ** -20).to(torch.float16)


def make_x_overflow(M, layer, seed, cols=256):
    """Integer activations in [-4, 4], M >= 3: row 0 = 4 sign(w[:, n0]) and row 1 = -row 0, n0 the column of the first
    `cols` with the largest sum |w| (the exact result there is +-4 sum |w|); row 2 = a sign(w[:, n2]) with the first
    (a, n2), a = 3, 2, 1, for which 2^15 <= a sum |w[:, n2]| < 65520; the other rows random."""
    assert M >= 3
    X = make_x(M, layer.K, seed, layer.dtype, witness=False).double()
    w = layer.w_exact(0, min(layer.N, cols))
    c = w.abs().sum(0)
    n0 = int(c.argmax())
    sgn = lambda n: torch.where(w[:, n] < 0, -1.0, 1.0).double()
    X[0] = 4 * sgn(n0)
    X[1] = -X[0]
    for a in (3, 2, 1):
        ok = ((a * c >= 2.0 ** 15) & (a * c < 65520.0)).nonzero()
        if len(ok):
            X[2] = a * sgn(int(ok[0]))
            break
    else:
        raise AssertionError("no column whose a sum |w| lies in [2^15, 65520)")
    return X.to(layer.dtype)


def _exact_in_fp32(X, layer, A, ux, ulut):
    """Every product is a multiple of u = ux ulut 2^emin and sum |x w| < 2^24 u, so every partial sum of the weight-rounded form
    is exact in fp32; a group's sum of x lut (the other form, scaled in fp32 by a power of two afterwards) is a multiple
    of ux ulut below 2^24 ux ulut."""
    u = ux * ulut * 2.0 ** layer.scale_exp[0]
    assert float(A.max()) < u * 2.0 ** 24, ("sum |x w| not exact in fp32", float(A.max()), u)
    assert layer.g * float(X.abs().max()) * float(layer.pairs.abs().max()) < ux * ulut * 2.0 ** 24


def premise_edge(kind, X, layer, R, A):
    """What makes round_T(R) the one allowed answer for an edge case of `kind`, and that the case sits at its edge;
    R, A = exact_product(..., abs_too=True).  premise()'s conditions are kept wherever the kind does not replace them."""
    T = layer.dtype
    Xd = X.double().cpu()
    w = layer.w_exact(0, min(layer.N, 256))
    Rt = R.to(T).double()
    assert _is_T(Xd, T) and _is_T(w, T), "operands exact in T"
    if kind == "subw":
        assert T == torch.float16 and layer.table_div == 64
        assert torch.equal(Xd, Xd.round()) and Xd.abs().max() <= 4, "activations: integers in [-4, 4]"
        t, s = layer.pairs, layer.S64
        assert not is_subnormal_f16(t).any() and not is_subnormal_f16(s).any(), "table and scales are normal numbers"
        assert torch.equal(w * 2.0 ** 18, (w * 2.0 ** 18).round()) and w.abs().max() <= 2.0 ** -13
        assert float(is_subnormal_f16(w).double().mean()) >= 0.5, "at least half the weights subnormal"
        assert float(A.max()) <= 2.0 * layer.K / 4096
        _exact_in_fp32(Xd, layer, A, 1.0, 2.0 ** -6)
        assert is_subnormal_f16(Rt).any(), "some outputs subnormal"
    elif kind == "subx":
        assert T == torch.float16 and layer.table_div == 1 and layer.scale_exp == (-3, 1)
        j = Xd * 2.0 ** 20
        assert torch.equal(j, j.round()) and j.abs().max() <= 4 and is_subnormal_f16(Xd).any()
        assert torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16, "weights: exact, multiples of 2^-3"
        _exact_in_fp32(Xd, layer, A, 2.0 ** -20, 1.0)
    elif kind == "overflow":
        assert T == torch.float16 and layer.table_div == 1 and layer.scale_exp[0] >= -3 and layer.scale_exp[1] <= 1
        assert torch.equal(Xd, Xd.round()) and Xd.abs().max() <= 4, "activations: integers in [-4, 4]"
        assert torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16, "weights: exact, multiples of 2^-3"
        assert float(A.max()) < EXACT_SUM_LIMIT, ("sum |x w| reaches 2^21", float(A.max()))
        fin = torch.isfinite(Rt)
        assert (Rt == float("inf")).any() and (Rt == -float("inf")).any(), "round_T(R) holds +inf and -inf"
        assert (fin & (R.abs() >= 2.0 ** 15)).any(), "a finite output above 2^15"
    else:
        raise ValueError(kind)
    assert not torch.isnan(Rt).any()


def poison_x(X, m_nan, m_inf, k_nan, k_inf):
    """X with one NaN in row m_nan and one +Inf in row m_inf."""
    X = X.clone()
    X[m_nan, k_nan] = float("nan")
    X[m_inf, k_inf] = float("inf")
    return X


def nonfinite_expected(D_clean, layer, m_nan, m_inf, k_inf):
    """The one allowed answer for poison_x(X, ...), by rule (no matmul on non-finite data): the NaN row all NaN; the Inf
    row NaN where w[k_inf, n] == 0 (inf x 0), +inf where it is positive, -inf where negative (every other term is
    finite); every other row the bits of the clean launch D_clean."""
    exp = D_clean.clone().cpu()
    w = layer.w_exact()[k_inf]
    exp[m_nan] = float("nan")
    exp[m_inf] = torch.where(w == 0, float("nan"), torch.where(w > 0, float("inf"), -float("inf"))).to(exp.dtype)
    return exp


def nonfinite_equal(D, exp):
    """Bit for bit, with every NaN equal to every NaN."""
    D, exp = D.cpu(), exp.cpu()
    nd, ne = torch.isnan(D), torch.isnan(exp)
    return torch.equal(nd, ne) and torch.equal(D.masked_fill(nd, 0).view(torch.int16), exp.masked_fill(ne, 0).view(torch.int16))


def edge_variants(family):
    """[(layer kwargs, M, overrides, expected plan fields)] for the edge kinds: the smallest layers of the family's section of
    forced_matrix() as fp16 layers, one per bit width the family serves, at one ragged M (family 0: M = 3, its
    persistent one-shot kernel M = 2; family 2's reduce launch: the M that needs it), once per way of combining K the family has
    (no split / inside the workgroup / grid split inside the launch / reduce launch; family 0: once per one_shot code).
    `assert_edge_coverage` states what that must amount to."""
    out = []

    def add(lay, M, ovr, exp):
        out.append((lay, M, dict(ovr, family=family), dict(exp, family=family)))

    if family == 0:
        for lay, ones in ((_lay(4, 4096, 512, 64, F16), (0, 1, 2, 4)), (_lay(2, 2048, 3 * 512, 128, F16, 64), (0, 1, 2)),
                          (_lay(3, 3072, 3 * 512, 32, F16), (0,))):
            for one in ones:
                M = 2 if one == 2 else 3
                exp = dict(one_shot={0: 0, 1: (1, 2), 2: 3, 4: 4}[one])
                if one == 0:
                    exp["m_block"] = 4
                add(lay, M, dict(one_shot=one, m_block=1), exp)
    elif family == 2:
        for lay, vs in ((_lay(4, 3584, 1024, 32, F16), ((1, 1, 1, 1), (2, 1, 2, 1), (1, 1, 4, 3), (2, 1, 8, 2))),
                        (_lay(2, 2048, 3 * 1024, 128, F16, 64), ((1, 1, 1, 1), (2, 1, 2, 1), (1, 1, 4, 3), (2, 1, 8, 2))),
                        (_lay(3, 2048 + 64, 3 * 512, 64, F16), ((1, 1, 4, 1), (1, 1, 8, 2), (1, 1, 4, 3)))):
            for mt, sl, kw, sk in vs:
                v = dict(m_tiles=mt, slabs_per_wave=sl, kw=kw, splitk=sk)
                add(lay, 17, v, v)
            # the reduce launch (splitk_mode 0): the planner meets inside the launch while splitk M N fp32 slabs stay within 4 MB,
            # so one ragged M just past that for three K slices
            M0 = (4 << 20) // (3 * lay["N"] * 4) + 1
            M0 += M0 % 16 == 0
            v = dict(m_tiles=1, slabs_per_wave=1, kw=4, splitk=3)
            add(lay, M0, v, dict(v, splitk_mode=0))
    elif family == 3:
        for lay in (_lay(4, 1024, 256, 32, F16), _lay(2, 2048, 1536, 128, F16, 64)):
            for mt, sk in ((4, 1), (4, 2), (8, 2)):
                add(lay, 129, dict(m_tiles=mt, splitk=sk), dict(m_block=4 if mt == 8 else 5, splitk=sk))
        lay = _lay(3, 2048, 1024, 64, F16)
        for mt, sk in ((8, 1), (4, 2)):
            add(lay, 13, dict(m_tiles=mt, splitk=sk), dict(m_block=4 if mt == 8 else 5, splitk=sk))
        for rt, sk in ((1, 1), (2, 2), (4, 2)):
            add(lay, 17, dict(m_block=rt, splitk=sk), dict(m_block=8 + rt, splitk=sk))
    elif family == 5:
        add(_lay(4, 2048, 3 * 128, 64, F16), 7, dict(waves=4), dict(waves=4))
        add(_lay(4, 1024, 256, 256, F16, 64), 7, dict(waves=8), dict(waves=8))
    elif family == 6:
        for lay in (_lay(4, 2048, 256, 32, F16), _lay(2, 3072, 3 * 512, 128, F16, 64)):
            for sk in (1, 2, 4):
                v = dict(splitk=sk, m_tiles=4, kw=2)
                add(lay, 17, v, dict(v, may_refuse=True))          # (not every split is legal for every K, as in forced_matrix)
    elif family == 7:
        for ng in (1, 2, 3):
            add(_lay(4, 4096, 1024, 256, F16, pair=True), 13, dict(slabs_per_wave=ng), dict(slabs_per_wave=ng))
    elif family == 8:
        for lay in (_lay(4, 1152, 5248, 64, F16), _lay(2, 1280, 3 * 256, 64, F16, pair=True)):
            for ng, vis, res in ((1, -1, -1), (2, -1, 0), (3, 3, -1)):
                exp = dict(slabs_per_wave=ng)
                if vis > 0:
                    exp["visits"] = vis
                if res == 0:
                    exp["one_shot"] = 0
                add(lay, 7, dict(slabs_per_wave=ng, m_tiles=vis, one_shot=res), exp)
    return out


def edge_way(family, bits, plan):
    """How a planned launch combines K: (bits, one_shot code) for family 0, else (bits, K split inside the workgroup,
    splitk_mode of a grid split or -1 without one)."""
    if family == 0:
        return (bits, plan["one_shot"])
    return (bits, plan["kw"] > 1, plan["splitk_mode"] if plan["splitk"] > 1 else -1)


def assert_edge_coverage(family, kind, cases, ways):
    """`ways`: the edge_way of every case of (family, kind) that was planned (host test) or launched (GPU test).  Every bit
    width of the cases is there; families 2, 3 and 6 run without a grid split and with one that meets inside the launch,
    families 2 and 3 also through the reduce launch (family 6 has none); family 0 runs every one_shot code its kind admits."""
    assert {w[0] for w in ways} == {kw["bits"] for kw, _, _, _ in cases}, (family, kind, ways)
    if family in (2, 3, 6):
        modes = {w[2] for w in ways}
        assert modes >= ({-1, 1} if family == 6 else {-1, 0, 1}), (family, kind, ways)
    if family == 2:
        assert all((b, True, 0) in ways for b in (2, 3, 4)), (family, kind, ways)
    if family == 0:
        codes = {1 if w[1] == 2 else w[1] for w in ways}              # (2: the pipelined form of the one-shot kernel)
        assert codes >= ({0, 1, 3, 4} if kind in ("subw", "subx") else {0, 1, 4}), (family, kind, ways)


def edge_x(kind, M, layer, seed):
    """The activations of an edge case of `kind`."""
    if kind == "subx":
        return make_x_subnormal(M, layer.K, seed)
    if kind == "overflow":
        return make_x_overflow(M, layer, seed)
    return make_x(M, layer.K, seed, layer.dtype)


def edge_cases(family, kind):
    """[(layer kwargs with the kind's Layer parameters, M, overrides, expected plan fields)].  The fp16-only kinds run the
    fp16 layers; "nonfinite" runs each of them in fp16 and in bf16.  "overflow" and "nonfinite" need three rows: they leave out
    the variants that take at most two (family 0's persistent one-shot kernel).  "overflow" runs the layers at
    K = OVERFLOW_K with scales +-1 / +-2 (the skinny kernel then with 8 waves)."""
    out = []
    for lay, M, ovr, exp in edge_variants(family):
        if kind in ("overflow", "nonfinite") and M < 3:
            continue
        extra = [dict()]
        if kind == "subw":
            extra = [SUBW]
        elif kind == "overflow":
            extra = [dict(OVERFLOW, K=OVERFLOW_K)]
            if family == 5:
                ovr, exp = dict(ovr, waves=8), dict(exp, waves=8)
        elif kind == "nonfinite":
            extra = [dict(dtype=F16), dict(dtype=BF16)]
        for x in extra:
            out.append((dict(lay, **x), M, ovr, exp))
    return out


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def layer_key(kw):
    return tuple(sorted((k, str(v)) for k, v in kw.items()))


def make_layer(kw, seed):
    return Layer(kw["bits"], kw["K"], kw["N"], kw["g"], kw["dtype"], seed, kw["tile_p"], kw["pair"],
                 kw.get("table_div", 1), kw.get("scale_exp", (-3, 1)))

