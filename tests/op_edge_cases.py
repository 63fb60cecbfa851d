"""Hostile operands for the MoE and training ops: the constructions and the by-rule expectations.

A test helper module (not a conftest).  `tests/test_op_edge_cases.py` checks every construction and every rule on the CPU,
`tests/test_grouped_edges_gpu.py`, `tests/test_block_edges_gpu.py` (the block variants) and `tests/test_grad_edges_gpu.py`
run them against the kernels.  Each builder asserts the premises of its case while it builds it, so a premise holds
wherever the case is used.

Range edges (fp16): an exact case outside the exact tests' operating region - subnormal weights (`Layer(**SUBW)`),
a subnormal row operand (j 2^-20), a result that overflows in both directions - still has ONE allowed answer, round_T of
the fp64 result, infinities included (tests/exact_cases.py, "the fp16 range edges").

Non-finite operands: the expectation follows by rule from the op's documented formula (include/flute_amd.h) and the
bits of the same launch on the unpoisoned operands ("clean").  A rule never multiplies non-finite data; the `*_ieee`
functions evaluate the formula in fp64 torch on the poisoned data, element by element (no BLAS call ever sees a
non-finite operand: a library may skip zero operands), and the CPU test asserts that rule and evaluation agree.
"""
import types

import torch

from tests import exact_cases as XC
from tests import scale_grad_ref as SR
from tests import table_grad_ref as TR

F16, BF16 = torch.float16, torch.bfloat16
NAN, INF = float("nan"), float("inf")

CONFIGS = ((4, 32), (3, 32), (2, 32), (4, 64), (2, 64))      # (bits, TileP)
G_CASES = tuple((b, p, 64) for b, p in CONFIGS) + ((4, 32, 32),)
K_EDGE = 320                      # five 64-groups: a ragged last k block of the grouped forward, a half last slab of the gradient
FWD_COUNTS = [0, 1, 15, 17, 0, 33, 5]       # seams inside a 16-row tile and a 32-row pass, an empty first and middle expert
ROW_BLOCK = 128                   # include/flute_amd.h FLUTE_GROUPED_INPUT_GRAD_ROW_BLOCK
GRAD_OVERFLOW_N, GRAD_OVERFLOW_K = 4096, 128
SG_COUNTS = [0, 31, 33, 0, 64, 5]
SG_M = 259                        # 9 steps of 32 rows: the dense scale gradient may split them in two (kSgMinSteps = 4)
WEIGHTS = (0.5, 1.0, 2.0, -1.0, -0.25, 0.0)
# The block forms (qgemm_grouped_blocks.h, qgemm_grouped_input_grad_blocks.h): 4 and 2 bits, 128-row blocks per expert.  Every
# builder below takes `block`: the same construction at shapes the block forms serve - grad_counts() for the forward too, N a
# multiple of 256, K = 8 groups in the forward, K = 512 (two k blocks of 256) in the gradient.
BLOCK_CONFIGS = tuple(c for c in CONFIGS if c[0] != 3)
BLOCK_G_CASES = tuple(c for c in G_CASES if c[0] != 3)
BLOCK_K_GRAD = 512
BLOCK_OVERFLOW_K_GRAD = 256


def grad_counts(rb=ROW_BLOCK):
    """grouped_cases.counts_of"""
    return [0, 1, rb - 1, rb, rb + 1, 0, 2 * rb + 3, 5]


def offsets_list(counts):
    off = [0]
    for n in counts:
        off.append(off[-1] + n)
    return off


def expert_of_row(counts, r):
    off = offsets_list(counts)
    return next(e for e in range(len(counts)) if off[e] <= r < off[e + 1])


_STACKS = {}


def stack(bits, tile_p, g, dtype, K, N, E, seed0, **kw):
    """E exact layers, seeds seed0 ..; built once per module run: cases that share a stack get the same list object."""
    key = (bits, tile_p, g, dtype, K, N, E, seed0, tuple(sorted(kw.items())))
    if key not in _STACKS:
        _STACKS[key] = [XC.Layer(bits, K, N, g, dtype, seed=seed0 + e, tile_p=tile_p, **kw) for e in range(E)]
    return _STACKS[key]


def searched_stack(bits, tile_p, g, dtype, K, N, counts, seed0, need, fits, **kw):
    """A stack in which `fits(layer)` holds for every expert with at least `need` rows.  A random table of few or small entries
    (2 bits: four of them) may miss what a premise asks of it - too few subnormal products, sums that do not reach 65520:
    such an expert takes the next seed, seed + 1000, + 2000, ...; the premise itself is asserted where the case is built."""
    key = ("searched", bits, tile_p, g, dtype, K, N, tuple(counts), seed0, need, tuple(sorted(kw.items())))
    if key in _STACKS:
        return _STACKS[key]
    out = _STACKS[key] = []
    for e, n in enumerate(counts):
        for j in range(50):
            lay = XC.Layer(bits, K, N, g, dtype, seed=seed0 + e + 1000 * j, tile_p=tile_p, **kw)
            if n < need or fits(lay):
                break
        else:
            raise AssertionError("no seed gives a fitting layer")
        out.append(lay)
    return out


def overflow_stack(bits, tile_p, g, dtype, K, N, counts, seed0, need, reaches):
    """Scales +-1 / +-2; `reaches`: 4 sum |w| passes 65520 somewhere and some a sum |w| lies in [2^15, 65520)."""
    return searched_stack(bits, tile_p, g, dtype, K, N, counts, seed0, need, reaches, **XC.OVERFLOW)


def mostly_subnormal(lay):
    return float(XC.is_subnormal_f16(lay.w_exact()).double().mean()) >= 0.5


def _reaches(c):
    return bool(4 * float(c.max()) >= 65520.0 and any(((a * c >= 2.0 ** 15) & (a * c < 65520.0)).any() for a in (3, 2, 1)))


def as_stack(lay):
    """One layer as a stack of one expert (the same list for the same layer object)."""
    return _STACKS.setdefault(("single", id(lay)), [lay])


def draw_weights(n, seed, choice=WEIGHTS):
    c = torch.tensor(choice)
    w = c[torch.randint(0, len(c), (n,), generator=torch.Generator().manual_seed(seed))]
    return w.float()


def sign_class(s, dtype):
    """A row of signs as the values the rule names: +-inf, NaN where the sign is zero."""
    return torch.where(s == 0, NAN, torch.where(s > 0, INF, -INF)).to(dtype)


def has_both_infs(R, dtype):
    Rt = R.to(dtype).double()
    return bool((Rt == INF).any() and (Rt == -INF).any())


def block_n(bits, tile_p):
    return max(256, XC.cols_per_block(bits, tile_p))


def largest(counts):
    return counts.index(max(counts))


def forward_blocks_eligible(bits, g, K, N):
    """include/flute_amd.h, "The block form serves" (the byte limits are far away)."""
    return bits in (4, 2) and K % g == 0 and (K // g) % 8 == 0 and N % 256 == 0


def grad_blocks_eligible(bits, K):
    return bits in (4, 2) and K % 256 == 0


def _forward_shape(bits, tile_p, g, block, overflow=False):
    """(counts, K, N) of a forward case."""
    if block:
        counts, K, N = grad_counts(), (XC.OVERFLOW_K if overflow else 8 * g), block_n(bits, tile_p)
        assert forward_blocks_eligible(bits, g, K, N)
        return counts, K, N
    return FWD_COUNTS, (XC.OVERFLOW_K if overflow else K_EDGE), 3 * XC.cols_per_block(bits, tile_p)


def _grad_shape(bits, tile_p, block, overflow=False):
    """(K, N) of a gradient case."""
    if block:
        K, N = (BLOCK_OVERFLOW_K_GRAD, GRAD_OVERFLOW_N) if overflow else (BLOCK_K_GRAD, block_n(bits, tile_p))
        assert grad_blocks_eligible(bits, K)
        return K, N
    return (GRAD_OVERFLOW_K, GRAD_OVERFLOW_N) if overflow else (K_EDGE, 3 * XC.cols_per_block(bits, tile_p))


def _block_key(block):
    """What a block variant adds to a seed's key: nothing for the cases that existed before it."""
    return ("blocks",) if block else ()


def _small_premise(kind, x, lay, A):
    """premise_edge's exactness conditions for an expert with fewer than three rows (no room for the edge rows)."""
    if kind == "subw":
        XC._exact_in_fp32(x.double(), lay, A, 1.0, 2.0 ** -6)
    elif kind == "subx":
        XC._exact_in_fp32(x.double(), lay, A, 2.0 ** -20, 1.0)
    else:
        assert float(A.max()) < XC.EXACT_SUM_LIMIT


# ---------------------------------------------------------------------------
# the grouped forward: Plain, Weighted, Glu
# ---------------------------------------------------------------------------

def forward_exact(layers, counts, X, rows=None, flush_w=False, flush_x=False):
    """(R, A) [rows, N] in fp64: per expert X[r] @ W_exact and |X[r]| @ |W_exact| (row r of X, or X[rows[r]])."""
    off = offsets_list(counts)
    R = torch.zeros(off[-1], layers[0].N, dtype=torch.float64)
    A = torch.zeros_like(R)
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 > r0:
            x = X[r0:r1] if rows is None else X[rows[r0:r1]]
            R[r0:r1], A[r0:r1] = XC.exact_product(x, lay, abs_too=True, flush_w=flush_w, flush_x=flush_x)
    return R, A


def forward_range_case(op, kind, bits, tile_p, g=64, block=False):
    """Plain / Weighted at a range edge: the expectation c.R is fp64, the allowed answer round_T(c.R) by value."""
    dtype = F16
    counts, K, N = _forward_shape(bits, tile_p, g, block, kind == "overflow")
    seed = XC.seed_of("forward", kind, bits, tile_p, g, *_block_key(block))
    if kind == "overflow":
        layers = overflow_stack(bits, tile_p, g, dtype, K, N, counts, seed, 3,
                                lambda lay: _reaches(lay.w_exact(0, min(N, 256)).abs().sum(0)))
    elif kind == "subw":
        layers = searched_stack(bits, tile_p, g, dtype, K, N, counts, seed, 1, mostly_subnormal, **XC.SUBW)
    else:
        layers = stack(bits, tile_p, g, dtype, K, N, len(counts), seed)
    off = offsets_list(counts)
    T = off[-1]
    X = XC.make_x_subnormal(T, K, seed + 1) if kind == "subx" else XC.make_x(T, K, seed + 1, dtype)
    if kind == "overflow":
        for e, n in enumerate(counts):
            if n >= 3:
                X[off[e]:off[e + 1]] = XC.make_x_overflow(n, layers[e], seed + 2 + e)
    R, A = forward_exact(layers, counts, X)
    for e, n in enumerate(counts):
        sl = slice(off[e], off[e + 1])
        if n >= 3:
            XC.premise_edge(kind, X[sl], layers[e], R[sl], A[sl])
        elif n:
            _small_premise(kind, X[sl], layers[e], A[sl])
    rw = None
    if op == "weighted":
        rw = draw_weights(T, seed + 3)                 # powers of two and zero: rw times an exact fp32 sum is exact
        big = off[largest(counts)]
        rw[big:big + 4] = torch.tensor([1.0, 1.0, 1.0, 0.0])  # the largest expert's edge rows keep their size; a zero
        R = R * rw.double()[:, None]
    if kind == "overflow":
        assert has_both_infs(R, dtype) and (torch.isfinite(R.to(dtype)) & (R.abs() >= 2.0 ** 15)).any()
    return types.SimpleNamespace(op=op, kind=kind, bits=bits, tile_p=tile_p, g=g, dtype=dtype, K=K, N=N, counts=counts,
                                 layers=layers, X=X, rw=rw, R=R, rows=None, block=block)


def weighted_pushed_case(bits, tile_p, g=64, block=False):
    """The unweighted result is finite; a power-of-two row weight alone pushes row a past 65520 (+inf), and the same
    weight negated on a copy of the row, b, gives -inf at the same place."""
    dtype = F16
    counts, K, N = _forward_shape(bits, tile_p, g, block)
    seed = XC.seed_of("pushed", bits, tile_p, g, *_block_key(block))
    layers = stack(bits, tile_p, g, dtype, K, N, len(counts), seed)
    off = offsets_list(counts)
    T = off[-1]
    X = XC.make_x(T, K, seed + 1, dtype)
    a, b = off[largest(counts)] + 1, off[largest(counts)] + 2
    X[b] = X[a]
    R, A = forward_exact(layers, counts, X)
    for e, n in enumerate(counts):
        if n:
            sl = slice(off[e], off[e + 1])
            XC.premise(X[sl], layers[e], R[sl], A[sl], witness=False)        # finite in T, sum |x w| < 2^21
    m = float(R[a].abs().max())
    assert 0 < m <= XC.FP16_MAX
    w = 1.0
    while w * m < 65520.0:
        w *= 2
    assert 2 <= w <= 2.0 ** 16                            # a power of two times an exact fp32 sum: exact, far from fp32's range
    rw = torch.ones(T)
    rw[a], rw[b] = w, -w
    R = R * rw.double()[:, None]
    Rt = R.to(dtype).double()
    assert (Rt[a] == INF).any() and torch.equal(Rt[b], -Rt[a]) and torch.isfinite(Rt[a]).any()
    pos = Rt[a] == INF
    assert bool((Rt[b][pos] == -INF).all())
    return types.SimpleNamespace(op="weighted", kind="pushed", bits=bits, tile_p=tile_p, g=g, dtype=dtype, K=K, N=N,
                                 counts=counts, layers=layers, X=X, rw=rw, R=R, rows=None, a=a, b=b, block=block)


# --- Glu saturation -----------------------------------------------------------------------------------------------

GLU_HI, GLU_LO, GLU_MID_LO = 18.0, -90.0, -88.0
GLU_SIGN_KS = (160, 128, 96, 64, 32)      # how many k the sign rows cover: the first that meets every premise is taken


def glu_exact(gate, up, counts, X, rows=None):
    (G, Ag), (U, Au) = forward_exact(gate, counts, X, rows), forward_exact(up, counts, X, rows)
    assert float(max(Ag.max(), Au.max())) < XC.EXACT_SUM_LIMIT          # g and u are exact fp32 sums in any order
    return G, U


def glu_saturation_case(bits, tile_p, g, dtype, use_rows):
    """Integer activations at p = 0.  In every expert with two rows or more, row 0 = sign(w_gate[:, n0]) over the first
    sign_k k and row 1 = -row 0: |g| of several hundred in column n0, ordinary values elsewhere; the other rows are
    integers in [-1, 1].  The classes per element (c.hi, c.lo, c.mid) and their premises are asserted here; sign_k is the
    first of GLU_SIGN_KS with which they hold (the tables differ in size: a stack of large entries needs fewer k to reach
    several hundred, and with more its products g u would leave the range in which they are exact in fp32)."""
    for sign_k in GLU_SIGN_KS:
        try:
            return _glu_saturation_case(bits, tile_p, g, dtype, use_rows, sign_k)
        except AssertionError as err:
            last = err
    raise AssertionError("no sign_k meets the premises; change the seed") from last


def _glu_saturation_case(bits, tile_p, g, dtype, use_rows, sign_k):
    counts, K = FWD_COUNTS, K_EDGE
    N = 3 * XC.cols_per_block(bits, tile_p)
    seed = XC.seed_of("glu sat", bits, tile_p, g, dtype)
    E = len(counts)
    gate = stack(bits, tile_p, g, dtype, K, N, E, seed)
    up = stack(bits, tile_p, g, dtype, K, N, E, seed + 500)
    off = offsets_list(counts)
    R = off[-1]
    Xs = torch.randint(-1, 2, (R, K), generator=torch.Generator().manual_seed(seed + 1)).double()
    for e, n in enumerate(counts):
        if n >= 2:
            w = gate[e].w_exact(0, min(N, 256))
            n0 = int(w[:sign_k].abs().sum(0).argmax())
            Xs[off[e]] = 0
            Xs[off[e], :sign_k] = torch.where(w[:sign_k, n0] < 0, -1.0, 1.0)
            Xs[off[e] + 1] = -Xs[off[e]]
    rows = None
    X = Xs.to(dtype)
    if use_rows:                                           # Xsrc[rows[r]] = the sorted row r
        rows = torch.randperm(R, generator=torch.Generator().manual_seed(seed + 2))
        X = torch.empty_like(X)
        X[rows] = Xs.to(dtype)
    G, U = glu_exact(gate, up, counts, X, rows)
    assert float(G.abs().max()) >= 200, float(G.abs().max())
    hi, lo = G >= GLU_HI, G <= GLU_LO
    mid = (G >= GLU_MID_LO) & (G < GLU_HI)
    out = ~(hi | lo | mid)
    assert float(out.double().mean()) <= 0.02, float(out.double().mean())
    assert int(hi.sum()) >= 64 and int(lo.sum()) >= 64 and int(mid.sum()) >= 64
    assert int((G > 89).sum()) >= 64                       # (where exp(g) overflows fp32)
    P = G * U
    assert torch.equal(P * 64, (P * 64).round()) and float(P[hi].abs().max()) < 2.0 ** 18, float(P[hi].abs().max())
    Eref = G / (1 + torch.exp(-G)) * U                     # the documented formula in fp64 (mid range)
    if dtype == F16:
        assert float(Eref[mid].abs().max()) < XC.FP16_MAX / 2
        assert torch.isinf(P.to(F16)[hi]).any(), "some round_T(g u) are +-inf: a store that saturates at 65504 fails"
    return types.SimpleNamespace(op="glu", kind="saturation", bits=bits, tile_p=tile_p, g=g, dtype=dtype, K=K, N=N,
                                 counts=counts, layers=gate, up=up, X=X, rows=rows, G=G, U=U, hi=hi, lo=lo, mid=mid,
                                 P=P, Eref=Eref, rw=None, sign_k=sign_k)


# --- non-finite rows ----------------------------------------------------------------------------------------------------

def rowwise_expected(clean, poisons):
    """The rule of the row-wise ops.  poisons: (row, None) - the row is all NaN - or (row, signs [columns]) - the row is
    +-inf by the sign and NaN where it is zero.  Every other row has the bits of `clean`."""
    exp = clean.clone().cpu()
    for r, s in poisons:
        exp[r] = NAN if s is None else sign_class(s, exp.dtype)
    return exp


def forward_inf_sign(c, r, k):
    """The signs that decide the Inf row r (a sorted row) whose +Inf sits at column k of its activation row."""
    e = expert_of_row(c.counts, r)
    s = torch.sign(c.layers[e].w_exact()[k])
    if c.op == "weighted":
        s = s * float(torch.sign(c.rw[r]))
    if c.op == "glu":       # g = +inf: silu = +inf, times u = +-inf; g = -inf: -inf / inf = NaN; a zero weight in either: NaN
        su = torch.sign(c.up[e].w_exact()[k])
        s = torch.where(s > 0, su, torch.zeros_like(s))
    return s


def block_places(first, last, later):
    """[(name, NaN row, Inf row, (column of the NaN, column of the Inf), the pair form's second stack)] over grad_counts(): the
    last valid row of a ragged 128-row block against the first row of the next expert, which follows it directly in memory;
    across the empty expert; the second and the third row block of the largest expert; the first seam once more the other way
    round - an Inf in the last valid row is what a tail masked by a multiplication would turn into NaN."""
    return (("seam 127|128, first chunk", 127, 128, first, False), ("seam 384|385, last chunk", 384, 385, last, True),
            ("later row blocks", 385 + 128 + 5, 642, later, False),
            ("seam 127|128, Inf in the last row", 128, 127, first, False))


BLOCK_ZERO_WEIGHT_ROW = 400       # a finite row of the largest expert whose row weight is zero
BLOCK_INF_ROW_WEIGHTS = ((128, -2.0), (385, 0.0), (642, 0.5))      # Inf rows: a negative weight, zero (all NaN), a small one


def _block_row_weights(rw):
    for r, w in BLOCK_INF_ROW_WEIGHTS + ((BLOCK_ZERO_WEIGHT_ROW, 0.0),):
        rw[r] = w
    assert float(rw[127]) != 0                               # (the fourth place's Inf row keeps a drawn, non-zero weight)
    return rw


def forward_nonfinite_case(op, bits, tile_p, g, dtype, use_rows=False, block=False):
    """One NaN and one +Inf per launch, on both sides of a seam between two experts that have rows (c.launches); glu
    through `rows`: each poisoned token has two slots in two different experts."""
    assert not (block and (op == "glu" or use_rows)), "the GLU launch has no block form"
    counts, K, N = _forward_shape(bits, tile_p, g, block)
    seed = XC.seed_of("forward nonfinite", op, bits, tile_p, g, dtype, use_rows, *_block_key(block))
    lseed = XC.seed_of("forward nonfinite layers", bits, tile_p, g, dtype, *_block_key(block))      # one stack for every op
    E = len(counts)
    layers = stack(bits, tile_p, g, dtype, K, N, E, lseed)
    up = stack(bits, tile_p, g, dtype, K, N, E, lseed + 500) if op == "glu" else None
    off = offsets_list(counts)
    R = off[-1]
    c = types.SimpleNamespace(op=op, kind="nonfinite", bits=bits, tile_p=tile_p, g=g, dtype=dtype, K=K, N=N, counts=counts,
                              layers=layers, up=up, rows=None, rw=None, block=block)
    first, last = (3, 6), (K - 2, K - 5)                    # (k of the NaN, k of the Inf): an even and an odd k each
    if block:
        assert off[3] == 128 and off[6] == 385 and counts[5] == 0 and counts[6] == 259
        places = tuple(p[:4] for p in block_places(first, last, (K - 2, 6)))
    else:
        assert off[3] == 16 and off[5] == 33 and counts[4] == 0
        # (NaN row, Inf row): the seam 15 | 16 inside a 16-row tile; 32 | 33 across the empty expert; the second row pass of the
        # largest expert (row 33 + 32 at 32 rows a pass, rows 49 .. 64 at 16)
        places = (("seam 15|16, first k-step", 15, 16, first), ("seam 32|33, last group", 32, 33, last),
                  ("second row pass", 65, 50, (K - 2, 6)))
    if op == "weighted":
        rw = draw_weights(R, seed + 3, (0.5, 1.0, 2.0, -1.0))
        if block:
            _block_row_weights(rw)
        else:
            rw[16], rw[33], rw[50], rw[40] = -2.0, 0.0, 0.5, 0.0   # Inf rows: a negative weight, zero (all NaN); a finite row: zero
        c.rw = rw
    scale = 2.0 ** -6 if op == "glu" else 1.0               # glu: pre-activations of moderate size, a finite clean result
    if use_rows:
        Tsrc, t_nan, t_inf = 40, 7, 22
        rows = torch.randint(0, Tsrc, (R,), generator=torch.Generator().manual_seed(seed + 2))
        rows[rows == t_nan] = 0
        rows[rows == t_inf] = 1
        rows[15], rows[33] = t_nan, t_nan                   # the last row of expert 2, the first row of expert 5
        rows[16], rows[65] = t_inf, t_inf                   # the first row of expert 3, the second row pass of expert 5
        c.rows = rows
        c.X = (XC.make_x(Tsrc, K, seed + 1, dtype).double() * scale).to(dtype)
        c.launches = []
        for name, (k_nan, k_inf) in (("first k-step", first), ("last group", last)):
            poisons = [(r, None) for r in (15, 33)] + [(r, forward_inf_sign(c, r, k_inf)) for r in (16, 65)]
            c.launches.append(types.SimpleNamespace(name=name, X=XC.poison_x(c.X, t_nan, t_inf, k_nan, k_inf), poisons=poisons))
    else:
        c.X = (XC.make_x(R, K, seed + 1, dtype).double() * scale).to(dtype)
        c.launches = [types.SimpleNamespace(name=name, X=XC.poison_x(c.X, r_nan, r_inf, k_nan, k_inf),
                                            poisons=[(r_nan, None), (r_inf, forward_inf_sign(c, r_inf, k_inf))])
                      for name, r_nan, r_inf, (k_nan, k_inf) in places]
    return c


def _ieee_rows(x, W):
    """x [m, K] @ W [K, N] in fp64 by elementwise products and sums: IEEE arithmetic on whatever x holds."""
    return torch.stack([(xr[:, None] * W).sum(0) for xr in x.double()])


def forward_ieee(c, X):
    """The op's documented formula in fp64 on X (which may hold NaN / Inf), rounded once to T."""
    off = offsets_list(c.counts)
    out = torch.zeros(off[-1], c.N, dtype=torch.float64)
    for e, lay in enumerate(c.layers):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        x = (X[r0:r1] if c.rows is None else X[c.rows[r0:r1]]).double()
        bad = ~torch.isfinite(x).all(dim=1)

        def prod(W):
            P = torch.zeros(r1 - r0, c.N, dtype=torch.float64)
            P[~bad] = x[~bad] @ W
            if bad.any():
                P[bad] = _ieee_rows(x[bad], W)
            return P

        y = prod(lay.w_exact())
        if c.op == "glu":
            y = y / (1 + torch.exp(-y)) * prod(c.up[e].w_exact())
        if c.op == "weighted":
            y = y * c.rw[r0:r1].double()[:, None]
        out[r0:r1] = y
    return out.to(c.dtype)


# ---------------------------------------------------------------------------
# the grouped input gradient: single, pair, row_weight
# ---------------------------------------------------------------------------

def grad_exact(layers, counts, dY, flush_w=False, flush_y=False):
    """(R, A) [rows, K] in fp64: per expert dY[r] @ W_exact^T and |dY[r]| @ |W_exact|^T."""
    off = offsets_list(counts)
    R = torch.zeros(off[-1], layers[0].K, dtype=torch.float64)
    A = torch.zeros_like(R)
    d = dY.double()
    if flush_y:
        d = XC.flush_subnormal_f16(d)
    for e, lay in enumerate(layers):
        r0, r1 = off[e], off[e + 1]
        if r1 > r0:
            W = lay.w_exact()
            if flush_w:
                W = XC.flush_subnormal_f16(W)
            R[r0:r1], A[r0:r1] = d[r0:r1] @ W.T, d[r0:r1].abs() @ W.abs().T
    return R, A


def make_dy_overflow(M, layer, seed):
    """make_x_overflow with the roles of K and N exchanged (the gradient contracts over N): row 0 = 4 sign(w[k0, :]) for
    the k0 with the largest sum_n |w|, row 1 = -row 0, row 2 = a sign(w[k2, :]) with 2^15 <= a sum_n |w[k2]| < 65520."""
    assert M >= 3
    dY = XC.make_x(M, layer.N, seed, layer.dtype, witness=False).double()
    w = layer.w_exact()
    c = w.abs().sum(1)
    sgn = lambda k: torch.where(w[k] < 0, -1.0, 1.0).double()
    dY[0] = 4 * sgn(int(c.argmax()))
    dY[1] = -dY[0]
    for a in (3, 2, 1):
        ok = ((a * c >= 2.0 ** 15) & (a * c < 65520.0)).nonzero()
        if len(ok):
            dY[2] = a * sgn(int(ok[0]))
            break
    else:
        raise AssertionError("no row whose a sum |w| lies in [2^15, 65520)")
    return dY.to(layer.dtype)


def grad_premise(kind, dY, lay, A):
    """premise_edge for dX = dY @ W^T: operands exact in T and every partial sum over N exact in fp32."""
    T = lay.dtype
    d, w = dY.double(), lay.w_exact()
    assert XC._is_T(d, T) and XC._is_T(w, T)
    if kind == "subw":
        assert torch.equal(d, d.round()) and d.abs().max() <= 4
        sub = float(XC.is_subnormal_f16(w).double().mean())
        assert sub >= 0.5, sub
        assert torch.equal(w * 2.0 ** 18, (w * 2.0 ** 18).round()) and float(A.max()) < 2.0 ** -18 * 2.0 ** 24
    elif kind == "subx":
        j = d * 2.0 ** 20
        assert torch.equal(j, j.round()) and j.abs().max() <= 4 and XC.is_subnormal_f16(d).any()
        assert torch.equal(w * 8, (w * 8).round()) and float(A.max()) < 2.0 ** -23 * 2.0 ** 24
    else:
        assert torch.equal(d, d.round()) and d.abs().max() <= 4
        assert torch.equal(w * 8, (w * 8).round()) and w.abs().max() <= 16
        assert float(A.max()) < XC.EXACT_SUM_LIMIT, float(A.max())


def grad_range_case(form, kind, bits, tile_p, g=64, block=False):
    """single / pair / weighted at a range edge; c.R fp64, the allowed answer round_T(c.R) by value."""
    dtype, counts = F16, grad_counts()
    K, N = _grad_shape(bits, tile_p, block, kind == "overflow")
    seed = XC.seed_of("grad", form, kind, bits, tile_p, g, *_block_key(block))
    lseed = XC.seed_of("grad layers", kind, bits, tile_p, g, *_block_key(block))      # one stack for the three forms
    E = len(counts)
    if kind == "overflow":
        layers = overflow_stack(bits, tile_p, g, dtype, K, N, counts, lseed, 5, lambda lay: _reaches(lay.w_exact().abs().sum(1)))
    elif kind == "subw":
        layers = searched_stack(bits, tile_p, g, dtype, K, N, counts, lseed, 1, mostly_subnormal, **XC.SUBW)
    else:
        layers = stack(bits, tile_p, g, dtype, K, N, E, lseed)
    off = offsets_list(counts)
    Rn = off[-1]
    mk = (lambda s: XC.make_x_subnormal(Rn, N, s)) if kind == "subx" else (lambda s: XC.make_x(Rn, N, s, dtype, witness=False))
    dY = mk(seed + 1)
    big = [e for e, n in enumerate(counts) if n >= 5]
    if kind == "overflow":
        for e in big:
            edge = make_dy_overflow(3, layers[e], seed + 2 + e)
            dY[off[e]:off[e] + 3] = edge
            dY[off[e] + 3:off[e] + 5] = edge[:2]
    R, A = grad_exact(layers, counts, dY)
    c = types.SimpleNamespace(form=form, kind=kind, bits=bits, tile_p=tile_p, g=g, dtype=dtype, K=K, N=N, counts=counts,
                              layers=layers, layers2=None, dY=dY, dY2=None, rw=None, block=block, big=big)
    if form == "pair":
        if kind == "overflow":
            # the same stack twice, dY2 = -dY on the two overflowing rows: two finite halves that would each overflow alone
            # add to exactly zero in the one fp32 accumulator; rows 3 and 4 repeat them against dY2 = 0 and do overflow
            c.layers2 = layers
            dY2 = mk(seed + 50)
            for e in big:
                dY2[off[e]:off[e] + 2] = -dY[off[e]:off[e] + 2]
                dY2[off[e] + 2:off[e] + 5] = 0
        else:
            c.layers2 = (searched_stack(bits, tile_p, g, dtype, K, N, counts, lseed + 700, 1, mostly_subnormal, **XC.SUBW)
                         if kind == "subw" else stack(bits, tile_p, g, dtype, K, N, E, lseed + 700))
            dY2 = mk(seed + 50)
        c.dY2 = dY2
        R2, A2 = grad_exact(c.layers2, counts, dY2)
        if kind == "overflow":
            for e in big:
                assert has_both_infs(R[off[e]:off[e] + 2], dtype) and not (R + R2)[off[e]:off[e] + 2].any()
        R, A = R + R2, A + A2
    for e, n in enumerate(counts):
        if n:
            sl = slice(off[e], off[e + 1])
            grad_premise(kind, dY[sl], layers[e], A[sl])
            if form == "pair":
                grad_premise(kind, c.dY2[sl], c.layers2[e], A[sl])
    if form == "weighted":
        c.rw = draw_weights(Rn, seed + 3, (0.25, -0.25, 1.0, -1.0, 2.0, 0.0))
        for e in big:
            c.rw[off[e]:off[e] + 5] = torch.tensor([1.0, 1.0, 1.0, -1.0, -1.0])
        R = R * c.rw.double()[:, None]
    Rt = R.to(dtype).double()
    if kind == "overflow":
        assert has_both_infs(R, dtype) and (torch.isfinite(Rt) & (R.abs() >= 2.0 ** 15)).any()
    elif kind == "subw":
        assert XC.is_subnormal_f16(Rt).any(), "some outputs subnormal"
    assert not torch.isnan(Rt).any()
    c.R = R
    return c


def grad_inf_sign(c, r, n, second=False):
    e = expert_of_row(c.counts, r)
    s = torch.sign((c.layers2 if second else c.layers)[e].w_exact()[:, n])
    return s * float(torch.sign(c.rw[r])) if c.rw is not None else s


def grad_nonfinite_case(form, bits, tile_p, g, dtype, block=False):
    counts = grad_counts()
    K, N = _grad_shape(bits, tile_p, block)
    seed = XC.seed_of("grad nonfinite", form, bits, tile_p, g, dtype, *_block_key(block))
    lseed = XC.seed_of("grad nonfinite layers", bits, tile_p, g, dtype, *_block_key(block))
    E = len(counts)
    off = offsets_list(counts)
    Rn = off[-1]
    assert off[3] == 128 and off[6] == 385 and counts[5] == 0 and counts[6] == 259
    c = types.SimpleNamespace(form=form, kind="nonfinite", bits=bits, tile_p=tile_p, g=g, dtype=dtype, K=K, N=N,
                              counts=counts, layers=stack(bits, tile_p, g, dtype, K, N, E, lseed), layers2=None,
                              dY=XC.make_x(Rn, N, seed + 1, dtype, witness=False), dY2=None, rw=None, block=block)
    if form == "pair":
        c.layers2 = stack(bits, tile_p, g, dtype, K, N, E, lseed + 700)
        c.dY2 = XC.make_x(Rn, N, seed + 50, dtype, witness=False)
    if form == "weighted":
        c.rw = _block_row_weights(draw_weights(Rn, seed + 3, (0.25, -0.25, 1.0, -1.0, 2.0)))
    first, last = (3, 6), (N - 2, N - 5)                    # the first and the last 64-column chunk of N
    # (NaN row, Inf row): the seam 127 | 128 inside a row block; 384 | 385 across the empty expert; the second and the third
    # row block of the largest expert; the block variant adds the first seam the other way round
    places = block_places(first, last, (N - 2, 6))
    c.launches = []
    for name, r_nan, r_inf, (n_nan, n_inf), second in places if block else places[:3]:
        second = second and form == "pair"
        dY, dY2 = c.dY, c.dY2
        if second:
            dY2 = XC.poison_x(c.dY2, r_nan, r_inf, n_nan, n_inf)
        else:
            dY = XC.poison_x(c.dY, r_nan, r_inf, n_nan, n_inf)
        c.launches.append(types.SimpleNamespace(name=name, dY=dY, dY2=dY2,
                                                poisons=[(r_nan, None), (r_inf, grad_inf_sign(c, r_inf, n_inf, second))]))
    return c


def grad_ieee(c, dY, dY2):
    off = offsets_list(c.counts)
    out = torch.zeros(off[-1], c.K, dtype=torch.float64)
    for e in range(len(c.counts)):
        r0, r1 = off[e], off[e + 1]
        if r1 == r0:
            continue
        y = torch.zeros(r1 - r0, c.K, dtype=torch.float64)
        for d, lays in ((dY, c.layers), (dY2, c.layers2)):
            if d is None:
                continue
            x = d[r0:r1].double()
            bad = ~torch.isfinite(x).all(dim=1)
            W = lays[e].w_exact().T.contiguous()
            P = torch.zeros_like(y)
            P[~bad] = x[~bad] @ W
            if bad.any():
                P[bad] = _ieee_rows(x[bad], W)
            y = y + P
        if c.rw is not None:
            y = y * c.rw[r0:r1].double()[:, None]
        out[r0:r1] = y
    return out.to(c.dtype)


# ---------------------------------------------------------------------------
# dequantize
# ---------------------------------------------------------------------------

DEQ_OVERFLOW = dict(scale_exp=(10, 15))           # table entries +-8 meet scales +-2^13 and above: 65536 rounds to +-inf in fp16


def dequant_case(kind, bits, tile_p):
    """round_T(lut * s) [N, K] bit for bit, subnormals kept ("subw") and +-inf where due ("overflow")."""
    K, N = K_EDGE, XC.cols_per_block(bits, tile_p)
    kw = XC.SUBW if kind == "subw" else DEQ_OVERFLOW
    lay = XC.Layer(bits, K, N, 64, F16, XC.seed_of("dequant", kind, bits, tile_p), tile_p=tile_p, **kw)
    w = lay.w_exact()
    want = w.T.contiguous().to(F16)
    if kind == "subw":
        assert torch.equal(want.double(), w.T) and float(XC.is_subnormal_f16(w).double().mean()) >= 0.5
    else:
        assert has_both_infs(w, F16) and torch.isfinite(want).any() and float(w.abs().max()) >= 65520.0
        assert torch.equal(want[torch.isfinite(want)].double(), w.T[torch.isfinite(want)])
    return types.SimpleNamespace(kind=kind, lay=lay, want=want)


# ---------------------------------------------------------------------------
# the M-reducing gradients: scale gradient (dense, split, grouped, row_weight), table gradient
# ---------------------------------------------------------------------------

SG_CASES = ((4, 64), (3, 64), (2, 64), (4, 32))            # (bits, g); TileP 32


def sg_shape(bits):
    return (320 if bits == 4 else 448), XC.cols_per_block(bits, 32)


def sg_splits(M, N, K, g, num_sms, scratch_bytes):
    """param_grad.hip's split of M (include/flute_amd.h: it follows from M, N, K, num_sms and scratch_bytes alone)."""
    blocks = (N // 128) * -(-K // 256)
    steps = -(-M // 32)
    target = 2 * (num_sms if num_sms >= 1 else 256)
    splits = min(-(-target // blocks), steps // 4, scratch_bytes // (N * (K // g) * 4), 1024)
    if splits < 2:
        return 1, steps
    sps = -(-steps // splits)
    return -(-steps // sps), sps


def lut(lay):
    return SR.lut_of_codes(lay.W, lay.pairs, lay.bits)


def sg_rows(kind, M, lay, seed, amp=4):
    """(dY [M, N], X [M, K]) of one expert / one dense launch and the fp64 reference, premises asserted.  amp: the size of
    the integer operand that meets the subnormal one (the j of j 2^-20 stay in [-4, 4])."""
    K, N, g, T = lay.K, lay.N, lay.g, lay.dtype
    L = lut(lay)
    assert torch.equal(L, L.round()) and L.abs().max() <= 8
    ints = lambda m, n, amp, s: torch.randint(-amp, amp + 1, (m, n), generator=torch.Generator().manual_seed(s)).double()
    assert amp == 4 or kind in ("subdy", "subx")
    dY, X = ints(M, N, amp if kind == "subx" else 4, seed), ints(M, K, amp if kind == "subdy" else 4, seed + 1)
    if kind == "subdy":
        dY = dY * 2.0 ** -20
    elif kind == "subx":
        X = X * 2.0 ** -20
    elif kind == "overflow":
        n0 = int(L[:2 * g].abs().sum(0).argmax())
        s = torch.where(L[:, n0] < 0, -1.0, 1.0).double()
        X[:, :g] = 4 * s[:g]
        X[:, g:2 * g] = -4 * s[g:2 * g]
        dY[:, n0] = 4
    dY, X = dY.to(T), X.to(T)
    R = SR.scale_grad(dY, X, L, g)
    A = SR.scale_grad(dY, X, L, g, absolute=True)
    if kind == "overflow":
        assert float(A.max()) < 2.0 ** 24, "every partial sum an integer below 2^24"
    else:
        assert XC.is_subnormal_f16((dY if kind == "subdy" else X).double()).any()
        assert float(A.max()) < 2.0 ** 4, "every partial sum a multiple of 2^-20 below 2^4"
    return dY, X, R


def sg_dense_case(kind, bits, g, tag="sg", amp=4):
    K, N = sg_shape(bits)
    lay = XC.Layer(bits, K, N, g, F16, XC.seed_of(tag, kind, bits, g), tile_p=32)
    dY, X, R = sg_rows(kind, SG_M, lay, lay.seed + 1, amp)
    Rt = R.to(F16).double()
    if kind == "overflow":
        row = ((Rt == INF).any(1) & (Rt == -INF).any(1) & torch.isfinite(Rt).any(1))
        assert row.any(), "+inf, -inf and finite neighbours in one row of dS"
    else:
        assert XC.is_subnormal_f16(Rt).any(), "some round_T(dS) subnormal"
    assert not torch.isnan(Rt).any()
    return types.SimpleNamespace(kind=kind, bits=bits, g=g, lay=lay, dY=dY, X=X, R=R, M=SG_M)


def sg_grouped_case(kind, bits, g, tag="sg grouped", amp=4):
    counts = SG_COUNTS
    K, N = sg_shape(bits)
    seed = XC.seed_of(tag, kind, bits, g)
    layers = stack(bits, 32, g, F16, K, N, len(counts), seed)
    off = offsets_list(counts)
    dY, X = torch.zeros(off[-1], N, dtype=F16), torch.zeros(off[-1], K, dtype=F16)
    R = torch.zeros(len(counts), N, K // g, dtype=torch.float64)
    for e, n in enumerate(counts):
        if n:
            dY[off[e]:off[e + 1]], X[off[e]:off[e + 1]], R[e] = sg_rows(kind, n, layers[e], seed + 100 + e, amp)
    Rt = R.to(F16).double()
    assert has_both_infs(R, F16) if kind == "overflow" else XC.is_subnormal_f16(Rt).any()
    return types.SimpleNamespace(kind=kind, bits=bits, g=g, layers=layers, counts=counts, dY=dY, X=X, R=R)


def sg_row_weight_case(bits, g):
    """row_weight as powers of two: round_T(rw dY) is subnormal on some rows and overflows on one."""
    c = sg_grouped_case("subx", bits, g)
    off = offsets_list(c.counts)
    Rn = off[-1]
    rw = draw_weights(Rn, c.layers[0].seed + 9, (1.0, 0.5, -2.0, 2.0 ** -20, 2.0 ** -22))
    r_big = off[4] + 7
    rw[r_big] = 2.0 ** 15
    c.X = XC.make_x(Rn, c.X.shape[1], c.layers[0].seed + 10, F16, witness=False)
    pre = (c.dY.float() * rw[:, None]).to(F16)              # the product in fp32, one round-to-nearest-even to T
    assert torch.isinf(pre[r_big]).any() and XC.is_subnormal_f16(pre.double()).any()
    assert int(torch.isinf(pre).any(1).sum()) == 1
    c.rw, c.pre, c.r_big, c.R = rw, pre, r_big, None
    return c


def reduce_class(npos, nneg, nnan):
    """What a sum of finite addends, npos addends of +inf, nneg of -inf and nnan NaNs is: 0 finite, +-1 +-inf, 2 NaN."""
    out = torch.zeros_like(npos)
    out[npos > 0] = 1
    out[nneg > 0] = -1
    out[(nnan > 0) | ((npos > 0) & (nneg > 0))] = 2
    return out


def apply_class(clean, cls):
    exp = clean.clone().cpu()
    exp[cls == 1], exp[cls == -1], exp[cls == 2] = INF, -INF, NAN
    return exp


def poison_sites(t):
    """[(row, column, is NaN)] of the non-finite entries of t."""
    idx = (~torch.isfinite(t)).nonzero().tolist()
    return [(r, col, bool(torch.isnan(t[r, col]))) for r, col in idx]


def scale_grad_expected(clean, dY, X, L, g):
    """The rule of the scale gradient for one expert's rows (dY [m, N], X [m, K], each with at most a few non-finite
    entries, never in the same row): a NaN at X[r, k0] makes dS[:, group(k0)] NaN; a NaN at dY[r, n0] makes dS[n0, :] NaN;
    an Inf at X[r, k0] gives in dS[n, group(k0)] +-inf by sign(dY[r, n]) sign(L[k0, n]), NaN where either is zero; an Inf at
    dY[r, n1] gives in dS[n1, j] +-inf by the one sign of X[r, k] L[k, n1] over the group, NaN where the group holds a
    zero or both signs.  Everything else has the bits of `clean`."""
    N, G = clean.shape
    npos, nneg, nnan = (torch.zeros(N, G, dtype=torch.long) for _ in range(3))
    dYd, Xd, L = dY.double(), X.double(), L.double()
    for r, k0, is_nan in poison_sites(X):
        j = k0 // g
        if is_nan:
            nnan[:, j] += 1
        else:
            s = torch.sign(dYd[r]) * torch.sign(L[k0]) * float(torch.sign(Xd[r, k0]))
            npos[:, j] += s > 0
            nneg[:, j] += s < 0
            nnan[:, j] += s == 0
    for r, n0, is_nan in poison_sites(dY):
        if is_nan:
            nnan[n0] += 1
        else:
            s = (torch.sign(Xd[r]) * torch.sign(L[:, n0]) * float(torch.sign(dYd[r, n0]))).reshape(G, g)
            npos[n0] += (s > 0).sum(1)
            nneg[n0] += (s < 0).sum(1)
            nnan[n0] += (s == 0).sum(1)
    return apply_class(clean, reduce_class(npos, nneg, nnan))


def _ieee_gram(A, B):
    """A^T B [a, b] in fp64 over the rows, the rows that hold a non-finite entry as elementwise outer products."""
    A, B = A.double(), B.double()
    bad = ~(torch.isfinite(A).all(1) & torch.isfinite(B).all(1))
    out = A[~bad].T @ B[~bad]
    for r in bad.nonzero().reshape(-1).tolist():
        out = out + A[r][:, None] * B[r][None, :]
    return out


def scale_grad_ieee(dY, X, L, g):
    """sum_m sum_{k in group} dY[m, n] X[m, k] L[k, n] in fp64, IEEE arithmetic on whatever dY and X hold: [N, K / g]."""
    Gm = _ieee_gram(dY, X)                                  # [N, K]
    N, K = Gm.shape
    return (Gm * L.double().T).reshape(N, K // g, g).sum(-1)


def table_grad_expected(clean, dY, X, codes, S, bits, g):
    """The rule of the table gradient dT2 [4^b, 2]: exactly the bins (pair index, half k & 1) that a non-finite
    G[k, n] = sum_m X[m, k] dY[m, n] feeds are non-finite, each by the signs of its addends S[n, group(k)] G[k, n]; a bin
    fed by a NaN, a zero times Inf or both signs is NaN.  Every other bin has the bits of `clean`."""
    idx = TR.pair_index(codes, bits)                        # [K / 2, N]
    nb = 4 ** bits
    cnt = [torch.zeros(nb, 2, dtype=torch.long) for _ in range(3)]      # +inf, -inf, NaN addends
    dYd, Xd, Sd = dY.double(), X.double(), S.double()

    def feed(bins, half, s, all_nan):
        none, every = torch.zeros_like(s, dtype=torch.bool), torch.ones_like(s, dtype=torch.bool)
        for i, m in enumerate((none, none, every) if all_nan else (s > 0, s < 0, s == 0)):
            cnt[i][:, half].index_add_(0, bins, m.long())

    for r, k0, is_nan in poison_sites(X):
        s = torch.sign(dYd[r]) * torch.sign(Sd[:, k0 // g]) * (1.0 if is_nan else float(torch.sign(Xd[r, k0])))
        feed(idx[k0 >> 1], k0 & 1, s, is_nan)
    for r, n0, is_nan in poison_sites(dY):
        s = torch.sign(Xd[r]) * torch.sign(Sd[n0].repeat_interleave(g)) * (1.0 if is_nan else float(torch.sign(dYd[r, n0])))
        for half in (0, 1):
            feed(idx[:, n0], half, s[half::2], is_nan)
    return apply_class(clean, reduce_class(*cnt))


def table_grad_ieee(dY, X, codes, S, bits, g):
    V = _ieee_gram(X, dY) * S.double().repeat_interleave(g, dim=1).T
    idx = TR.pair_index(codes, bits).reshape(-1)
    out = torch.zeros(4 ** bits, 2, dtype=torch.float64)
    for e in range(2):
        out[:, e].index_add_(0, idx, V[e::2].reshape(-1))
    return out


def poison(t, sites):
    t = t.clone()
    for r, col, v in sites:
        t[r, col] = v
    return t


def mreduce_launches(r_nan, r_inf, K, N, g, tag=""):
    """[(name, X sites, dY sites)]: once on X (an even k in the first group, an odd k in the last), once on dY."""
    return [("on X" + tag, [(r_nan, 2, NAN), (r_inf, K - 3, INF)], []),
            ("on dY" + tag, [], [(r_nan, 5, NAN), (r_inf, N - 2, INF)])]


def seam_launches(r_last, r_first, K, N, g):
    """The NaN in the last row of one expert and the Inf in the first row of the next, then the other way round: an Inf in a
    last row is what a row masked by `clamp to the last row and multiply by zero` would turn into NaN (inf x 0)."""
    return mreduce_launches(r_last, r_first, K, N, g) + mreduce_launches(r_first, r_last, K, N, g, ", Inf in the last row")


def one_sign_rows(X, rows, L, g, n):
    """X[r, :g] = sign(L[:g, n]) for the rows that take an Inf at dY[r, n]: it meets one sign (or a zero) in group 0."""
    for r in rows:
        X[r, :g] = torch.sign(L[:g, n]).to(X.dtype)


def sg_nonfinite_dense_case(bits, g, dtype):
    """The dense op: c.unsplit poisons rows 31 | 32, the two sides of a 32-row step; c.split rows that fall into different
    splits of M."""
    K, N = sg_shape(bits)
    lay = XC.Layer(bits, K, N, g, dtype, XC.seed_of("sg nonfinite", bits, g, dtype), tile_p=32)
    M = SG_M
    dY = XC.make_x(M, N, lay.seed + 1, dtype, witness=False)
    X = XC.make_x(M, K, lay.seed + 2, dtype, witness=False)
    one_sign_rows(X, (31, 32, M - 1), lut(lay), g, N - 2)
    return types.SimpleNamespace(bits=bits, g=g, dtype=dtype, lay=lay, M=M, dY=dY, X=X,
                                 unsplit=seam_launches(31, 32, K, N, g), tail=mreduce_launches(M - 2, M - 1, K, N, g, ", tail"))


def sg_nonfinite_grouped_case(bits, g, dtype, weighted):
    """NaN in the last row of expert 1, Inf in the first row of expert 2; experts 4 and 5 stay clean, 0 and 3 zeros."""
    return _mreduce_nonfinite_grouped_case("sg grouped nonfinite", bits, g, dtype, weighted)


def tg_nonfinite_grouped_case(bits, g, dtype, weighted):
    """The same seam for flute_qgemm_grouped_table_grad.  Per expert e: dT2[e] = table_grad_expected(clean[e], premultiplied
    dY, X, codes_e, S_e) and the by-product dS[e] = scale_grad_expected(...) on the expert's rows; experts without a
    poisoned row keep the clean launch's bits, experts without rows are zeros."""
    return _mreduce_nonfinite_grouped_case("tg grouped nonfinite", bits, g, dtype, weighted)


def _mreduce_nonfinite_grouped_case(tag, bits, g, dtype, weighted):
    counts = SG_COUNTS
    K, N = sg_shape(bits)
    seed = XC.seed_of(tag, bits, g, dtype, weighted)
    layers = stack(bits, 32, g, dtype, K, N, len(counts), seed)
    off = offsets_list(counts)
    Rn = off[-1]
    dY = XC.make_x(Rn, N, seed + 1, dtype, witness=False)
    X = XC.make_x(Rn, K, seed + 2, dtype, witness=False)
    r_nan, r_inf = off[2] - 1, off[2]
    assert expert_of_row(counts, r_nan) == 1 and expert_of_row(counts, r_inf) == 2 and counts[0] == 0 and counts[3] == 0
    one_sign_rows(X, (r_inf,), lut(layers[2]), g, N - 2)
    one_sign_rows(X, (r_nan,), lut(layers[1]), g, N - 2)
    rw = draw_weights(Rn, seed + 3, (0.5, 1.0, -2.0)) if weighted else None
    return types.SimpleNamespace(bits=bits, g=g, dtype=dtype, layers=layers, counts=counts, dY=dY, X=X, rw=rw,
                                 launches=seam_launches(r_nan, r_inf, K, N, g), touched=(1, 2))


def premultiplied(dY, rw):
    return dY if rw is None else (dY.float() * rw[:, None]).to(dY.dtype)


def tg_nonfinite_case(bits, g, dtype):
    K, N = sg_shape(bits)
    lay = XC.Layer(bits, K, N, g, dtype, XC.seed_of("tg nonfinite", bits, g, dtype), tile_p=32)
    M = 40
    dY = XC.make_x(M, N, lay.seed + 1, dtype, witness=False)
    X = XC.make_x(M, K, lay.seed + 2, dtype, witness=False)
    return types.SimpleNamespace(bits=bits, g=g, dtype=dtype, lay=lay, M=M, dY=dY, X=X,
                                 launches=[("on X", [(31, 2, NAN), (32, K - 4, INF)], []),      # both in half 0 of their pairs: half 1
                                           mreduce_launches(31, 32, K, N, g)[1],           # of every bin stays clean
                                           ("on X, tail", [(M - 2, 2, NAN), (M - 1, K - 4, INF)], []),
                                           mreduce_launches(M - 2, M - 1, K, N, g, ", tail")[1]])
# (a 2- or 3-bit table has 16 or 64 bins: one pair row over N columns reaches all of them, and a column of dY both halves)


TG_RANGE_KINDS = ("subdy", "subx")
TG_AMP = 1        # the integer operand of the table gradient's range cases: a bin sums thousands of (k, n) over all rows


def tg_exact(dY, X, lay):
    """The fp64 table gradient of one layer's rows and the premise that makes it the one allowed answer in fp32: every term
    X dY S is a multiple of 2^-23 (j 2^-20, an integer, a scale 2^e with e >= -3) and every bin's sum of |terms| stays
    below 2^24 of them, so every partial sum - in any order, over any split of the rows or workgroups - is exact in fp32
    and so is the total."""
    assert lay.scale_exp[0] >= -3 and lay.dtype == F16
    sub = dY if XC.is_subnormal_f16(dY.double()).any() else X
    assert XC.is_subnormal_f16(sub.double()).sum() == (sub != 0).sum(), "a kernel that flushes the operand returns zeros"
    R = TR.table_grad(dY, X, lay.W, lay.S, lay.bits, lay.g)
    A = TR.table_grad(dY, X, lay.W, lay.S, lay.bits, lay.g, absolute=True)
    assert float(A.max()) < 2.0 ** -23 * 2.0 ** 24, float(A.max())
    assert torch.equal(R.float().double(), R) and float(R.abs().max()) > 0
    return R


def tg_range_case(kind, bits, g, grouped):
    """dY ("subdy") or X ("subx") is j 2^-20: dT2 in fp32 equals c.RT (fp64) by value; c.R is the by-product dS in fp64,
    round_T by value.  Dense: c.lay and SG_M rows; grouped: c.layers over SG_COUNTS, c.RT [E, 4^b, 2]."""
    assert kind in TG_RANGE_KINDS
    if not grouped:
        c = sg_dense_case(kind, bits, g, "tg", TG_AMP)
        c.RT = tg_exact(c.dY, c.X, c.lay)
        return c
    c = sg_grouped_case(kind, bits, g, "tg grouped", TG_AMP)
    off = offsets_list(c.counts)
    c.RT = torch.zeros(len(c.counts), 4 ** bits, 2, dtype=torch.float64)
    for e, n in enumerate(c.counts):
        if n:
            c.RT[e] = tg_exact(c.dY[off[e]:off[e + 1]], c.X[off[e]:off[e + 1]], c.layers[e])
    return c


def tg_row_weight_case(bits, g):
    """sg_row_weight_case for the table gradient.  c.pre = round_T(rw dY) overflows on row c.r_big alone, in every column
    whose |dY| is 2 or more; c.pre_finite is c.pre with those entries zero - the clean operand of the rules: a bin or a dS
    entry that no infinite entry feeds does not depend on them."""
    c = sg_row_weight_case(bits, g)
    inf = torch.isinf(c.pre)
    c.pre_finite = torch.where(inf, torch.zeros_like(c.pre), c.pre)
    c.e_big = expert_of_row(c.counts, c.r_big)
    assert inf[c.r_big].any() and torch.isfinite(c.pre[c.r_big]).any() and not inf[torch.arange(len(inf)) != c.r_big].any()
    assert XC.is_subnormal_f16(c.pre_finite.double()).any() and not torch.isnan(c.pre).any()
    return c


# ---------------------------------------------------------------------------
# moe_combine
# ---------------------------------------------------------------------------

def combine_case(dtype):
    """T = 6, k = 3, N = 64, E = 4.  Sorted rows Y [18, 64], 16 of them served.  A NaN in one served row; +Inf and -Inf in two
    slots of one token, same column; a NaN in an unserved row (never read).  The clean rows hold 40000 in two slots of one token:
    the fp32 sum is finite, its rounding to fp16 is +inf."""
    T, k, N, E = 6, 3, 64, 4
    P = T * k
    gen = torch.Generator().manual_seed(XC.seed_of("combine", dtype))
    pos = torch.randperm(P, generator=gen).reshape(T, k).int()
    served = 16
    offsets = torch.tensor([0, 5, 5, 11, served], dtype=torch.int32)
    Y = torch.randint(-4, 5, (P, N), generator=gen).to(dtype)
    flat = pos.reshape(-1).tolist()
    token_of = {p: i // k for i, p in enumerate(flat)}
    # a token with three served slots takes the two infinities, another token's served row takes the NaN
    t_inf = next(t for t in range(T) if all(int(p) < served for p in pos[t]))
    p_nan = next(p for p in range(served) if token_of[p] != t_inf)
    Y[int(pos[t_inf, 0]), 50] = Y[int(pos[t_inf, 2]), 50] = 40000.0
    sites = [(p_nan, 9, NAN), (int(pos[t_inf, 0]), 40, INF), (int(pos[t_inf, 2]), 40, -INF), (int(pos[t_inf, 1]), 3, INF),
             (served, 0, NAN), (P - 1, 63, INF)]
    return types.SimpleNamespace(dtype=dtype, T=T, k=k, N=N, E=E, pos=pos, offsets=offsets, served=served, Y=Y,
                                 Yp=poison(Y, sites), t_inf=t_inf, t_nan=token_of[p_nan])


def combine_expected(clean, c):
    exp = clean.clone().cpu()
    exp[c.t_nan, 9] = NAN
    exp[c.t_inf, 40] = NAN                                  # +inf + -inf
    exp[c.t_inf, 3] = INF
    return exp


def combine_ieee(c, Y):
    out = torch.zeros(c.T, c.N, dtype=torch.float64)
    for t in range(c.T):
        for j in range(c.k):
            p = int(c.pos[t, j])
            if 0 <= p < c.served:
                out[t] = out[t] + Y[p].double()
    return out.to(c.dtype)


# ---------------------------------------------------------------------------
# the case lists: the CPU test and the GPU tests walk the same ones
# ---------------------------------------------------------------------------

RANGE_KINDS = ("subw", "subx", "overflow")


def forward_range_params():
    return [(op, kind, b, p, g) for op in ("plain", "weighted") for kind in RANGE_KINDS for b, p, g in G_CASES
            if g == 64 or kind == "subw"]


def pushed_params():
    return list(CONFIGS)


def glu_saturation_params():
    return [(b, p, 64, F16, use_rows) for b, p in CONFIGS for use_rows in (True, False)] + [(4, 32, 32, BF16, True)]


def forward_nonfinite_params():
    out = []
    for b, p, g in G_CASES:
        for dtype in (F16, BF16):
            if g == 32 and dtype == BF16:
                continue
            out += [("plain", b, p, g, dtype, False), ("weighted", b, p, g, dtype, False), ("glu", b, p, g, dtype, True),
                    ("glu", b, p, g, dtype, False)]
    return out


def grad_range_params():
    return [(form, kind, b, p, g) for form in ("single", "pair", "weighted") for kind in RANGE_KINDS for b, p, g in G_CASES
            if g == 64 or (kind == "subw" and form == "single")]


def grad_nonfinite_params():
    return [(form, b, p, g, dtype) for form in ("single", "pair", "weighted") for b, p, g in G_CASES for dtype in (F16, BF16)
            if g == 64 or (dtype == F16 and form == "single")]


def dequant_params():
    return [(kind, b, p) for kind in ("subw", "overflow") for b, p in CONFIGS]


def sg_range_params():
    return [(kind, b, g) for kind in ("subdy", "subx", "overflow") for b, g in SG_CASES]


def sg_nonfinite_params():
    return [(b, g, dtype) for b, g in SG_CASES for dtype in (F16, BF16) if g == 64 or dtype == F16]


def block_forward_range_params():
    return [(op, kind, b, p, g) for op, kind, b, p, g in forward_range_params() if b != 3]


def block_pushed_params():
    return list(BLOCK_CONFIGS)


def block_forward_nonfinite_params():
    return [(op, b, p, g, dtype) for op, b, p, g, dtype, _ in forward_nonfinite_params() if b != 3 and op != "glu"]


def block_grad_range_params():
    return [p for p in grad_range_params() if p[2] != 3]


def block_grad_nonfinite_params():
    return [p for p in grad_nonfinite_params() if p[1] != 3]


def tg_range_params():
    return [(kind, b, g) for kind in TG_RANGE_KINDS for b, g in SG_CASES]


def tg_nonfinite_grouped_params():
    return [(b, g, dtype, weighted) for b, g, dtype in sg_nonfinite_params() for weighted in (False, True)]
