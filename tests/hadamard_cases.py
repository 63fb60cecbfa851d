"""Integer inputs whose Hadamard transform every kernel must return bit for bit, at every h = 2 .. 32768.

A test helper module (not a conftest), importable without a GPU: `tests/test_hadamard_host.py` checks the checkers on the
CPU, `tests/test_hadamard_gpu.py` runs them against the kernels.

Exact by construction
---------------------
The op is out = in.reshape(-1, h) @ (H_h / sqrt(h)), Sylvester order.  On integer input every partial sum of the
butterflies is an integer, and while |S| < 2^24 it is exact in fp32 whatever the order of the stages.  The documented
arithmetic (csrc/hadamard.hip: "all arithmetic is fp32, one rounding at the end"; launch_fwht: scale = 1.0f / sqrtf(h);
fwht.h scale_round: the product rounded to fp32, THEN to T) is therefore a deterministic function of the exact integer
sums S = `fwht_int(x, h)`:

    model(S, h, T) = round_T(fl32(fl32(S) * scale32)),   scale32 = fl32(1 / fl32(sqrt(h)))

and a kernel can be compared with it bit for bit at every h, not only where 1 / sqrt(h) is a power of two.  (The two
roundings are part of the contract: `rounding_witnesses` are the sums at which one rounding would give another value.)

The independent bound
---------------------
Against r = S / sqrt(h) in fp64: scale32 is at most two fp32 roundings away from 1 / sqrt(h), the product adds one more,
then comes one rounding to T, so |y - r| <= (u_T + 3 * 2^-24 + higher order) |r| <= (u_T + 2^-21) |r|; where |r| lies in
T's subnormal range the rounding to T errs by at most half of T's smallest subnormal instead.
"""
import math

import torch

from tests import exact_cases as E

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
SIZES = tuple(1 << k for k in range(1, 16))          # 2 .. 32768
WAVE_MAX = 512                                       # h <= 512: fwht_wave_kernel, fusable; above: fwht_block_kernel
SIG_BITS = {F16: 11, BF16: 8}
INT_MAX = {F16: 2047, BF16: 255}                     # every integer up to here is exact in T (11 / 8 significand bits)
FINITE_MAX = {F16: 65504, BF16: 2 ** 127}            # as integers (bf16: beyond every sum here)
RESULT_CAP = {F16: 65000, BF16: 2 ** 127}            # results of the finite cases stay below this
MIN_NORMAL = {F16: 2.0 ** -14, BF16: 2.0 ** -126}
MIN_SUBNORMAL = {F16: 2.0 ** -24, BF16: 2.0 ** -133}
EXACT_INT_LIMIT = 1 << 24                            # |S| below this: every partial sum exact in fp32
REL_SLACK = 2.0 ** -21                               # the fp32 roundings of the scale and of the product (see above)


def log2_of(h):
    k = h.bit_length() - 1
    assert h >= 1 and 1 << k == h, h
    return k


def _butterflies(v, n):
    """log2(n) butterfly steps over the last dimension (size n) of the 2-D tensor v, low index bit first."""
    rows = v.shape[0]
    for s in range(log2_of(n)):
        w = v.reshape(rows, n >> (s + 1), 2, 1 << s)
        a, b = w[:, :, 0], w[:, :, 1]
        v = torch.stack((a + b, a - b), dim=2).reshape(rows, n)
    return v


def fwht_int(x, h):
    """Unnormalised Sylvester-order transform of x.reshape(-1, h) in int64: log2(h) butterfly steps on the CPU."""
    return _butterflies(x.to(torch.int64).reshape(-1, h), h)


def sylvester(h):
    """H_h in int64 (entries +-1), H[j, i] = (-1)^popcount(i & j); for h <= 1024 only (dense)."""
    assert h <= 1024
    H = torch.ones(1, 1, dtype=torch.int64)
    while H.shape[0] < h:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    return H


def sylvester_row(j, h):
    """H_h[j, :] in int64 without the dense matrix."""
    i = torch.arange(h, dtype=torch.int64) & j
    par = torch.zeros(h, dtype=torch.int64)
    for s in range(log2_of(h)):
        par ^= (i >> s) & 1
    return 1 - 2 * par


def scale32(h):
    """1.0f / sqrtf((float)h), as launch_fwht and flute_qgemm_ex compute it."""
    return torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(h), dtype=torch.float32))


def model(S, h, T, unit=1.0):
    """The documented arithmetic on exact sums: round_T(fl32(fl32(S * unit) * scale32)), valid while |S| < 2^24.  `unit`: a
    power of two that the inputs were multiples of (the subnormal cases), exact in fp32."""
    assert int(S.abs().max()) < EXACT_INT_LIMIT
    return ((S.to(torch.float32) * unit) * scale32(h)).to(T)


def reference(S, h, unit=1.0):
    """r = S / sqrt(h) in fp64."""
    return S.double() * unit / math.sqrt(h)


def bound(r, T):
    """The per-element bound on |y - r| (module docstring)."""
    b = (E.U_T[T] + REL_SLACK) * r.abs()
    return torch.where(r.abs() < MIN_NORMAL[T], b + MIN_SUBNORMAL[T] / 2, b)


def bound_excess(y, r, T):
    """max over the finite elements of y of |y - r| - bound (<= 0: within the bound)."""
    y = y.double().cpu()
    fin = torch.isfinite(y)
    return float(((y - r).abs() - bound(r, T))[fin].max()) if fin.any() else 0.0


def equal_by_value(y, m):
    """Element for element, -0.0 == +0.0 (the DPP stages carry a pending sign: v - v may come out as -0), inf == inf, and
    no NaN on either side."""
    y, m = y.double().cpu().reshape(-1), m.double().cpu().reshape(-1)
    return not bool(torch.isnan(y).any() or torch.isnan(m).any()) and torch.equal(y, m)


def inexact_share(S, h, T):
    """The share of results that the rounding to T changes."""
    r = reference(S, h)
    return float((r.to(T).double() != r).double().mean())


# ---------------------------------------------------------------------------
# draws: integers exact in T, |S| < 2^24
# ---------------------------------------------------------------------------

def spread_amp(h, T):
    return min(INT_MAX[T], int(8192 / math.sqrt(h)))


def spread(h, T, rows, seed):
    """Uniform integers in [-A, A], A = min(2047 | 255, floor(8192 / sqrt(h))): |r| <= A sqrt(h) <= 8192, nothing overflows."""
    gen = torch.Generator().manual_seed(seed)
    A = spread_amp(h, T)
    return torch.randint(-A, A + 1, (rows, h), generator=gen).to(T)


def concentrated(h, T, rows, seed):
    """h >= 1024: only the first 1024 elements of each block are nonzero, drawn from the full +-2047 / +-255 range: two
    512-blocks with large partial transforms that are inexact in T, while the results (divided by sqrt(h) >= 32) stay
    finite.  (One 512-block would not do at even log2(h): rounding commutes with the power-of-two scale.)"""
    assert h >= 1024
    gen = torch.Generator().manual_seed(seed)
    A = INT_MAX[T]
    x = torch.zeros(rows, h, dtype=torch.int64)
    x[:, :1024] = torch.randint(-A, A + 1, (rows, 1024), generator=gen)
    return x.to(T)


def impulse_positions(h):
    return sorted({0, h - 1} | {1 << s for s in range(log2_of(h))})


def impulses(h, T):
    """One row per position j in {0, 1, 2, 4, .., h / 2, h - 1}, a single 3 at j: the output is 3 H[j, :] / sqrt(h), so a
    failure names the index bit whose stage is wrong."""
    pos = impulse_positions(h)
    x = torch.zeros(len(pos), h, dtype=T)
    for row, j in enumerate(pos):
        x[row, j] = 3
    return x


def round_to(v, T):
    """fp64 values rounded ONCE to T's precision, to nearest even, as fp64 (normal range of T only: a cast from fp64 goes
    through fp32 and so rounds twice)."""
    _, e = torch.frexp(v)
    q = torch.ldexp(torch.ones_like(v), e - SIG_BITS[T])
    return torch.round(v / q) * q


def split_exact(W, T, max_terms):
    """The integer W as a sum of at most `max_terms` integers exact and finite in T (each the nearest such value to what is
    left), or None."""
    p, out, rem = SIG_BITS[T], [], W
    while rem and len(out) < max_terms:
        k = max(abs(rem).bit_length() - p, 0)
        t = int(round(rem / (1 << k))) << k                          # (round half to even; any nearest value will do)
        t = max(-32768, min(32768, t)) if abs(t) > FINITE_MAX[T] else t
        out.append(t)
        rem -= t
    return None if rem else out


_WITNESS = {}


def rounding_witness_sums(T):
    """The integers W < 2^20 at which one rounding and two differ: round_T(W c) != round_T(fl32(W c)), c = scale32(8192) (W c
    then lies in the normal range of fp16).  scale32(h) is c times a power of two at every odd log2(h), so they serve all of them."""
    if T not in _WITNESS:
        W = torch.arange(1, 1 << 20, dtype=torch.int64)
        c = scale32(8192)
        two = (W.to(torch.float32) * c).to(T).double()
        _WITNESS[T] = W[two != round_to(W.double() * c.double(), T)].tolist()
    return _WITNESS[T]


def rounding_witnesses(h, T, count=6):
    """Odd log2(h): up to `count` rows whose element 0 sums to a W of rounding_witness_sums (the terms of split_exact at positions
    0, 1, ..: H[j, 0] = 1 for every j), the result finite: a kernel that contracts the multiply and the conversion into one
    mixed-precision instruction (one rounding) returns another value there than scale_round's two roundings."""
    assert log2_of(h) % 2
    rows = []
    for W in rounding_witness_sums(T):
        terms = split_exact(W, T, min(h, 8))
        if terms is None or sum(abs(t) for t in terms) / math.sqrt(h) >= RESULT_CAP[T]:        # (every element of the row stays finite)
            continue
        x = torch.zeros(h, dtype=torch.int64)
        x[:len(terms)] = torch.tensor(terms)
        rows.append(x)
        if len(rows) == count:
            break
    return torch.stack(rows).to(T)


def mutant_single_rounding(S, h, T):
    """A kernel whose final multiply and conversion are one instruction with one rounding (fp64 values)."""
    return round_to(S.double() * scale32(h).double(), T)


def matrix_rows(h):
    """Row counts of the exact matrix.  h <= 512: 37 rows give a partial last wave, a second workgroup from h = 64 and the
    tail path of load8 / store8 at h = 2 (74 elements) and h = 4 (148); above, one workgroup per row."""
    return (1, 37) if h <= WAVE_MAX else (1, 3)


class Case:
    """One input of the exact matrix with its exact sums, the model's answer and the fp64 reference."""

    def __init__(self, name, x, h, T):
        self.name, self.x, self.h, self.T = name, x, h, T
        self.S = fwht_int(x, h)
        assert_premise(x, self.S, h, T)
        self.model = model(self.S, h, T)
        self.ref = reference(self.S, h)


_MATRIX = {}


def matrix_cases(h, T):
    """The exact matrix at (h, T): `spread` at both row counts, `concentrated` for h >= 1024, `impulses`, and at odd
    log2(h) the `rounding_witnesses`.  Built once and shared; nobody writes to it."""
    key = (h, T)
    if key not in _MATRIX:
        out = []
        for rows in matrix_rows(h):
            out.append(Case("spread-%d" % rows, spread(h, T, rows, E.seed_of("spread", h, str(T), rows)), h, T))
            if h >= 1024:
                out.append(Case("concentrated-%d" % rows, concentrated(h, T, rows, E.seed_of("conc", h, str(T), rows)), h, T))
        out.append(Case("impulses", impulses(h, T), h, T))
        if log2_of(h) % 2:
            out.append(Case("witness", rounding_witnesses(h, T), h, T))
        _MATRIX[key] = out
    return _MATRIX[key]


def subnormal_f16(h, rows, seed):
    """fp16 inputs k 2^-24, |k| <= 1023 (every one subnormal or zero); returns (x, k)."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(-1023, 1024, (rows, h), generator=gen)
    x = (k.double() * 2.0 ** -24).to(F16)
    assert torch.equal(x.double() * 2.0 ** 24, k.double())
    return x, k


def overflow_amp(h):
    """The smallest a of the form 2^k or 1.5 * 2^k with a sqrt(h) > 65520 (round_f16 then gives inf); a / 2 stays finite."""
    for k in range(1, 16):
        for a in (1 << k, 3 << (k - 1)):
            if a * math.sqrt(h) > 65520:
                return a
    raise AssertionError(h)


def overflow_f16(h, seed):
    """Four fp16 blocks: a H[j0, :] (the result a sqrt(h) at j0 passes 65520: +inf), -a H[j1, :] (-inf), (a / 2) H[j2, :]
    (finite, above 32760), and one `spread` block.  Every value is +-a or +-a / 2, a power of two or 1.5 times one."""
    a = overflow_amp(h)
    assert a % 2 == 0 and a <= 57344
    gen = torch.Generator().manual_seed(seed)
    j0, j1, j2 = (int(j) for j in torch.randint(0, h, (3,), generator=gen))
    x = torch.stack([a * sylvester_row(j0, h), -a * sylvester_row(j1, h), (a // 2) * sylvester_row(j2, h),
                     spread(h, F16, 1, seed)[0].to(torch.int64)])
    return x.to(F16), (j0, j1, j2)


def assert_premise(x, S, h, T, finite=True):
    """What makes model() the one allowed answer: integer inputs exact in T, |S| < 2^24; with `finite`, no result overflows."""
    xd = x.double()
    assert torch.equal(xd, xd.round()) and torch.equal(x.to(T).double(), xd), "inputs: integers exact in T"
    assert int(S.abs().max()) < EXACT_INT_LIMIT, int(S.abs().max())
    if finite:
        assert torch.isfinite(reference(S, h).to(T)).all()


# ---------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would return (the host test shows that the draws tell them from the model)
# ---------------------------------------------------------------------------

def mutant_round_partials(x, h, T):
    """A block kernel that keeps T values in LDS between its two phases: the 512-point partial transforms rounded to T, then
    the remaining stages, the scale and the final rounding."""
    assert h >= 1024
    P = fwht_int(x, 512).double().to(T).double().reshape(-1, h // 512, 512)          # [rows, h / 512, 512]
    rows = P.shape[0]
    v = _butterflies(P.transpose(1, 2).reshape(-1, h // 512), h // 512)                # the remaining bits, a transform of its own
    Sm = v.reshape(rows, 512, h // 512).transpose(1, 2).reshape(rows, h)
    return (Sm.to(torch.float32) * scale32(h)).to(T)


def mutant_round_then_scale(S, h, T):
    """A kernel that rounds the sums to T before it scales them."""
    return (S.double().to(T).to(torch.float32) * scale32(h)).to(T)


def differs(a, b):
    """Element mask: a and b differ by value (a NaN differs from everything)."""
    return ~(a.double() == b.double())


# ---------------------------------------------------------------------------
# reporting
# ---------------------------------------------------------------------------

def describe_index(e, h):
    """The index bits of element e of a block, named by the stage that handles them."""
    e %= h
    parts = ["reg=%d" % (e & 7), "dpp=%d" % ((e >> 3) & 15), "permlane=%d" % ((e >> 7) & 3)]
    if h > WAVE_MAX:
        parts.append("lds/r=%d" % (e >> 9))
    return "index %d (%s)" % (e, " ".join(parts))


def mismatch(y, m, h):
    """None when y equals m by value, else a description: h, the count, the first differing element and its index bits."""
    if equal_by_value(y, m):
        return None
    y, m = y.double().cpu().reshape(-1), m.double().cpu().reshape(-1)
    bad = differs(y, m).nonzero().reshape(-1)
    f = int(bad[0])
    return "h=%d: %d of %d elements differ; first at flat %d = block %d %s: got %r, model %r" % (
        h, len(bad), y.numel(), f, f // h, describe_index(f, h), float(y[f]), float(m[f]))


# ---------------------------------------------------------------------------
# the identity layer: D = had(X) @ I exposes every element of the fused rotation as an exact product
# ---------------------------------------------------------------------------

class IdentityLayer(E.Layer):
    """4 bits, TileP 32, g = 64, K = N = 1024: code 1 on the diagonal and 0 elsewhere, table [0, 1, 0, ..], scales 1."""

    def __init__(self, dtype):
        n = 16
        self.bits, self.K, self.N, self.g, self.dtype, self.seed, self.tile_p, self.pair = 4, 1024, 1024, 64, dtype, 0, 32, False
        self.table_div, self.scale_exp = 1, (0, 0)
        self.W = torch.eye(self.K, dtype=torch.uint8)
        t = torch.zeros(n, dtype=torch.float64)
        t[1] = 1
        self.pairs = torch.stack([t[:, None].expand(n, n), t[None, :].expand(n, n)], dim=-1).reshape(n * n, 2)
        self.table = t.to(dtype)
        q = self.table
        self.table2 = torch.stack([q[:, None].expand(n, n), q[None, :].expand(n, n)], dim=-1).contiguous().view(torch.float32)
        self.S64 = torch.ones(self.N, self.K // self.g, dtype=torch.float64)
        self.S = self.S64.to(dtype)
