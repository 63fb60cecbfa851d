"""What the long-row tests share (tests/test_long_rows_host.py, test_grouped_long_rows_gpu.py, test_row_stream_long_rows_gpu.py):
the shape, its constants derived from the 32-bit limits, the two row tables, the source-row bands, exact stacks per expert with
their chunked references, and NaN-guarded output buffers.  A test helper module (not a conftest, not a test module); importable
without a GPU.

The shape.  K = 7168 throughout: a row of a 16-bit tensor is 14 336 B, which divides neither 2^31 nor 2^32, so one row
straddles each limit.  K % 256 == 0 and (K / 64) % 8 == 0: every block form is eligible for the layer, and only the row counts
decide.  A DeepSeek-shaped prefill of 37 450 tokens at top-8 is R = 299 600 sorted rows: 4.0 GiB of gathered activations.

The data are exact by construction (tests/exact_cases.py): integer activations in [-4, 4] drawn on the device in 4096-row
chunks, integer tables, +-2^e scales, K 4 max|w| < 2^21, so each output element has ONE allowed value, round_T of the fp64
product, whatever the form or summation order.  `device_x`, `ExactStack.reference`, `cross_check` and `assert_equal_rows`
restate the helpers of tests/test_long_prefill_gpu.py for per-expert weights: that file is a test module, and test modules are
not imported from (README)."""
import math

import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import exact_layers, stack_exact

F16, BF16 = torch.float16, torch.bfloat16
GIB = 1 << 30
LIMIT = 0xFFFFFFF0               # grouped_rows.h: a descriptor's byte count stays below 2^32 - 16
K = 7168
ROW_BYTES = 2 * K
ROWS = 4096                      # row chunk of the device-side draws and checks
GUARD = 4096                     # elements on each side of a guarded output
BLOCK = 128                      # grouped_rows.h kGroupedBlockRows

ROW_2G = (1 << 31) // ROW_BYTES                       # its bytes straddle 2^31
ROW_4G = (1 << 32) // ROW_BYTES                       # ... and 2^32
T_EDGE = (LIMIT - 1) // ROW_BYTES - 256               # the last T the plain and weighted block forms admit
TSRC_EDGE = (LIMIT - 1) // ROW_BYTES                  # the last Tsrc the GLU block form admits
R_LONG = 300000                                       # [R_LONG, K] in 16 bits: 4.006 GiB, past 2^31 elements


def check_constants():
    """Both sides of every inequality the constants stand for."""
    assert ROW_BYTES == 14336 and (1 << 31) % ROW_BYTES and (1 << 32) % ROW_BYTES
    assert K % 256 == 0 and (K // 64) % 8 == 0
    assert ROW_2G == 149796 and ROW_2G * ROW_BYTES < 1 << 31 < (ROW_2G + 1) * ROW_BYTES
    assert (1 << 31) - ROW_2G * ROW_BYTES == 8192
    assert ROW_4G == 299593 and ROW_4G * ROW_BYTES < 1 << 32 < (ROW_4G + 1) * ROW_BYTES
    assert (1 << 32) - ROW_4G * ROW_BYTES == 2048
    assert T_EDGE == 299337 and (T_EDGE + 256) * ROW_BYTES < LIMIT <= (T_EDGE + 1 + 256) * ROW_BYTES
    assert TSRC_EDGE == 299593 and TSRC_EDGE * ROW_BYTES < LIMIT <= (TSRC_EDGE + 1) * ROW_BYTES
    assert T_EDGE + 1 < TSRC_EDGE + 1 < R_LONG < 2 ** 31 - 2 * BLOCK
    assert R_LONG * K > 1 << 31 and R_LONG * ROW_BYTES > 1 << 32
    assert abs(R_LONG * ROW_BYTES / GIB - 4.006) < 0.001


check_constants()


# ---- the row tables ------------------------------------------------------------------------------------------------------

def served_offsets(counts, served=None):
    """[0, c0, c0 + c1, ..], every entry clamped to `served` (the rows from there on are served by no expert)."""
    off = [0]
    for n in counts:
        off.append(off[-1] + n)
    return off if served is None else [min(o, served) for o in off]


def fat_counts(T):
    """E = 3: one expert holds all rows but 135, so its relative byte offsets reach the descriptor limit where T does, and its
    last 128-row block is ragged: its idle rows form offsets up to 127 rows past the expert's end."""
    counts = [5, T - 135, 130]
    assert sum(counts) == T and counts[1] % BLOCK
    return counts


def spread_counts(T):
    """E = 8, ragged counts (no multiple of 128), expert 1 empty: every relative offset is small, the expert bases carry the
    size.  Expert 3 starts two rows past the row that straddles 2^31; where T rows pass 2^32 bytes (T_EDGE rows do not: the
    eligibility rule ends 256 rows below), expert 7 starts past the row that straddles 2^32."""
    counts = [70001, 0, 79797, 333, 60013, 50021, T - 260165 - 203, 203]
    off = served_offsets(counts)
    assert sum(counts) == T and all(c % BLOCK for c in counts if c) and counts[6] > 0
    assert off[3] == ROW_2G + 2 and (off[2] < ROW_2G < off[3])
    if T > ROW_4G + 204:
        assert off[7] > ROW_4G
    return counts


TABLES = {"fat": fat_counts, "spread": spread_counts}


def bands(M, n_random=0, seed=0):
    """Sorted row indices below M: the first and the last 64, the rows around the two that straddle 2^31 and 2^32
    (ROW_2G - 1 .. ROW_2G + 1, ROW_4G - 1 .. ROW_4G + 1 where they exist), and `n_random` random rows."""
    rows = set(range(min(64, M))) | set(range(max(M - 64, 0), M))
    rows |= {r for r in (ROW_2G - 1, ROW_2G, ROW_2G + 1, ROW_4G - 1, ROW_4G, ROW_4G + 1) if 0 <= r < M}
    if n_random:
        gen = torch.Generator().manual_seed(seed)
        rows |= set(torch.randint(0, M, (n_random,), generator=gen).tolist())
    return sorted(rows)


def edge_rows(off):
    """The first and the last row of every expert that has rows."""
    out = []
    for e in range(len(off) - 1):
        if off[e + 1] > off[e]:
            out += [off[e], off[e + 1] - 1]
    return out


# ---- device data ---------------------------------------------------------------------------------------------------------

def device_ints(M, N, seed, dtype, amp=4, witness_rows=(), div=1):
    """Integers in [-amp, amp] (over `div`) from a seeded device generator, drawn in ROWS-row chunks; `witness_rows` are the
    accumulator witness, every entry `amp`."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty(M, N, dtype=dtype, device="cuda")
    for r0 in range(0, M, ROWS):
        r1 = min(M, r0 + ROWS)
        v = torch.randint(-amp, amp + 1, (r1 - r0, N), generator=gen, device="cuda", dtype=dtype)
        X[r0:r1] = v if div == 1 else v / div
    for r in witness_rows:
        X[r] = amp
    return X


def device_x(M, seed, dtype, witness_rows):
    """Integer activations [M, K] in [-4, 4]; `witness_rows` (the last row of every prefix a case uses) every entry 4."""
    return device_ints(M, K, seed, dtype, 4, witness_rows)


def nan_filled(rows, cols, dtype, dev):
    """[rows, cols] of the type's NaN bits."""
    return torch.full((rows, cols), XC.NAN_BITS[dtype], dtype=torch.int16, device=dev).view(dtype)


def snapshot(*tensors):
    """Bit copies of the inputs of a raw-pointer launch (None passes)."""
    return [None if t is None else t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()]).clone()
            for t in tensors]


def assert_unchanged(before, *tensors):
    for b, t in zip(before, tensors):
        if t is not None:
            assert torch.equal(b, t.view(b.dtype)), "an input was modified"


# ---- guarded outputs -----------------------------------------------------------------------------------------------------

NAN32 = 0x7FC00000


class Guarded:
    """An output [shape] of `dtype` in the middle of a buffer filled with the type's NaN bits (fp32: 0x7fc00000), GUARD
    elements on each side."""

    def __init__(self, shape, dtype, dev):
        self.n = math.prod(shape)
        self.canary, it = (NAN32, torch.int32) if dtype == torch.float32 else (XC.NAN_BITS[dtype], torch.int16)
        self.buf = torch.full((GUARD + self.n + GUARD,), self.canary, dtype=it, device=dev)
        self.out = self.buf[GUARD:GUARD + self.n].view(dtype).view(shape)

    def refill(self):
        self.buf.fill_(self.canary)

    def ints(self):
        return self.buf[GUARD:GUARD + self.n].view(self.out.shape)

    def assert_guards(self):
        assert torch.all(self.buf[:GUARD] == self.canary), "write in front of the output"
        assert torch.all(self.buf[GUARD + self.n:] == self.canary), "write behind the output"

    def assert_untouched(self):
        assert torch.all(self.buf == self.canary), "a refused launch wrote"

    def assert_written(self, r0=0, r1=None):
        """No element of rows [r0, r1) still holds NaN (the data are finite)."""
        out = self.out
        r1 = out.shape[0] if r1 is None else r1
        for a in range(r0, r1, ROWS):
            assert not torch.isnan(out[a:min(r1, a + ROWS)]).any(), ("output element left unwritten", a)

    def assert_unwritten(self, r0, r1):
        ints = self.ints()
        for a in range(r0, r1, ROWS):
            assert torch.all(ints[a:min(r1, a + ROWS)] == self.canary), ("a row no expert serves was written", a)

    def assert_zero_bits(self, r0, r1=None):
        ints = self.ints()
        r1 = ints.shape[0] if r1 is None else r1
        for a in range(r0, r1, ROWS):
            assert not ints[a:min(r1, a + ROWS)].any(), ("an unserved row is not +0", a)


def assert_equal_rows(D, R, what, r0=0, r1=None):
    """By value (-0.0 == +0.0, NaN never equal), chunk by chunk over rows [r0, r1)."""
    r1 = D.shape[0] if r1 is None else r1
    for a in range(r0, r1, ROWS):
        b = min(r1, a + ROWS)
        bad = D[a:b] != R[a:b]
        if bad.any():
            rr = torch.nonzero(bad.any(1))[:, 0] + a
            pytest.fail("%s: %d elements differ in rows [%d, %d), first row %d, last row %d"
                        % (what, int(bad.sum()), a, b, int(rr[0]), int(rr[-1])))


def assert_equal_bits(A, B, what):
    a, b = A.contiguous().view(torch.int16), B.contiguous().view(torch.int16)
    for r0 in range(0, a.shape[0], ROWS):
        assert torch.equal(a[r0:r0 + ROWS], b[r0:r0 + ROWS]), (what, "bits differ in the rows from", r0)


# ---- exact stacks --------------------------------------------------------------------------------------------------------

POW2_WEIGHTS = (0.25, 0.5, 1.0, 2.0, -1.0)          # +-2^e: w times an exact fp32 sum is exact


def device_row_weights(T, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    choice = torch.tensor(POW2_WEIGHTS, device="cuda")
    return choice[torch.randint(0, len(POW2_WEIGHTS), (T,), generator=gen, device="cuda")]


class ExactStack:
    """E exact layers [N, K = 7168] (4 / 2 bits, g = 64, TileP 32) on the device, each with its dense exact weight in fp64 and
    fp32, and the premise of exactness asserted for both contractions: K 4 max|w| < 2^21 (the forward, over K) and
    N 4 max|w| < 2^21 (the input gradient, over N) bound every sum of |x w|."""

    def __init__(self, env, bits, N, dtype, E, tag):
        self.bits, self.N, self.dtype, self.E, self.g = bits, N, dtype, E, 64
        seed0 = XC.seed_of("long rows", tag, bits, N, str(dtype), E) // 2
        self.layers = exact_layers(bits, 32, self.g, dtype, K, N, False, E, seed0)
        self.Q, self.S, self.t2, self.tid = stack_exact(env, self.layers)
        self.dev = env.dev
        self.W64 = [lay.w_exact(0, N, env.dev) for lay in self.layers]
        self.W32 = [W.float() for W in self.W64]
        for W, W32 in zip(self.W64, self.W32):
            assert torch.equal(W32.double(), W) and torch.equal(W.to(dtype).double(), W), "weights exact in fp32 and in T"
            assert torch.equal(W * 8, (W * 8).round()), "weights: multiples of 2^-3"
        self.wmax = max(float(W.abs().max()) for W in self.W64)
        assert self.wmax <= 16 and max(K, N) * 4 * self.wmax < XC.EXACT_SUM_LIMIT, ("sum |x w| may reach 2^21", self.wmax)

    def witness(self, x_row, e):
        """x_row (every entry 4) against expert e: an accumulator in T would end elsewhere."""
        XC.assert_witness(x_row.double().cpu(), self.layers[e].w_exact(0, 64), self.dtype)

    def _rounded(self, C, rw):
        assert torch.isfinite(C).all()
        if rw is not None:
            assert float(C.abs().max()) < 2.0 ** 19          # (w C is then exact in fp32 for every w of POW2_WEIGHTS)
            C = C * rw[:, None]
        if self.dtype == F16:
            assert float(C.abs().max()) <= XC.FP16_MAX
        return C.to(self.dtype)

    def _integers(self, Xc):
        assert torch.equal(Xc, Xc.round()) and float(Xc.abs().max()) <= 4, "operand rows: integers in [-4, 4]"

    def reference(self, X, off, rw=None, backward=False):
        """round_T(w_r X[r] @ W_e) for the rows [off[e], off[e + 1]) from fp32 (exact under the premise), zeros from off[E]
        on; `backward`: X is dY [T, N] and the product dY[r] @ W_e^T [T, K], the input gradient."""
        out = torch.zeros(X.shape[0], K if backward else self.N, dtype=self.dtype, device=X.device)
        for e in range(self.E):
            W = self.W32[e].T if backward else self.W32[e]
            for r0 in range(off[e], off[e + 1], ROWS):
                r1 = min(off[e + 1], r0 + ROWS)
                Xc = X[r0:r1].float()
                self._integers(Xc)
                out[r0:r1] = self._rounded(Xc @ W, None if rw is None else rw[r0:r1])
        return out

    def cross_check(self, X, R, off, rows, rw=None, backward=False):
        """On `rows` the fp32 product equals the fp64 one and R is its rounding to T."""
        rows = sorted({r for r in rows if 0 <= r < off[-1]})
        seen = 0
        for e in range(self.E):
            sel = [r for r in rows if off[e] <= r < off[e + 1]]
            if not sel:
                continue
            idx = torch.tensor(sel, device=X.device)
            Xb = X[idx]
            W64, W32 = (self.W64[e].T, self.W32[e].T) if backward else (self.W64[e], self.W32[e])
            R64 = Xb.double() @ W64
            assert torch.equal((Xb.float() @ W32).double(), R64), ("fp32 reference inexact", e)
            if rw is not None:
                R64 = R64 * rw[idx].double()[:, None]
            assert torch.equal(R[idx], R64.to(self.dtype)), ("reference rows differ from round_T(fp64)", e)
            seen += len(sel)
        assert seen == len(rows)


def check_rows(off, T):
    """The rows on which a reference is checked against fp64: the bands and the first and last row of every expert."""
    return bands(T) + edge_rows(off)
