"""The Hadamard cases' checkers, checked on the CPU (no GPU needed): tests/hadamard_cases.py.

The integer reference against the dense Sylvester matrix and against the oracle; for every input of the exact matrix what
makes the model the one allowed answer; that the model itself lies within the independent fp64 bound; and that the
mutants a wrong kernel could be (T values in LDS between the block kernel's phases; rounding before the scale; the scale and
the conversion contracted into one rounding) are told from the model by these inputs - so the GPU comparison is known to be able to fail.
"""
import math

import pytest
import torch

from oracle import flute_oracle as O
from tests import exact_cases as E
from tests import hadamard_cases as C

IDS = {C.F16: "f16", C.BF16: "bf16"}
dtypes = pytest.mark.parametrize("T", C.DTYPES, ids=IDS.get)


def test_fwht_int_is_the_sylvester_product():
    gen = torch.Generator().manual_seed(1)
    for h in C.SIZES[:10]:                                   # 2 .. 1024: the dense matrix stays small
        x = torch.randint(-2047, 2048, (5, h), generator=gen)
        H = C.sylvester(h)
        assert torch.equal(C.fwht_int(x, h), x @ H), h
        assert torch.equal(H, H.T) and torch.equal(H @ H, h * torch.eye(h, dtype=torch.int64))
        for j in (0, 1, h // 2, h - 1):
            assert torch.equal(C.sylvester_row(j, h), H[j]), (h, j)
    x = torch.randint(-9, 10, (2, 3, 64), generator=gen)     # any shape: the flat reshape(-1, h)
    assert torch.equal(C.fwht_int(x, 32), x.reshape(-1, 32) @ C.sylvester(32))


@dtypes
def test_fwht_int_rounded_equals_the_oracle(T):
    """Where 1 / sqrt(h) is a power of two the scale is exact, so round_T(S / sqrt(h)) is the oracle's answer and the model's."""
    for h in (4, 16, 64, 256):
        x = C.spread(h, T, 7, h)
        S = C.fwht_int(x, h)
        ref = O.hadamard_transform(x, h)
        assert torch.equal(C.reference(S, h).to(T).reshape(ref.shape), ref), h
        assert torch.equal(C.model(S, h, T).reshape(ref.shape), ref), h
    for h in (2, 8, 32, 128, 512):                           # elsewhere the oracle's fp64 product lies within the bound of r
        x = C.spread(h, T, 7, h)
        S = C.fwht_int(x, h)
        assert C.bound_excess(O.hadamard_transform(x, h).reshape(-1, h), C.reference(S, h), T) <= 0, h


def test_scale32_is_the_host_codes_float():
    for h in C.SIZES:
        s = float(C.scale32(h))
        assert abs(s * math.sqrt(h) - 1) <= 2.0 ** -23, h     # two fp32 roundings
        if C.log2_of(h) % 2 == 0:
            assert s == 2.0 ** -(C.log2_of(h) // 2)


@dtypes
@pytest.mark.parametrize("h", C.SIZES)
def test_exact_matrix_premises(h, T):
    """Every input of the exact matrix: integers exact in T, |S| < 2^24, no infinite result (asserted when the case is
    built), the model within the fp64 bound; `spread` rounds at least 15 % of its results."""
    cases = C.matrix_cases(h, T)
    names = {c.name.split("-")[0] for c in cases}
    assert names == ({"spread", "impulses"} | ({"concentrated"} if h >= 1024 else set()) | ({"witness"} if C.log2_of(h) % 2 else set())), names
    for c in cases:
        C.assert_premise(c.x, c.S, h, T)
        assert c.x.shape[1] == h and torch.isfinite(c.model).all()
        assert C.bound_excess(c.model, c.ref, T) <= 0, (h, c.name)
    S = torch.cat([c.S for c in cases if c.name.startswith("spread")])
    share = C.inexact_share(S, h, T)
    print("h=%d %s: spread inexact share %.3f over %d elements" % (h, IDS[T], share, S.numel()))
    assert share >= 0.15, (h, T, share)
    imp = [c for c in cases if c.name == "impulses"][0]
    pos = C.impulse_positions(h)
    assert pos[:2] == [0, 1] and pos[-1] == h - 1 and len(pos) == (C.log2_of(h) + 2 if h > 2 else 2)
    for row, j in enumerate(pos):
        assert torch.equal(imp.S[row], 3 * C.sylvester_row(j, h)), (h, j)


@dtypes
@pytest.mark.parametrize("h", [h for h in C.SIZES if h >= 1024])
def test_rounded_partials_mutant_is_rejected(h, T):
    """A block kernel that kept T values in LDS between its phases differs from the model in at least 25 % of the elements
    of every `concentrated` input."""
    for c in C.matrix_cases(h, T):
        if c.name.startswith("concentrated"):
            d = C.differs(C.mutant_round_partials(c.x, h, T), c.model)
            assert float(d.double().mean()) >= 0.25, (h, T, c.name, float(d.double().mean()))
            assert not C.equal_by_value(C.mutant_round_partials(c.x, h, T), c.model)


@dtypes
@pytest.mark.parametrize("h", [h for h in C.SIZES if C.log2_of(h) % 2])
def test_round_then_scale_mutant_is_rejected(h, T):
    """Rounding the sums to T before the scale shows at every odd log2(h)."""
    S = torch.cat([c.S for c in C.matrix_cases(h, T) if c.name.startswith("spread")])
    assert C.differs(C.mutant_round_then_scale(S, h, T), C.model(S, h, T)).any(), (h, T)


@dtypes
@pytest.mark.parametrize("h", [h for h in C.SIZES if C.log2_of(h) % 2])
def test_single_rounding_mutant_is_rejected(h, T):
    """A kernel that contracted the multiply with the scale and the conversion into one mixed-precision instruction (one
    rounding where scale_round makes two) differs from the model at element 0 of every witness row."""
    c = [c for c in C.matrix_cases(h, T) if c.name == "witness"][0]
    assert c.x.shape[0] >= 2 and set(c.S[:, 0].tolist()) <= set(C.rounding_witness_sums(T))
    m = C.mutant_single_rounding(c.S, h, T)
    assert bool((m[:, 0] != c.model.double()[:, 0]).all()), (h, T)
    assert C.bound_excess(m, c.ref, T) <= 0                # (both lie within the fp64 bound: only the bit comparison tells them apart)
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30, 3.0], dtype=torch.float64)              # round_to itself: one rounding
    assert C.round_to(x, C.F16).tolist() == [1.0 + 2.0 ** -10, 3.0] and x.to(C.F16).double().tolist() == [1.0, 3.0]


def test_mutant_partials_equal_model_without_rounding():
    """The mutant's own butterflies are right: with partials that are exact in T it is the model."""
    for h in (1024, 4096, 32768):
        x = torch.zeros(2, h, dtype=torch.int64)
        x[:, 5], x[:, 700], x[:, h - 1] = 3, -2, 1
        x = x.to(C.F16)
        assert C.equal_by_value(C.mutant_round_partials(x, h, C.F16), C.model(C.fwht_int(x, h), h, C.F16))


def test_split_exact():
    for T in C.DTYPES:
        for W in (1, 2047, 26327, 105308, 252703, 1010812):
            for n in (2, 8):
                terms = C.split_exact(W, T, n)
                if terms is not None:
                    t = torch.tensor(terms, dtype=torch.float64)
                    assert sum(terms) == W and len(terms) <= n and torch.equal(t.to(T).double(), t), (W, T, terms)
    assert C.split_exact(26327, C.F16, 2) == [26320, 7] and C.split_exact(252703, C.BF16, 2) == [252928, -225]
    assert C.split_exact(1010812, C.F16, 2) is None


def test_hostile_draws():
    for h in C.SIZES:
        x, (j0, j1, j2) = C.overflow_f16(h, h)
        S = C.fwht_int(x, h)
        C.assert_premise(x, S, h, C.F16, finite=False)
        m = C.model(S, h, C.F16)
        assert m[0, j0] == float("inf") and m[1, j1] == -float("inf") and int(torch.isinf(m).sum()) == 2, h
        assert torch.isfinite(m[2, j2]) and float(m[2, j2]) > 32760 and torch.isfinite(m[3]).all(), h
        assert not torch.isnan(m).any()
        x, k = C.subnormal_f16(h, 3, h)
        assert bool(((x != 0) & (x.abs().double() < C.MIN_NORMAL[C.F16])).any()) and float(x.abs().max()) < C.MIN_NORMAL[C.F16]
        S = C.fwht_int(k, h)
        assert int(S.abs().max()) < C.EXACT_INT_LIMIT
        m, r = C.model(S, h, C.F16, 2.0 ** -24), C.reference(S, h, 2.0 ** -24)
        sub = (m != 0) & (m.abs().double() < C.MIN_NORMAL[C.F16])
        assert float(sub.double().mean()) >= 0.5, (h, float(sub.double().mean()))      # subnormal results too
        assert C.bound_excess(m, r, C.F16) <= 0, h
        flushed = torch.where(sub, torch.zeros_like(m), m)
        assert not C.equal_by_value(flushed, m)


def test_equal_by_value_and_mismatch_report():
    a = torch.tensor([0.0, 1.0, -2.0, float("inf")], dtype=C.F16)
    b = torch.tensor([-0.0, 1.0, -2.0, float("inf")], dtype=C.F16)
    assert C.equal_by_value(a, b) and C.mismatch(a, b, 4) is None
    b[2] = 2.0
    assert not C.equal_by_value(a, b) and "index 2 (reg=2" in C.mismatch(a, b, 4)
    assert not C.equal_by_value(torch.tensor([float("nan")]), torch.tensor([float("nan")]))
    assert C.describe_index(4096 + 8 * 17 + 5 + 512 * 3, 4096) == "index %d (reg=5 dpp=1 permlane=1 lds/r=3)" % (8 * 17 + 5 + 512 * 3)
    assert C.bound_excess(torch.tensor([1.0 + 2.0 ** -9], dtype=C.F16), torch.tensor([1.0], dtype=torch.float64), C.F16) > 0


@dtypes
def test_identity_layer(T):
    lay = C.IdentityLayer(T)
    assert torch.equal(lay.w_exact(), torch.eye(1024, dtype=torch.float64))
    assert lay.N % E.cols_per_block(lay.bits, lay.tile_p) == 0 and lay.K % lay.g == 0
    assert lay.table.dtype == T and lay.S.shape == (1024, 16) and lay.table2.shape == (16, 16, 1)
