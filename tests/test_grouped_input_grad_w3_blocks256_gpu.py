"""The 256-row block form of the grouped input gradient for 3-bit stacks (qgemm_grouped_input_grad_w3_blocks256.h: one workgroup per
256-row block of an expert x 256 k, waves of 128 rows x 64 k, the three-plane decoder) on the GPU, through
`qgemm_grouped_input_grad_w3_blocks256`, at the smallest shapes at which it can still go wrong: N = 512 is the narrowest 3-bit layer
(8 chunks), 1024 a second 512-column block; one and two k blocks; both group sizes; an expert with no block, a block whose upper
wave group is idle (1 row), partly filled (129), a full block (256), a second block (300 = 256 + 44), one expert with 257 rows, and
rows past offsets[E].

Every result must have the bits of `qgemm_grouped_input_grad(..., form="slabs")` and lie within exact_cases' componentwise bound
of the fp64 product with the exact lut * s weight."""
import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import random_stack
from tests.support import bits16, env, first_template, offsets_of  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
BITS, TILE_P = 3, 32
TABLES = [(0, 1, 129, 256, 300), (257,)]
TAIL = 3                                         # rows from offsets[E] on: served by no expert, written as zeros


def launch_both(env, counts, dY, stack, g, **operands):
    """(the 256-row block form's dX, the slab form's dX) for a table of `counts` followed by TAIL unserved rows."""
    args = (dY.to(env.dev), offsets_of(counts, env.dev), *stack, BITS, g, first_template(BITS, TILE_P))
    return env.fa.qgemm_grouped_input_grad_w3_blocks256(*args, **operands), env.fa.qgemm_grouped_input_grad(*args, form="slabs", **operands)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("g", [64, 32])
@pytest.mark.parametrize("N,K", [(512, 256), (512, 512), (1024, 256)])
def test_slab_bits_and_fp64_reference(env, N, K, g, dtype, pair):
    E = len(TABLES[0])
    Q, S, t2, Ws = random_stack(env, BITS, TILE_P, g, dtype, K, N, E, seed=3560)
    Q2, S2, t22, Ws2 = random_stack(env, BITS, TILE_P, g, dtype, K, N, E, seed=3570) if pair else (None,) * 4
    for counts in TABLES:
        first = E - len(counts)                                    # the one-expert table runs on the last expert's layers
        served, R = sum(counts), sum(counts) + TAIL
        gen = torch.Generator().manual_seed(R)
        dY = torch.randn(R, N, generator=gen).to(dtype)
        dY2 = torch.randn(R, N, generator=gen).to(dtype) if pair else None
        second = dict(grad_output2=dY2.to(env.dev), weight2=Q2[first:], scales2=S2[first:], table22=t22[first:]) if pair else {}
        new, slabs = launch_both(env, counts, dY, (Q[first:], S[first:], t2[first:]), g, **second)
        assert new.shape == (R, K) and new.dtype == dtype
        assert torch.equal(bits16(new), bits16(slabs)), (counts, "bits differ from the slab form")
        dX, off = new.cpu(), offsets_of(counts).tolist()
        assert torch.all(bits16(dX[served:]) == 0)
        for e in range(len(counts)):
            r0, r1 = off[e], off[e + 1]
            if r1 == r0:
                continue
            X, W = dY[r0:r1], Ws[first + e].T                      # W [N, K]
            if pair:
                X, W = torch.cat([X, dY2[r0:r1]], 1), torch.cat([W, Ws2[first + e].T], 0)
            XC.assert_componentwise(dX[r0:r1], X, W, X.shape[1], dtype, what=(counts, e))


@pytest.fixture(scope="module")
def small(env):
    g, dtype, N, K = 64, F16, 512, 256
    Q, S, t2, _ = random_stack(env, BITS, TILE_P, g, dtype, K, N, len(TABLES[0]), seed=3590)
    R = sum(TABLES[0]) + TAIL
    dY = torch.randn(R, N, generator=torch.Generator().manual_seed(3591)).to(dtype)
    return dict(g=g, stack=(Q, S, t2), dY=dY, R=R)


def test_row_weight_keeps_the_slab_bits(env, small):
    c = small
    rw = (torch.randn(c["R"], generator=torch.Generator().manual_seed(3592)) * 2).to(env.dev)
    new, slabs = launch_both(env, TABLES[0], c["dY"], c["stack"], c["g"], row_weight=rw)
    plain, _ = launch_both(env, TABLES[0], c["dY"], c["stack"], c["g"])
    assert torch.equal(bits16(new), bits16(slabs)) and not torch.equal(bits16(new), bits16(plain))


def test_a_non_finite_row_stays_in_its_row(env, small):
    """A NaN and an inf in row 200 of dY (inside the 256-row expert's block) make that row of dX NaN and change no other row's bits."""
    c = small
    clean, _ = launch_both(env, TABLES[0], c["dY"], c["stack"], c["g"])
    bad = c["dY"].clone()
    row = 200
    bad[row, 5], bad[row, 70] = float("nan"), float("inf")
    dX, slabs = launch_both(env, TABLES[0], bad, c["stack"], c["g"])
    assert torch.isnan(dX[row]).all() and torch.isnan(slabs[row]).all()
    keep = torch.arange(c["R"], device=env.dev) != row
    assert torch.equal(bits16(dX[keep]), bits16(clean[keep])) and torch.isfinite(dX[keep]).all()


def test_flute_experts_backward_keeps_its_bits(env):
    """One backward of a 3-bit FluteExperts(fused=True, native_routing=True) at top-1, 300 tokens over two experts: with
    `w3_grad_blocks256=True` hidden.grad is, bit for bit, the default's."""
    E, K, F, g, T, dtype, d = 2, 512, 512, 64, 300, F16, env.dev
    tid, gen = first_template(BITS, TILE_P), torch.Generator().manual_seed(35900)
    table = torch.randn(8, generator=gen).sort().values.to(dtype).to(d)

    def linear(kk, nn):
        codes = torch.randint(0, 8, (kk, nn), generator=gen, dtype=torch.uint8).to(d)
        scales = (torch.rand(nn, kk // g, generator=gen) * 0.1 + 0.02).to(dtype).to(d)
        return env.FluteLinear.from_codes(codes, scales, table, BITS, g, tid)

    layers = [[linear(kk, nn) for _ in range(E)] for kk, nn in ((K, F), (K, F), (F, K))]
    hidden = torch.randn(T, K, generator=gen).to(dtype).to(d)
    dOut = torch.randn(T, K, generator=gen).to(dtype).to(d)
    ids = torch.randint(0, E, (T, 1), generator=gen).to(d)
    weights = (torch.rand(T, 1, generator=gen) * 0.5 + 0.5).to(dtype).to(d)
    grads = {}
    for value in (False, True):
        experts = env.moe.FluteExperts.from_linears(*layers, fused=True, native_routing=True, w3_grad_blocks256=value)
        h = hidden.clone().requires_grad_()
        experts(h, ids, weights).backward(dOut)
        grads[value] = h.grad
    assert torch.isfinite(grads[False]).all() and float(grads[False].abs().max()) > 0
    assert torch.equal(bits16(grads[True]), bits16(grads[False]))
