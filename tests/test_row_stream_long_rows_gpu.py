"""The row streams of the MoE backward past 2^31 elements: swiglu_grad, moe_gather, moe_combine and moe_weight_grad on
[R_LONG, 7168] tensors of 16 bits - 4.006 GiB each (tests/long_rows_cases.py has the constants and the helpers).

Each kernel forms its row from blockIdx.x / column blocks as an int and its element offset as (size_t) row * width + column;
a 32-bit product there would corrupt only the rows from ROW_2G (a byte offset past 2^31), from 2^31 / 7168 = 299 593.1 (an
element offset past 2^31) or from ROW_4G on.  So every element is compared, in 4096-row chunks on the device: the data are
drawn so that each result has one allowed value (integers and powers of two; for swiglu_grad the three exact regimes of its
formula: g = 0, 18 <= g <= 64, g <= -104), and swiglu_grad is held against the fp64 formula within the header's account as
well.  Every launch goes through the C ABI into buffers guarded on both sides with NaN bits, once with an `offsets` whose
offsets[E] is R - 300 - the rows from there on come back as +0 bits and whatever they hold is never read - and once with
offsets = None; guards and inputs must be as they were."""
import pytest
import torch

from tests import exact_cases as XC
from tests import long_rows_cases as LC
from tests import swiglu_grad_cases as SC
from tests.support import make_env

pytestmark = pytest.mark.gpu

F16, BF16 = LC.F16, LC.BF16
K, GIB, R, ROWS = LC.K, LC.GIB, LC.R_LONG, LC.ROWS
SERVED = R - 300
E = 8


@pytest.fixture(scope="module")
def env():
    e = make_env()
    torch.cuda.reset_peak_memory_stats(e.dev)
    yield e
    print("peak device memory: %.2f GiB" % (torch.cuda.max_memory_allocated(e.dev) / GIB))
    e.cache.clear()
    torch.cuda.empty_cache()


def need(gib):
    """Skip when the device cannot hold the case (peak of this module: DESIGN.md, "Long rows").  Blocks the allocator holds
    free count as free: the cache is kept between the tests, so the 4 GiB buffers of one test are the next one's."""
    free, _ = torch.cuda.mem_get_info()
    free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free < gib * GIB:
        pytest.skip("needs %.0f GiB of free device memory, %.1f GiB free" % (gib, free / GIB))


def dtype_id(dtype):
    return 0 if dtype == F16 else 1


def tables(env):
    """(offsets, rows served): the spread table with offsets[E] = R - 300, and no table."""
    off = torch.tensor(LC.served_offsets(LC.spread_counts(R), SERVED), dtype=torch.int32, device=env.dev)
    assert int(off[-1]) == SERVED and off.shape[0] == E + 1
    return ((off, SERVED), (None, R))


def poison_tail(*tensors):
    """The rows no expert serves hold NaN: they are never read."""
    for t in tensors:
        t[SERVED:] = float("nan")


def band_index(env, n_rows, seed):
    """The bands of tests/long_rows_cases.py below the served rows, with 3000 random rows, as a device index."""
    return torch.tensor(LC.bands(n_rows, 3000, seed), device=env.dev)


# ---- 6: swiglu_grad ------------------------------------------------------------------------------------------------------

LOW_G = (-104.0, -128.0, -1000.0)


def swiglu_operands(dtype, seed):
    """g, u, dh [R, K] drawn per chunk, and the regime of every element (int8): 0: g = 0, 1: g an integer in [18, 64],
    2: g <= -104.  dh = +-2^e, u an integer in [-3, 3]: dh u, dh u / 2 and dh g are exact in either type."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g, u, dh = (torch.empty(R, K, dtype=dtype, device="cuda") for _ in range(3))
    regime = torch.empty(R, K, dtype=torch.int8, device="cuda")
    pow2 = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0, -4.0], device="cuda")
    low = torch.tensor(LOW_G, device="cuda")
    draw = lambda lo, hi, n: torch.randint(lo, hi, (n, K), generator=gen, device="cuda")
    for r0 in range(0, R, ROWS):
        n = min(R, r0 + ROWS) - r0
        sel = draw(0, 3, n)
        mid = draw(18, 65, n).float()
        gg = torch.where(sel == 0, torch.zeros_like(mid), torch.where(sel == 1, mid, low[draw(0, 3, n)]))
        g[r0:r0 + n], regime[r0:r0 + n] = gg.to(dtype), sel.to(torch.int8)
        dh[r0:r0 + n] = pow2[draw(0, 8, n)].to(dtype)
        u[r0:r0 + n] = draw(-3, 4, n).to(dtype)
    return g, u, dh, regime


def swiglu_launch(env, g, u, dh, off, dg, du):
    rows, F = g.shape
    with torch.cuda.device(env.dev):
        env.check(env.lib.flute_swiglu_grad(dtype_id(g.dtype), rows, F, 0 if off is None else off.shape[0] - 1, g.data_ptr(),
                                            u.data_ptr(), dh.data_ptr(), None if off is None else off.data_ptr(),
                                            dg.out.data_ptr(), du.out.data_ptr(), env.stream_ptr(env.dev)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_swiglu_grad_past_2_31_elements(env, dtype):
    """dg, du against the exact value of each regime - g = 0: dh u / 2 and 0; 18 <= g <= 64: dh u and dh g; g <= -104: zeros
    of either sign - by value on every element, and against the fp64 formula within the header's account
    (swiglu_grad_cases.bounds, its constant read from the header; in the run without offsets only on the chunk that holds the
    rows the first run did not serve - the other operands are the first run's).  The bands are bit for bit a launch on their
    compact copy."""
    need(40)
    c = SC.header_c()
    g, u, dh, regime = swiglu_operands(dtype, XC.seed_of("long rows swiglu", str(dtype)))
    dg, du = LC.Guarded((R, K), dtype, env.dev), LC.Guarded((R, K), dtype, env.dev)
    band = band_index(env, SERVED, 61)
    cg, cu, cdh = g[band], u[band], dh[band]
    cdg, cdu = LC.Guarded(cg.shape, dtype, env.dev), LC.Guarded(cg.shape, dtype, env.dev)
    swiglu_launch(env, cg, cu, cdh, None, cdg, cdu)
    for off, served in tables(env):
        if off is not None:
            before = LC.snapshot(g[:served], u[:served], dh[:served])
            poison_tail(g, u, dh)
        else:
            if torch.isnan(g[-1]).any():                               # (the run with offsets came first)
                g[SERVED:], u[SERVED:], dh[SERVED:] = 0, 1, 1
                regime[SERVED:] = 0
            before = LC.snapshot(g, u, dh)
        dg.refill(), du.refill()
        swiglu_launch(env, g, u, dh, off, dg, du)
        dg.assert_guards(), du.assert_guards()
        dg.assert_zero_bits(served), du.assert_zero_bits(served)
        LC.assert_unchanged(before, g[:served], u[:served], dh[:served])
        worst = [0.0, 0.0]
        for r0 in range(0, served, ROWS):
            r1 = min(served, r0 + ROWS)
            gc, uc, hc, reg = g[r0:r1], u[r0:r1], dh[r0:r1], regime[r0:r1]
            prod = hc.double() * uc.double()
            want_dg = torch.where(reg == 0, prod / 2, torch.where(reg == 1, prod, torch.zeros_like(prod)))
            want_du = torch.where(reg == 1, hc.double() * gc.double(), torch.zeros_like(prod))
            assert torch.equal(want_dg.to(dtype).double(), want_dg) and torch.equal(want_du.to(dtype).double(), want_du)
            got_dg, got_du = dg.out[r0:r1].double(), du.out[r0:r1].double()
            assert torch.equal(got_dg, want_dg), ("dg", r0, off is not None)
            assert torch.equal(got_du, want_du), ("du", r0, off is not None)
            if off is None and r1 <= SERVED:                           # (the same operands as in the run with offsets)
                continue
            rdg, rdu, bdg, bdu, vdg, vdu = SC.bounds(gc, uc, hc, dtype, c)
            assert torch.all(((got_dg - rdg).abs() <= bdg) | vdg) and torch.all(((got_du - rdu).abs() <= bdu) | vdu), r0
            for i, (x, r, b, v) in enumerate(((got_dg, rdg, bdg, vdg), (got_du, rdu, bdu, vdu))):
                worst[i] = max(worst[i], float(torch.where(v, torch.zeros_like(b), (x - r).abs() / b).max()))
        print("swiglu_grad %s offsets %s: exact; worst error / bound dg %.3f du %.3f" % (dtype, off is not None, *worst))
        LC.assert_equal_bits(dg.out[band], cdg.out, "dg on the bands")
        LC.assert_equal_bits(du.out[band], cdu.out, "du on the bands")
        del before
    del g, u, dh, regime, dg, du


# ---- 7: moe_gather -------------------------------------------------------------------------------------------------------

def gather_launch(env, X, rows, off, out):
    Tsrc, width = X.shape
    with torch.cuda.device(env.dev):
        env.check(env.lib.flute_moe_gather(dtype_id(X.dtype), rows.shape[0], Tsrc, width, 0 if off is None else off.shape[0] - 1,
                                           X.data_ptr(), rows.data_ptr(), None if off is None else off.data_ptr(),
                                           out.out.data_ptr(), env.stream_ptr(env.dev)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_moe_gather_from_a_source_past_4_gib(env, dtype):
    """The source [R_LONG, 7168] is NaN bits but for the rows a 4096-entry `rows` names (the bands; the last entry names the
    last row): the output is bit for bit the compact copy, so a misaddressed read shows as NaN."""
    need(40)
    n = 4096
    src = band_index(env, R, 71)
    compact = LC.device_ints(src.shape[0], K, XC.seed_of("long rows gather", str(dtype)), dtype)
    X = LC.nan_filled(R, K, dtype, env.dev)
    X[src] = compact
    pick = torch.randint(0, src.shape[0], (n,), generator=torch.Generator().manual_seed(72)).to(env.dev)
    pick[-1] = src.shape[0] - 1
    rows = src[pick].int()
    assert int(rows[-1]) == R - 1
    want = compact[pick]
    before = LC.snapshot(X, rows)
    off = torch.tensor([0, 1000, 1000, n - 300], dtype=torch.int32, device=env.dev)
    for o, served in ((off, n - 300), (None, n)):
        out = LC.Guarded((n, K), dtype, env.dev)
        gather_launch(env, X, rows, o, out)
        out.assert_guards()
        out.assert_zero_bits(served)
        LC.assert_unchanged(before, X, rows)
        LC.assert_equal_bits(out.out[:served], want[:served], ("gather", o is not None))
    del X


def test_moe_gather_into_an_output_past_4_gib(env):
    """A 200-row source, `rows` [R_LONG] and an output of 4.006 GiB: X[rows], chunk by chunk; with offsets the tail is +0 and
    its `rows` entries (far outside the source) are never read."""
    need(40)
    dtype = F16
    X = LC.device_ints(200, K, XC.seed_of("long rows gather out"), dtype)
    rows = torch.randint(0, 200, (R,), generator=torch.Generator().manual_seed(73)).int().to(env.dev)
    before = LC.snapshot(X)
    out = LC.Guarded((R, K), dtype, env.dev)
    for off, served in tables(env):
        r = rows.clone()
        if off is not None:
            r[served:] = 2 ** 31 - 1
        out.refill()
        gather_launch(env, X, r, off, out)
        out.assert_guards()
        out.assert_zero_bits(served)
        LC.assert_unchanged(before, X)
        for r0 in range(0, served, ROWS):
            r1 = min(served, r0 + ROWS)
            assert torch.equal(out.out[r0:r1].view(torch.int16), X[rows[r0:r1].long()].view(torch.int16)), r0
    del out


# ---- 8: moe_combine ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16])
def test_moe_combine_over_4_gib_of_rows(env, dtype):
    """Y [R_LONG, 7168] of integers in [-4, 4], pos from moe_route on 37 500 tokens at top-8 with 300 pairs no expert serves
    (offsets[E] = R - 300): out[t] is the fp32 sum over the served slots in slot order - at most eight integers, exact - rounded
    once.  `rows` is read by the backward only: with it the gradient of Y is one moe_gather launch, bit for bit the plain
    backward, +0 in the rows no expert serves."""
    need(40)
    T, k = 37500, 8
    assert T * k == R
    gen = torch.Generator().manual_seed(81)
    ids = torch.rand(T, 2 * E, generator=gen).argsort(1)[:, :k].int().contiguous()  # k distinct experts of 16
    flat = ids.view(-1)
    flat[torch.randperm(R, generator=gen)[:300]] = 2 * E                          # 300 pairs whose id no expert has
    ids = ids.to(env.dev)
    offsets, rows, _, pos, _ = env.fa.moe_route(ids, None, 2 * E)
    assert int(offsets[-1]) == SERVED and pos.shape == (T, k) and int(pos.max()) == R - 1
    Y = LC.device_ints(R, K, XC.seed_of("long rows combine", str(dtype)), dtype)
    Y[SERVED:] = float("nan")                                                     # never read
    before = LC.snapshot(Y, pos, offsets)
    out = LC.Guarded((T, K), dtype, env.dev)
    with torch.cuda.device(env.dev):
        env.check(env.lib.flute_moe_combine(dtype_id(dtype), T, k, 2 * E, K, Y.data_ptr(), pos.data_ptr(), offsets.data_ptr(),
                                            out.out.data_ptr(), env.stream_ptr(env.dev)))
    torch.cuda.synchronize()
    out.assert_guards()
    out.assert_written()
    LC.assert_unchanged(before, Y, pos, offsets)
    step = 1024
    for t0 in range(0, T, step):
        p = pos[t0:t0 + step].long()
        live = p < SERVED
        acc = torch.zeros(p.shape[0], K, dtype=torch.float32, device=env.dev)
        for j in range(k):                                                        # slot order, fp32
            acc += torch.where(live[:, j, None], Y[p[:, j].clamp(max=SERVED - 1)].float(), torch.zeros_like(acc))
        assert torch.equal(out.out[t0:t0 + step].float(), acc.to(dtype).float()), t0
    by_op = env.fa.moe_combine(Y, pos, offsets)
    LC.assert_equal_bits(by_op, out.out, "the operator")
    del by_op, before, out
    # the backward: with `rows` (one moe_gather launch) and without (torch ops)
    dOut = LC.device_ints(T, K, XC.seed_of("long rows combine grad", str(dtype)), dtype)
    grads = []
    for r in (rows, None):
        y = Y.detach().requires_grad_()
        env.fa.moe_combine(y, pos, offsets, r).backward(dOut)
        grads.append(y.grad)
        del y
    LC.assert_equal_bits(grads[0], grads[1], "backward with rows and without")
    assert not grads[0][SERVED:].view(torch.int16).any()
    for r0 in range(0, SERVED, ROWS):
        r1 = min(SERVED, r0 + ROWS)
        assert torch.equal(grads[0][r0:r1].view(torch.int16), dOut[rows[r0:r1].long()].view(torch.int16)), r0
    del grads, Y


# ---- 9: moe_weight_grad --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16])
def test_moe_weight_grad_past_2_31_elements(env, dtype):
    """dHp and h integers in [-4, 4]: d_row_weight is the exact row sum (|sum| <= 7168 x 16 < 2^24, exact in fp32 in any order)
    and dH is bit for bit round_T(w dHp), w in {0.25, 0.5, 1, 2, -1}; the rows from offsets[E] on are +0 in both."""
    need(40)
    dHp = LC.device_ints(R, K, XC.seed_of("long rows wg dhp", str(dtype)), dtype)
    H = LC.device_ints(R, K, XC.seed_of("long rows wg h", str(dtype)), dtype)
    rw = LC.device_row_weights(R, 91)
    assert K * 16 < 2 ** 24
    dw, dH = LC.Guarded((R,), torch.float32, env.dev), LC.Guarded((R, K), dtype, env.dev)
    for off, served in tables(env):
        if off is not None:
            poison_tail(dHp, H)
            rw[SERVED:] = float("nan")
            before = LC.snapshot(dHp[:served], H[:served], rw[:served])
        else:
            dHp[SERVED:], H[SERVED:], rw[SERVED:] = 4, -4, 2.0                  # the tail serves as rows of the largest sum
            before = LC.snapshot(dHp, H, rw)
        dw.refill(), dH.refill()
        with torch.cuda.device(env.dev):
            env.check(env.lib.flute_moe_weight_grad(dtype_id(dtype), R, K, 0 if off is None else off.shape[0] - 1, dHp.data_ptr(),
                                                    H.data_ptr(), rw.data_ptr(), None if off is None else off.data_ptr(),
                                                    dw.out.data_ptr(), dH.out.data_ptr(), env.stream_ptr(env.dev)))
        torch.cuda.synchronize()
        dw.assert_guards(), dH.assert_guards()
        dH.assert_zero_bits(served)
        assert not dw.out[served:].view(torch.int32).any()
        LC.assert_unchanged(before, dHp[:served], H[:served], rw[:served])
        for r0 in range(0, served, ROWS):
            r1 = min(served, r0 + ROWS)
            a, b = dHp[r0:r1].double(), H[r0:r1].double()
            assert torch.equal(dw.out[r0:r1].double(), (a * b).sum(1)), ("d_row_weight", r0)
            want = a * rw[r0:r1].double()[:, None]
            assert torch.equal(want.to(dtype).double(), want)
            assert torch.equal(dH.out[r0:r1].view(torch.int16), want.to(dtype).view(torch.int16)), ("dH", r0)
        if off is None:
            assert float(dw.out[-1]) == -16.0 * K
        del before
    del dHp, H, dw, dH
