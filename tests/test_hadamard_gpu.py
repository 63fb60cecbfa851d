"""The Hadamard transform, bit for bit, at every h = 2 .. 32768, out of place and in place, stand-alone and fused.

On integer input every fp32 partial sum of the butterflies is exact whatever their order, so the documented arithmetic
(fp32 butterflies, the product with 1.0f / sqrtf(h) rounded to fp32, one rounding to T) allows one answer only:
`hadamard_cases.model` of the exact integer sums.  Every launch through the C ABI reads its input from the middle of a
NaN-filled buffer and writes into the middle of another (in place: into its input); afterwards the guard bands are
intact, every output element was written and an out-of-place input is unchanged.  Results are compared by value
(-0.0 == +0.0: the DPP stages carry a pending sign, so v - v may come out as -0), element for element, and separately
against the fp64 reference within (u_T + 2^-21) |r|.  tests/test_hadamard_host.py shows on the CPU that these inputs tell
a kernel that keeps T values between the block kernel's phases, that rounds before it scales, or that contracts the scale
and the conversion into one rounding, from the model.

This is also where csrc/fwht.h's claim is tested that the DPP / lane-swap form of the lane stages returns the bits of
the plain butterflies: the model is the plain butterflies.
"""
import pytest
import torch

from tests import exact_cases as E
from tests import hadamard_cases as C
from tests.qgemm_cases import GUARD, Carved, DevLayer, check_plan, guarded_qgemm
from tests.support import bits16, env  # noqa: F401

pytestmark = pytest.mark.gpu

IDS = {C.F16: "f16", C.BF16: "bf16"}
dtypes = pytest.mark.parametrize("T", C.DTYPES, ids=IDS.get)


def launch(env, x, h, in_place=False, nonfinite=False):
    """flute_hadamard on a Carved copy of `x` (CPU, any shape, numel % h == 0), into a NaN-prefilled output between NaN
    guard bands, or with in == out on the copy.  Checks the guards, that every element was written (`nonfinite`: the input
    holds NaN or Inf itself) and, out of place, that the input is unchanged.  Returns the result on the CPU, [numel / h, h]."""
    T, n = x.dtype, x.numel()
    nan = E.NAN_BITS[T]
    Xc = Carved(x, env.dev, nan)
    if in_place:
        out = Xc.t
    else:
        buf = torch.full((GUARD + n + GUARD,), nan, dtype=torch.int16, device=env.dev)
        out = buf[GUARD:GUARD + n].view(T)
        assert out.data_ptr() % 16 == 0
        before = bits16(Xc.t).clone()
    with torch.cuda.device(env.dev):
        rc = env.lib.flute_hadamard(0 if T == torch.float16 else 1, Xc.t.data_ptr(), out.data_ptr(), n, h, env.stream_ptr(env.dev))
    env.check(rc)
    torch.cuda.synchronize()
    assert Xc.intact(), "write outside the input (h=%d, in_place=%s)" % (h, in_place)
    if not in_place:
        assert torch.all(buf[:GUARD] == nan) and torch.all(buf[GUARD + n:] == nan), "write outside out (h=%d)" % h
        assert torch.equal(bits16(Xc.t), before), "the input was modified (h=%d)" % h
    assert nonfinite or not torch.isnan(out).any(), "output element left unwritten or NaN (h=%d, in_place=%s)" % (h, in_place)
    return out.clone().cpu().reshape(-1, h)


@dtypes
@pytest.mark.parametrize("h", C.SIZES)
def test_exact_matrix(env, h, T):
    """`spread` at both row counts, `concentrated` for h >= 1024, `impulses`, the rounding witnesses at odd log2(h); each out of
    place and in place."""
    compared = 0
    for c in C.matrix_cases(h, T):
        for in_place in (False, True):
            y = launch(env, c.x, h, in_place)
            bad = C.mismatch(y, c.model, h)
            assert bad is None, (c.name, IDS[T], "in place" if in_place else "out of place", bad)
            assert C.bound_excess(y, c.ref, T) <= 0, (h, c.name, in_place)
            compared += y.numel()
    print("h=%d %s: %d elements compared bit for bit" % (h, IDS[T], compared))


@dtypes
def test_python_entry_shapes_and_views(env, T):
    """flute_amd.hadamard_transform: flat reshape(-1, h) semantics on 3-D input and on a last dimension that h does not divide;
    a transposed view and a misaligned buf[1:1 + n] view (cloned on the way in) equal the call on a contiguous copy bit for bit
    and leave their input untouched."""
    had, d = env.fa.hadamard_transform, env.dev
    for h in (8, 64, 512, 2048):
        x = C.spread(h, T, 24, E.seed_of("entry", h)).reshape(2, 3, 4 * h)
        y = had(x.to(d), h)
        assert y.shape == x.shape and y.dtype == T
        bad = C.mismatch(y.reshape(-1, h), C.model(C.fwht_int(x, h), h, T), h)
        assert bad is None, bad
    x = C.spread(64, T, 3, 5).reshape(2, 96)                  # 96 % 64 != 0, numel % 64 == 0
    y = had(x.to(d), 64)
    assert y.shape == (2, 96) and C.mismatch(y.reshape(-1, 64), C.model(C.fwht_int(x, 64), 64, T), 64) is None
    with pytest.raises(RuntimeError):
        had(x[:, :95].to(d), 64)
    for h in (64, 1024):
        base = C.spread(h, T, 6, E.seed_of("views", h)).to(d)
        tr = base.T.contiguous().T                            # [6, h] with strides (1, 6)
        assert not tr.is_contiguous() and torch.equal(tr, base)
        buf = torch.zeros(1 + base.numel() + 7, dtype=T, device=d)
        buf[1:1 + base.numel()] = base.reshape(-1)
        mis = buf[1:1 + base.numel()].view(6, h)
        assert mis.is_contiguous() and mis.data_ptr() % 16 != 0
        want = had(base.clone(), h)
        assert C.mismatch(want, C.model(C.fwht_int(base.cpu(), h), h, T), h) is None
        for name, v in (("transposed", tr), ("misaligned", mis)):
            keep = bits16(v).clone()
            got = had(v, h)
            assert got.shape == v.shape and torch.equal(bits16(got), bits16(want)), (h, name)
            assert torch.equal(bits16(v), keep), (h, name, "input modified")
        assert float(buf[0]) == 0 and not buf[1 + base.numel():].any()


@pytest.fixture(scope="module")
def identity(env):
    return {T: DevLayer(env, C.IdentityLayer(T)) for T in C.DTYPES}


def _operator(env, dl, X, h):
    lay = dl.lay
    return env.fa.qgemm_hadamard(X.to(env.dev), dl.Q, dl.S, dl.table, dl.table2, env.ws, lay.bits, lay.g, h, dl.tid, env.num_sms)


@dtypes
@pytest.mark.parametrize("h", C.SIZES[:9])
def test_fused_rotation_through_identity_layer(env, identity, h, T):
    """D = had(X) @ I: every element of the decode kernel's fused rotation (fwht_piece) as an exact product, h = 2 .. 512,
    M = 1 and 4, forced onto the decode kernels through the C ABI (the family's own choice and each of its kernels that carries a
    copy of the rotation) and through the operator's automatic plan."""
    dl = identity[T]
    lay, fa = dl.lay, env.fa
    for M in (1, 4):
        X = C.spread(h, T, M * lay.K // h, E.seed_of("fused", h, M))
        if C.log2_of(h) % 2:                                  # the first blocks: where one rounding and scale_round's two differ
            wit = C.rounding_witnesses(h, T)[:X.shape[0] // 2]
            X[:wit.shape[0]] = wit
        X = X.reshape(M, lay.K)
        want = C.model(C.fwht_int(X, h), h, T).reshape(M, lay.K)
        fused = env.lib.flute_qgemm_hadamard_fused(0 if T == torch.float16 else 1, lay.bits, lay.g, h, M, lay.N, lay.K, dl.tid,
                                                   env.num_sms, env.ws.numel())
        print("h=%d %s M=%d: automatic plan fuses the rotation: %d" % (h, IDS[T], M, fused))
        assert fused == 1, (h, M, fused)                      # M * K <= 8192 and h <= 512: the operator's launch is the fused one
        two = fa.qgemm(fa.hadamard_transform(X.to(env.dev), h), dl.Q, dl.S, dl.table, dl.table2, env.ws, lay.bits, lay.g, dl.tid, env.num_sms)
        outs = {"decode": guarded_qgemm(env, dl, X, dict(family=0), hadamard_size=h), "operator": _operator(env, dl, X, h), "two": two}
        # each decode kernel that carries a copy of the rotation: ring (one_shot 0), one-shot (1), persistent one-shot (2, M <= 2)
        for one, code in ((0, 0), (1, (1, 2)), (2, 3)):
            if one == 2 and M > 2:
                continue
            ovr = dict(family=0, one_shot=one)
            check_plan(env, dl, M, ovr, dict(family=0, one_shot=code))
            outs["one_shot=%d" % one] = guarded_qgemm(env, dl, X, ovr, hadamard_size=h)
        for name, D in outs.items():
            bad = C.mismatch(D, want, h)
            assert bad is None, (name, IDS[T], M, bad)
            assert torch.equal(D.double().cpu(), two.double().cpu()), (name, "differs from qgemm(hadamard_transform(X))")
            assert C.bound_excess(D.reshape(-1, h), C.reference(C.fwht_int(X, h), h), T) <= 0, (name, h, M)
    assert dl.guards_intact()


@dtypes
def test_operator_two_launches_at_1024(env, identity, T):
    """h = 1024 is above the fused range: the operator rotates into its scratch with the block kernel, then multiplies."""
    dl, h = identity[T], 1024
    lay = dl.lay
    for M in (1, 4):
        X = C.concentrated(h, T, M, E.seed_of("op1024", M)).reshape(M, lay.K)
        fused = env.lib.flute_qgemm_hadamard_fused(0 if T == torch.float16 else 1, lay.bits, lay.g, h, M, lay.N, lay.K, dl.tid,
                                                   env.num_sms, env.ws.numel())
        assert fused == 0, (M, fused)
        want = C.model(C.fwht_int(X, h), h, T).reshape(M, lay.K)
        for name, D in (("operator", _operator(env, dl, X, h)), ("guarded", guarded_qgemm(env, dl, X, None, hadamard_size=h))):
            bad = C.mismatch(D, want, h)
            assert bad is None, (name, IDS[T], M, bad)


HOSTILE_SIZES = (2, 16, 128, 512, 2048)


def _equal_with_nan(a, b):
    a, b = a.double(), b.double()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0), b.masked_fill(nb, 0))


@dtypes
@pytest.mark.parametrize("h", HOSTILE_SIZES)
def test_nonfinite_blocks_are_contained(env, h, T):
    """One NaN in block 1, one +Inf in block 2, one -Inf in block 3 of a clean `spread` input: at h <= 128 these blocks share a
    wave with their neighbours, at h = 16 a DPP row, at h = 2 a lane.  The NaN block is all NaN, the Inf blocks are +-Inf with
    the sign of H[j, i], every other block has the bits of the clean launch."""
    rows = 37 if h <= C.WAVE_MAX else 5
    x = C.spread(h, T, rows, E.seed_of("hostile", h))
    jn, jp, jm = h - 1, 0 if h == 2 else 5 % h, h // 2
    bad = x.clone()
    bad[1, jn], bad[2, jp], bad[3, jm] = float("nan"), float("inf"), -float("inf")
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    want_p, want_m = C.sylvester_row(jp, h).double() * inf, -C.sylvester_row(jm, h).double() * inf
    for in_place in (False, True):
        clean = launch(env, x, h, in_place)
        assert C.mismatch(clean, C.model(C.fwht_int(x, h), h, T), h) is None
        y = launch(env, bad, h, in_place, nonfinite=True)
        assert torch.isnan(y[1]).all(), (h, "NaN block", int(torch.isnan(y[1]).sum()))
        assert torch.equal(y[2].double(), want_p), (h, "+Inf block")
        assert torch.equal(y[3].double(), want_m), (h, "-Inf block")
        others = [0] + list(range(4, rows))
        assert torch.equal(bits16(y[others]), bits16(clean[others])), (h, "a clean block changed", in_place)


@pytest.mark.parametrize("h", HOSTILE_SIZES)
def test_f16_overflow_and_subnormals(env, h):
    """fp16 range edges: results past 65520 are +-Inf exactly where the model's are (and nowhere else); subnormal inputs
    k 2^-24 and subnormal results equal the model - nothing is flushed."""
    T = C.F16
    x, (j0, j1, j2) = C.overflow_f16(h, h)
    m = C.model(C.fwht_int(x, h), h, T)
    assert m[0, j0] == float("inf") and m[1, j1] == -float("inf") and int(torch.isinf(m).sum()) == 2
    xs, k = C.subnormal_f16(h, 5, E.seed_of("sub", h))
    Ss = C.fwht_int(k, h)
    ms, rs = C.model(Ss, h, T, 2.0 ** -24), C.reference(Ss, h, 2.0 ** -24)
    assert bool(((ms != 0) & (ms.abs().double() < C.MIN_NORMAL[T])).any())
    for in_place in (False, True):
        y = launch(env, x, h, in_place)
        bad = C.mismatch(y, m, h)
        assert bad is None, ("overflow", in_place, bad)
        ys = launch(env, xs, h, in_place)
        bad = C.mismatch(ys, ms, h)
        assert bad is None, ("subnormal", in_place, bad)
        assert C.bound_excess(ys, rs, T) <= 0


@dtypes
def test_repeat_launch_returns_equal_bits(env, T):
    for h in (2, 128, 512, 1024, 16384, 32768):
        x = C.spread(h, T, 3, E.seed_of("repeat", h))
        assert torch.equal(bits16(launch(env, x, h)), bits16(launch(env, x, h))), h


@dtypes
@pytest.mark.parametrize("h", [64, 2048, 32768])
def test_graph_replay_follows_the_input(env, h, T):
    """hadamard_transform captured into a graph and replayed after the input buffer's content changed returns the eager
    result of the new content (launch_fwht sets the dynamic LDS limit of the h >= 16384 kernels on the way)."""
    had, d = env.fa.hadamard_transform, env.dev
    x0, x1 = (C.spread(h, T, 3, E.seed_of("graph", h, i)) for i in (0, 1))
    buf = x0.to(d)
    side = torch.cuda.Stream(d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        had(buf, h)                                           # first use outside the capture
    torch.cuda.current_stream(d).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = had(buf, h)
    for x in (x1, x0, x1):
        buf.copy_(x.to(d))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits16(y), bits16(had(buf, h))), h
        bad = C.mismatch(y, C.model(C.fwht_int(x, h), h, T), h)
        assert bad is None, bad
