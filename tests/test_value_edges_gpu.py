"""The dense qgemm kernels at the edges of the fp16 range and on non-finite rows (tests/exact_cases.py, edge_cases).

The exact tests stay in one operating region: integer activations, weights of ordinary size, finite outputs.  Here every
family runs, per bit width and per way of combining K, exact cases whose weights are fp16 subnormals, whose activations
are fp16 subnormals, and whose exact result overflows fp16 in both directions - each still with one allowed answer,
round_T(X @ W_exact), infinities included - and cases with one NaN and one +Inf in X (fp16 and bf16), whose answer
follows by rule: the NaN row is NaN, the Inf row is +-inf by the sign of the weight it meets (NaN where that weight is
zero), every other row has the bits of the clean launch.  Every launch goes through qgemm_cases.guarded_qgemm: all
operands and the output between poisoned guards.  Measured on gfx950: no family flushes an fp16 subnormal operand - the
packed dot instructions and the matrix unit keep them - so the documented arithmetic holds without exception."""
import pytest
import torch

from tests import exact_cases as E
from tests import qgemm_cases as G
from tests.support import env  # noqa: F401

pytestmark = pytest.mark.gpu


def differing(D, R, T):
    return int((D.double().cpu() != R.to(T).double().cpu()).sum())


def diagnose(env, D, X, lay):
    """Which other product D equals, for the failure message: the operands with their fp16 subnormals flushed, or a
    result saturated at 65504."""
    T, out = lay.dtype, []
    for fw, fx in ((True, False), (False, True), (True, True)):
        if E.exact_equal(D, E.exact_product(X, lay, env.dev, flush_w=fw, flush_x=fx), T):
            out.append("equals the product with subnormal %s flushed" % "+".join(n for n, f in (("w", fw), ("x", fx)) if f))
    R = E.exact_product(X, lay, env.dev)
    if E.exact_equal(D, R.clamp(-E.FP16_MAX, E.FP16_MAX), T):
        out.append("saturates at 65504")
    out.append("%d NaN, %d inf in D" % (int(torch.isnan(D).sum()), int(torch.isinf(D).sum())))
    return out


def run_range_edge(env, dl, kind, M, ovr):
    lay = dl.lay
    X = E.edge_x(kind, M, lay, E.seed_of(kind, M))
    R, A = E.exact_product(X, lay, env.dev, abs_too=True)
    E.premise_edge(kind, X, lay, R.cpu(), A.cpu())
    D = G.guarded_qgemm(env, dl, X, ovr)
    if not E.exact_equal(D, R, lay.dtype):
        return [(kind, lay, M, ovr, differing(D, R, lay.dtype), diagnose(env, D, X, lay))]
    return []


def run_nonfinite(env, dl, M, ovr):
    lay = dl.lay
    K = lay.K
    X = E.make_x(M, K, E.seed_of("nonfinite", M), lay.dtype)
    R, A = E.exact_product(X, lay, env.dev, abs_too=True)
    E.premise(X, lay, R.cpu(), A.cpu(), witness=False)
    clean = G.guarded_qgemm(env, dl, X, ovr)
    failed = []
    if not E.exact_equal(clean, R, lay.dtype):
        failed.append(("clean", lay, M, ovr, differing(clean, R, lay.dtype)))
    m_nan, m_inf = 0, 1
    # once inside the first K chunk, once in the last group of K (an even and an odd k: both halves of a packed pair)
    for where, k_nan, k_inf in (("first chunk", 3, 6), ("last group", K - 2, K - 5)):
        D = G.guarded_qgemm(env, dl, E.poison_x(X, m_nan, m_inf, k_nan, k_inf), ovr, nan_expected=True)
        exp = E.nonfinite_expected(clean, lay, m_nan, m_inf, k_inf)
        if not E.nonfinite_equal(D, exp):
            D = D.cpu()
            rows = [m for m in range(M) if not E.nonfinite_equal(D[m], exp[m])]
            failed.append((where, lay, M, ovr, "rows", rows, "NaN row all NaN", bool(torch.isnan(D[m_nan]).all()),
                           "Inf row: %d NaN, %d +inf, %d -inf, expected %d, %d, %d" % (
                               int(torch.isnan(D[m_inf]).sum()), int((D[m_inf] == float("inf")).sum()), int((D[m_inf] == -float("inf")).sum()),
                               int(torch.isnan(exp[m_inf]).sum()), int((exp[m_inf] == float("inf")).sum()), int((exp[m_inf] == -float("inf")).sum()))))
    return failed


@pytest.mark.parametrize("kind", E.EDGE_KINDS)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_value_edges(env, family, kind):
    ran, failed, ways = 0, [], set()
    cases = E.edge_cases(family, kind)
    for kw, M, ovr, exp in cases:
        dl = G.get_layer(env, kw)
        plan = G.check_plan(env, dl, M, ovr, exp)
        if plan is None:
            continue
        ways.add(E.edge_way(family, kw["bits"], plan))
        failed += run_nonfinite(env, dl, M, ovr) if kind == "nonfinite" else run_range_edge(env, dl, kind, M, ovr)
        ran += 1
    print("family %d, %s: %d variants" % (family, kind, ran))
    assert ran == len(cases) or family == 6, (family, kind, ran, len(cases))      # (family 6 may refuse a split: exact_cases)
    E.assert_edge_coverage(family, kind, cases, ways)
    assert not failed, failed
