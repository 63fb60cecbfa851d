"""CPU checks of tests/exact_cases.py: the generator keeps its premise, the fp64 reference is exact, the exact check and
the componentwise bound reject the errors kernels make, the forced-plan matrix plans to what it asks for.  No GPU."""
import torch

from tests import exact_cases as E
from tests.qgemm_cases import FAMILIES
from tests.support import first_template

NUM_SMS = 256


def _layers():
    seen = {}
    for fam, kw, M, ovr, exp in E.forced_matrix():
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        seen.setdefault(key, (kw, set()))[1].add(M)
    for kw, M in E.auto_grid():
        key = tuple(sorted((k, str(v)) for k, v in kw.items()))
        seen.setdefault(key, (kw, set()))[1].add(M)
    return list(seen.values())


def test_premise_holds_for_every_case():
    """Every layer of the forced matrix and the automatic grid, at its largest M: sum |x w| < 2^21, |exact| within fp16,
    weights and activations exact in T, the witness row needs an fp32 accumulator."""
    for kw, Ms in _layers():
        lay = E.Layer(kw["bits"], kw["K"], kw["N"], kw["g"], kw["dtype"], 1, kw["tile_p"], kw["pair"])
        assert kw["K"] * 64 < E.EXACT_SUM_LIMIT             # |x w| <= 64: exact for any codes and activations
        X = E.make_x(max(Ms), kw["K"], 2, kw["dtype"])
        if kw["K"] * kw["N"] <= (16 << 20):
            R, A = E.exact_product(X, lay, abs_too=True)
        else:                                                   # large layers: a column slice (the bound above covers the sum)
            lay.N = 1024
            R, A = E.exact_product(X, lay, abs_too=True)
        E.premise(X, lay, R, A)


def test_reference_equals_int64():
    for bits, dtype, pair in ((4, torch.float16, False), (2, torch.bfloat16, True), (3, torch.float16, False)):
        lay = E.Layer(bits, 1024, 512, 64, dtype, 3, 32, pair)
        X = E.make_x(13, 1024, 4, dtype)
        R = E.exact_product(X, lay)
        Wi = (lay.w_exact() * 8).round().long()
        assert torch.equal(Wi.double(), lay.w_exact() * 8)
        Ri = X.double().long() @ Wi
        assert torch.equal(R * 8, Ri.double())


def test_w_exact_equals_oracle_dequantize():
    from oracle import flute_oracle as O
    for bits, tile_p, g, dtype, pair in ((4, 32, 64, torch.float16, False), (4, 64, 128, torch.bfloat16, True),
                                         (2, 64, 32, torch.float16, False), (3, 32, 256, torch.bfloat16, False)):
        lay = E.Layer(bits, 512, E.cols_per_block(bits, tile_p) * 3, g, dtype, 5, tile_p, pair)
        Q = O.pack(lay.W.numpy(), bits, tile_p)
        Wh = O.dequantize(Q, lay.S, lay.table2, bits, g, tile_p)
        assert torch.equal(Wh.double(), lay.w_exact())


def _corruptions(X, lay, R):
    """Results a kernel bug would produce, each as the fp64 value before the output rounding (or the rounded result)."""
    T = lay.dtype
    D = R.to(T)
    W = lay.w_exact()
    out = {}
    bad = D.clone()
    v = bad[3, 5:6]
    bad[3, 5] = torch.nextafter(v.float(), torch.tensor([float("inf")])).to(T)[0] if T == torch.float16 else \
        torch.nextafter(v, torch.tensor([float("inf")], dtype=T))[0]
    if torch.equal(bad, D):                                     # (fp16 nextafter through fp32 can round back: step the bits)
        bad[3, 5] = (D[3, 5:6].view(torch.int16) + 1).view(T)[0]
    out["one ulp"] = bad
    j, k0 = 7, 128                                              # one 64-wide K group missing from one column of a 16-row tile
    R2 = R.clone()
    R2[:16, j] -= X.double()[:16, k0:k0 + 64] @ W[k0:k0 + 64, j]
    out["missing K group"] = R2.to(T)
    gi = k0 // lay.g                                            # the next group's scale on group gi of column j (same tile)
    lut = W[k0:k0 + lay.g, j] / lay.S64[j, gi]
    R3 = R.clone()
    R3[:16, j] += X.double()[:16, k0:k0 + lay.g] @ (lut * (lay.S64[j, gi + 1] - lay.S64[j, gi]))
    out["neighbouring scale"] = R3.to(T)
    D4 = D.clone()                                              # two columns swapped inside a 16-column tile
    D4[:16, [18, 19]] = D[:16, [19, 18]]
    out["swapped columns"] = D4
    R5 = R.clone()                                              # one K slice of a 16 x 16 tile added twice
    s0, s1 = lay.K // 4, lay.K // 2
    R5[16:32, 32:48] += X.double()[16:32, s0:s1] @ W[s0:s1, 32:48]
    out["split-K slice twice"] = R5.to(T)
    for name, bad in out.items():
        assert not torch.equal(bad.double(), D.double()), name
    return D, out


def test_checks_reject_kernel_bugs():
    """The exact check rejects all five corruptions; the componentwise bound rejects all but the one-ulp error; the suite's
    rel-Frobenius limits (1e-3 fp16, 4e-3 bf16) accept at least two of them."""
    accepted_by_rel = {}
    for dtype, tol in ((torch.float16, 1e-3), (torch.bfloat16, 4e-3)):
        lay = E.Layer(4, 8192, 1024, 64, dtype, 11)
        X = E.make_x(256, 8192, 12, dtype)
        R, A = E.exact_product(X, lay, abs_too=True)
        E.premise(X, lay, R, A)
        D, bad = _corruptions(X, lay, R)
        assert E.exact_equal(D, R, dtype) and E.componentwise_excess(D, R, A, lay.K, dtype) <= 0
        for name, B in bad.items():
            assert not E.exact_equal(B, R, dtype), (dtype, name)
            ex = E.componentwise_excess(B, R, A, lay.K, dtype)
            if name == "one ulp":
                assert ex <= 0, (dtype, name, ex)               # within the rounding the bound grants
            else:
                assert ex > 0, (dtype, name, ex)
            rel = ((B.double() - D.double()).norm() / D.double().norm()).item()
            if rel < tol:
                accepted_by_rel.setdefault(dtype, []).append(name)
    assert len(accepted_by_rel.get(torch.bfloat16, [])) >= 2, accepted_by_rel
    assert "one ulp" in accepted_by_rel.get(torch.float16, []), accepted_by_rel


def test_forced_matrix_plans_to_its_variants():
    """Host planner only: every forced case plans to the family and variant it asks for (family 7 falls back and family 8
    could clamp its overrides - the GPU test re-checks with the device's CU count)."""
    from flute_amd import dev
    fams, refused = {}, 0
    for fam, kw, M, ovr, exp in E.forced_matrix():
        try:
            plan = dev.get_plan(M, kw["N"], kw["K"], kw["bits"], kw["g"], first_template(kw["bits"], kw["tile_p"]), NUM_SMS,
                                kw["dtype"], dev.Overrides(**ovr))
        except RuntimeError:
            assert exp.get("may_refuse"), (fam, kw, M, ovr)
            refused += 1
            continue
        for k, v in exp.items():
            if k != "may_refuse":
                assert plan[k] in (v if isinstance(v, tuple) else (v,)), (kw, M, ovr, k, v, plan)
        fams[fam] = fams.get(fam, 0) + 1
    assert set(fams) == {0, 2, 3, 5, 6, 7, 8}, fams


def test_automatic_grid_reaches_every_family():
    from flute_amd import dev
    got = set()
    for kw, M in E.auto_grid():
        got.add(dev.get_plan(M, kw["N"], kw["K"], kw["bits"], kw["g"], first_template(kw["bits"], kw["tile_p"]), NUM_SMS,
                             kw["dtype"])["family"])
    assert got == E.AUTO_FAMILIES, got


def test_persistm_sets_override_that_cannot_apply_is_refused():
    """Family 8 with one set per workgroup on 28672 x 8192 at M = 4 would need 896 workgroups on 256 CUs: the override is
    refused (FLUTE_ERR_SHAPE), not silently replaced by four sets per workgroup."""
    import pytest
    from flute_amd import dev
    tid = first_template(4, 32)
    with pytest.raises(RuntimeError, match="Unsupported shape"):
        dev.get_plan(4, 28672, 8192, 4, 64, tid, NUM_SMS, torch.float16, dev.Overrides(family=8, m_tiles=1))
    p = dev.get_plan(4, 28672, 8192, 4, 64, tid, NUM_SMS, torch.float16, dev.Overrides(family=8, m_tiles=4))
    assert p["family"] == 8 and p["visits"] == 4 and p["grid"] <= NUM_SMS, p
    p = dev.get_plan(4, 28672, 8192, 4, 64, tid, NUM_SMS, torch.float16, dev.Overrides(family=8))
    assert p["family"] == 8 and p["grid"] <= NUM_SMS, p


# ---------------------------------------------------------------------------
# the fp16 range edges and non-finite rows (exact_cases.edge_cases, tests/test_value_edges_gpu.py)
# ---------------------------------------------------------------------------

def _edge_layers(kind):
    seen = {}
    for fam in FAMILIES:
        for kw, M, ovr, exp in E.edge_cases(fam, kind):
            seen.setdefault(E.layer_key(kw), (kw, set()))[1].add(M)
    return list(seen.values())


def test_edge_premises_hold():
    """Every layer of the three fp16 kinds, with the seeds the GPU test uses: operands representable, sums exact in fp32, at least
    half the weights and some outputs subnormal ("subw"), every activation subnormal ("subx"), +inf, -inf and a finite
    output above 2^15 ("overflow").  Wide layers: their first 1024 columns (the overflow rows are built from the first 256)."""
    for kind in ("subw", "subx", "overflow"):
        layers = _edge_layers(kind)
        assert layers
        for kw, Ms in layers:
            lay = E.make_layer(kw, E.seed_of(E.layer_key(kw)))
            for M in sorted(Ms):
                X = E.edge_x(kind, M, lay, E.seed_of(kind, M))
                full = lay.N
                lay.N = min(full, 1024)
                R, A = E.exact_product(X, lay, abs_too=True)
                lay.N = full
                E.premise_edge(kind, X, lay, R, A)
                if kind == "overflow":                      # the old premise but for the output range it leaves on purpose
                    assert kw["K"] * 64 < E.EXACT_SUM_LIMIT
                    assert float(R.abs().max()) > E.FP16_MAX


def test_edge_cases_plan_to_their_variants():
    """Host planner only: every edge case plans to the family and variant it asks for, and within a family every bit width
    and every way of combining K is there."""
    from flute_amd import dev
    for fam in FAMILIES:
        for kind in E.EDGE_KINDS:
            cases = E.edge_cases(fam, kind)
            assert cases, (fam, kind)
            ways = set()
            for kw, M, ovr, exp in cases:
                try:
                    plan = dev.get_plan(M, kw["N"], kw["K"], kw["bits"], kw["g"], first_template(kw["bits"], kw["tile_p"]), NUM_SMS,
                                        kw["dtype"], dev.Overrides(**ovr))
                except RuntimeError:
                    assert exp.get("may_refuse"), (fam, kind, kw, M, ovr)
                    continue
                for k, v in exp.items():
                    if k == "may_refuse":
                        continue
                    assert plan[k] in (v if isinstance(v, tuple) else (v,)), (kind, kw, M, ovr, k, v, plan)
                ways.add(E.edge_way(fam, kw["bits"], plan))
            E.assert_edge_coverage(fam, kind, cases, ways)


def test_edge_checks_reject_wrong_kernels():
    """Three wrong kernels, simulated in torch on the CPU, that the suite's operating region let through: one that reads fp16
    subnormal weights and activations as zero, one that saturates at 65504 where IEEE rounds to infinity, one that reads a
    NaN-carrying padded row of the weight (past K) and masks it by multiplying with a zero activation."""
    T = torch.float16
    kw = dict(bits=4, K=4096, N=512, g=64, dtype=T, tile_p=32, pair=False)
    for kind in ("subw", "subx"):
        lay = E.make_layer(dict(kw, **(E.SUBW if kind == "subw" else {})), 21)
        X = E.edge_x(kind, 5, lay, 22)
        R, A = E.exact_product(X, lay, abs_too=True)
        E.premise_edge(kind, X, lay, R, A)
        assert E.exact_equal(R.to(T), R, T)
        flushed = E.flush_subnormal_f16(X.double()) @ E.flush_subnormal_f16(lay.w_exact())
        assert not E.exact_equal(flushed.to(T), R, T), kind
        assert E.exact_equal(flushed.to(T), E.exact_product(X, lay, flush_w=True, flush_x=True), T)
    lay = E.make_layer(dict(kw, **E.OVERFLOW), 23)
    X = E.edge_x("overflow", 5, lay, 24)
    R, A = E.exact_product(X, lay, abs_too=True)
    E.premise_edge("overflow", X, lay, R, A)
    assert E.exact_equal(R.to(T), R, T)
    assert not E.exact_equal(R.clamp(-E.FP16_MAX, E.FP16_MAX).to(T), R, T)
    # the weight padded to the next multiple of 1024 rows with a neighbour's NaN, the activations padded with zeros
    lay = E.make_layer(dict(kw, K=3584), 25)
    X = E.make_x(5, lay.K, 26, T)
    R = E.exact_product(X, lay)
    Wp = torch.cat([lay.w_exact(), torch.full((512, lay.N), float("nan"), dtype=torch.float64)])
    Xp = torch.cat([X.double(), torch.zeros(5, 512, dtype=torch.float64)], 1)
    masked = (Xp[:, :, None] * Wp[None, :, :64]).sum(1)              # x * w term by term: 0 * NaN = NaN
    assert torch.isnan(masked).all() and not E.exact_equal(masked.to(T), R[:, :64], T)
    selected = (Xp[:, :lay.K, None] * Wp[None, :lay.K, :64]).sum(1)  # a predicate on k < K instead
    assert E.exact_equal(selected.to(T), R[:, :64], T)


def test_nonfinite_rule():
    """nonfinite_expected against IEEE arithmetic term by term on a small layer, and nonfinite_equal's NaN handling."""
    for T in (torch.float16, torch.bfloat16):
        lay = E.Layer(4, 256, 128, 64, T, 31, pair=True)
        X = E.make_x(4, 256, 32, T)
        clean = E.exact_product(X, lay).to(T)
        k_inf = next(k for k in range(256) if (lay.w_exact()[k] == 0).any() and (lay.w_exact()[k] > 0).any() and (lay.w_exact()[k] < 0).any())
        Xp = E.poison_x(X, 1, 2, 7, k_inf)
        ieee = (Xp.double()[:, :, None] * lay.w_exact()[None]).sum(1).to(T)
        exp = E.nonfinite_expected(clean, lay, 1, 2, k_inf)
        assert E.nonfinite_equal(ieee, exp)
        assert torch.isnan(exp[1]).all() and torch.isnan(exp[2]).any() and (exp[2] == float("inf")).any() and (exp[2] == -float("inf")).any()
        assert not E.nonfinite_equal(clean, exp)
        bad = exp.clone()
        bad[2] = float("nan")
        assert not E.nonfinite_equal(bad, exp)
