"""flute_amd.moe_gate_limited / moe_gate_route_limited (moe_gate.hip), FluteExperts.forward_logits_limited and the group
arguments of FluteSparseMoeBlock on the GPU.

The yardstick is the contract in fp64 on the host (tests/moe_gate_limited_ref.py on tests/moe_gate_ref.py).

Choice.  `ids` value for value, three logit dtypes x both scorings x with and without the selection bias x both group scores,
every output of a direct call in a canary-padded buffer.  Keys that are the logits' own values (no bias; with "max" the group
keys too) are exact and even their ties have to come out as the reference's; wherever a key is a rounded score, or a sum of
two, the inputs are drawn until the fp64 keys satisfy the 2^-16 condition (moe_gate_limited_ref.separated_limited: the chosen
expert keys and the best allowed one left out; the chosen group keys and the best group left out).

Weights.  |w - w64| <= r |w64| element by element, r = four times the worst relative error of torch's own fp32 chain
(softmax / sigmoid, gather, sum, div) on the GPU on the same inputs and the same ids against the same fp64 values - measured
in the test, per scoring and renormalisation, not fixed here, and printed by the test (torch's chain / the kernel); no GPU run
has been recorded here yet.

Degenerate cases, the masking identity, equal bits and the module are described on the tests."""
import pytest
import torch

from tests import moe_gate_limited_ref as L
from tests import moe_gate_ref as R
from tests.moe_cases import (DTYPE_CODE, SCORING_CODE, canary_padded, draw_bias, draw_logits, gate_abi, host_route, intact,  # noqa: F401
                             native, same_bits, top3_case)
from tests.support import bits16, env  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
I32 = torch.int32
GROUP_SCORE_CODE = {"max": 0, "top2sum": 1}
GAP = 2.0 ** -16

# (T, E, k, n_group, topk_group)
SHAPES = [
    (1, 2, 1, 2, 1),            # the smallest: gs = 1, "max" only
    (1, 4, 2, 2, 1),            # the smallest top2sum, k = topk_group gs
    (4, 8, 2, 8, 3),            # gs = 1
    (5, 60, 4, 6, 2),           # E is not a multiple of 64
    (37, 64, 8, 4, 2),          # more tokens than the routed form has waves
    (3, 160, 6, 8, 3),          # DeepSeek-V2; gs = 20: experts 60 .. 79 sit in two registers
    (3, 256, 8, 8, 4),          # DeepSeek-V3
    (2, 1000, 16, 8, 2),        # gs = 125, sixteen values per lane, a tail past E
    (2, 1024, 64, 64, 4),       # both caps, k = every allowed expert
    (1030, 8, 2, 4, 2),         # the standalone grid: many workgroups, the last one not full
]


def group_scores(E, n_group):
    return ("max", "top2sum") if E // n_group >= 2 else ("max",)


# ---- inputs and calls --------------------------------------------------------------------------------------------------------

def draw_separated_limited(T, E, k, n_group, topk_group, dtype, scoring, bias, group_score, seed, exact_too=False):
    """Logits whose fp64 keys satisfy separated_limited in every token: tokens that fail are drawn again with the next seed."""
    x = draw_logits(T, E, dtype, seed)
    for attempt in range(1, 200):
        bad = ~L.separated_limited(x, k, n_group, topk_group, scoring, bias, group_score, GAP, exact_too)
        if not bool(bad.any()):
            return x
        x[bad] = draw_logits(T, E, dtype, seed + 7919 * attempt)[bad]
    raise AssertionError("no separated draw for %s" % ((T, E, k, n_group, topk_group, dtype, scoring, group_score),))


def limited_abi(env, logits, k, n_group, topk_group, scoring="softmax", renormalize=False, bias=None, scale=1.0,
                group_score="max", routed=False):
    """The direct call with every output in the middle of a larger buffer: (ids, weights) or, routed, also (offsets, rows,
    row_weight, pos, perm)."""
    d = env.dev
    T, E = logits.shape
    P = T * k
    sizes = dict(ids=P, weights=P)
    if routed:
        sizes.update(offsets=E + 1, perm=P, rows=P, row_weight=P, pos=P)
    bufs = {n: canary_padded(s, F32 if n in ("weights", "row_weight") else I32, d) for n, s in sizes.items()}
    head = (DTYPE_CODE[logits.dtype], T, E, k, n_group, topk_group, GROUP_SCORE_CODE[group_score], SCORING_CODE[scoring],
            int(renormalize), float(scale), logits.data_ptr(), None if bias is None else bias.data_ptr(),
            bufs["ids"][1].data_ptr(), bufs["weights"][1].data_ptr())
    lib = env.lib
    with torch.cuda.device(d):
        stream = torch.cuda.current_stream(d).cuda_stream
        if routed:
            rc = lib.flute_moe_gate_route_limited(
                *head, *(bufs[n][1].data_ptr() for n in ("offsets", "perm", "rows", "row_weight", "pos")), stream)
        else:
            rc = lib.flute_moe_gate_limited(*head, stream)
    assert rc == 0
    torch.cuda.synchronize()
    for n, s in sizes.items():
        assert intact(bufs[n][0], s), "canary around " + n
    out = {n: bufs[n][1] for n in sizes}
    ids, weights = out["ids"].view(T, k), out["weights"].view(T, k)
    if not routed:
        return ids, weights
    return ids, weights, out["offsets"], out["rows"], out["row_weight"], out["pos"].view(T, k), out["perm"]


def four_callers(env, xd, k, n_group, topk_group, scoring, bd, group_score):
    E = xd.shape[1]
    yield limited_abi(env, xd, k, n_group, topk_group, scoring, bias=bd, group_score=group_score)[0]
    yield limited_abi(env, xd, k, n_group, topk_group, scoring, bias=bd, group_score=group_score, routed=True)[0]
    yield env.fa.moe_gate_limited(xd, k, n_group, topk_group, scoring, bias=bd, group_score=group_score)[0]
    yield env.fa.moe_gate_route_limited(xd, k, n_group, topk_group, E, scoring, bias=bd, group_score=group_score)[0]


# ---- 1. the choice, value for value ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16, F32])
@pytest.mark.parametrize("T,E,k,n_group,topk_group", SHAPES)
def test_ids_equal_the_reference(env, T, E, k, n_group, topk_group, dtype):
    d = env.dev
    gs = E // n_group
    for scoring in ("softmax", "sigmoid"):
        for with_bias in (False, True):
            for group_score in group_scores(E, n_group):
                seed = 100 * T + E + k + n_group
                bias = draw_bias(E, seed + 1) if with_bias else None
                x = draw_separated_limited(T, E, k, n_group, topk_group, dtype, scoring, bias, group_score, seed)
                want, _ = L.gate_limited(x, k, n_group, topk_group, scoring, bias=bias, group_score=group_score)
                allowed = L.allowed_mask(x, n_group, topk_group, scoring, bias, group_score)
                assert int(allowed.sum()) == T * topk_group * gs
                xd, bd = x.to(d), None if bias is None else bias.to(d)
                what = (T, E, k, n_group, topk_group, dtype, scoring, with_bias, group_score)
                for got in four_callers(env, xd, k, n_group, topk_group, scoring, bd, group_score):
                    assert got.dtype == I32 and got.shape == (T, k)
                    got = got.cpu().long()
                    assert torch.equal(got, want), what
                    assert bool(allowed.gather(1, got).all()), what               # every chosen id lies in an allowed group
                    assert all(len(set(row)) == k for row in got.tolist()), what  # and none repeats


# ---- 2. defined ties and edges: ids only -------------------------------------------------------------------------------------

def check_ids(env, x, k, n_group, topk_group, want=None, scorings=("softmax", "sigmoid"), bias=None, score_kinds=None):
    xd = x.to(env.dev)
    bd = None if bias is None else bias.to(env.dev)
    E = x.shape[1]
    for group_score in score_kinds or group_scores(E, n_group):
        for scoring in scorings:
            ref = L.gate_limited(x, k, n_group, topk_group, scoring, bias=bias, group_score=group_score)[0]
            if want is not None:
                assert ref.tolist() == want, ("the reference itself", scoring, group_score)
            for got in (limited_abi(env, xd, k, n_group, topk_group, scoring, bias=bd, group_score=group_score)[0],
                        env.fa.moe_gate_route_limited(xd, k, n_group, topk_group, None, scoring, bias=bd,
                                                      group_score=group_score)[0]):
                assert got.cpu().tolist() == ref.tolist(), (tuple(x.shape), k, n_group, topk_group, x.dtype, scoring, group_score)


def test_all_logits_equal_gives_the_first_groups_in_index_order(env):
    for dtype in (F16, F32):
        check_ids(env, torch.full((3, 160), 1.5, dtype=dtype), 6, 8, 3, [[0, 1, 2, 3, 4, 5]] * 3)
        check_ids(env, torch.full((2, 160), -7.0, dtype=dtype), 45, 8, 3, [list(range(45))] * 2)       # into the third group
        check_ids(env, torch.zeros(2, 1024, dtype=dtype), 64, 64, 4, [list(range(64))] * 2)
        check_ids(env, torch.zeros(1, 8, dtype=dtype), 3, 8, 3, [[0, 1, 2]])
    mixed = torch.zeros(1, 130)
    mixed[0, ::2] = -0.0                                                 # -0 equals +0, in the experts' and in the groups' keys
    check_ids(env, mixed, 6, 13, 2, [[0, 1, 2, 3, 4, 5]])


def test_groups_with_equal_keys_go_to_the_lower_group(env):
    x = draw_logits(4, 160, F32, 5, spread=0.5)                          # 8 groups of 20; groups 5 and 2 share the best key(s)
    x[:, 100] = x[:, 119] = x[:, 41] = x[:, 59] = 6.0                    # (small enough for a sigmoid to tell them apart)
    x[:, 70] = 5.0                                                       # group 3: the second best by max, by top2sum too
    x[:, 71] = 4.5
    check_ids(env, x, 2, 8, 1, [[41, 59]] * 4)                           # group 2 over group 5, whichever group score
    check_ids(env, x, 4, 8, 2, [[41, 59, 100, 119]] * 4)
    check_ids(env, x, 5, 8, 3, [[41, 59, 100, 119, 70]] * 4)
    y = draw_logits(2, 1000, F32, 6, spread=0.5)                         # gs = 125: group 7 (875 ..) and group 0 tie
    y[:, 999] = y[:, 875] = y[:, 124] = y[:, 0] = 6.0
    check_ids(env, y, 2, 8, 1, [[0, 124]] * 2)
    check_ids(env, y, 4, 8, 2, [[0, 124, 875, 999]] * 2)
    # one holder of the maximum is left out of the second maximum, not its equals: 7 + 7 beats 7 + 6.5
    z = torch.full((1, 8), -3.0)
    z[0, 0], z[0, 1], z[0, 4], z[0, 5] = 7.0, 6.5, 7.0, 7.0
    check_ids(env, z, 2, 2, 1, [[4, 5]], score_kinds=("top2sum",))
    check_ids(env, z, 2, 2, 1, [[0, 1]], score_kinds=("max",))           # by max the groups tie: the lower one


def test_a_nan_or_minus_infinity_group_ranks_last(env):
    inf, nan = float("inf"), float("nan")
    z = torch.tensor([[nan, nan, -inf, -inf, -5.0, -6.0, 9.0, nan]])
    check_ids(env, z, 2, 4, 3, [[6, 4]], score_kinds=("max",))
    check_ids(env, z, 6, 4, 3, [[6, 4, 5, 0, 1, 7]], score_kinds=("max",))           # groups 3, 2, then 0 before 1
    check_ids(env, z, 2, 4, 1, [[4, 5]], scorings=("sigmoid",), score_kinds=("top2sum",))   # 9 + NaN counts as -infinity
    check_ids(env, z.to(F16), 4, 4, 2, [[6, 4, 5, 7]], score_kinds=("max",))
    check_ids(env, torch.full((1, 12), -inf), 3, 6, 2, [[0, 1, 2]], score_kinds=("max",))
    check_ids(env, torch.full((1, 12), nan), 4, 6, 2, [[0, 1, 2, 3]])
    y = draw_logits(3, 160, F32, 9)
    y[:, 20:40] = nan                                                     # group 1 entirely NaN, group 4 entirely -inf
    y[:, 80:100] = -inf
    y[1, 60:80] = nan                                                     # a group across the register boundary
    ids = L.gate_limited(y, 6, 8, 3)[0]
    assert not any(20 <= e < 40 or 80 <= e < 100 for e in ids.reshape(-1).tolist())
    check_ids(env, y, 6, 8, 3)
    check_ids(env, y, 6, 8, 7, score_kinds=("max",))                      # NaN as -inf ties with -inf: the lower group, 1, is allowed
    assert bool(L.allowed_mask(y, 8, 7)[:, 20:40].all()) and not bool(L.allowed_mask(y, 8, 7)[:, 80:100].any())


def test_an_entirely_negative_row_and_a_negative_bias(env):
    """Negative keys lie below the 0 that marks "no expert here" in float order, not in key order: a maximum that started at a
    float 0, or the HF code's 0.0 fill of the groups left out, would pick wrong here."""
    for (T, E, k, n_group, topk_group) in ((3, 60, 4, 6, 2), (2, 160, 6, 8, 3), (3, 8, 2, 8, 3)):
        for dtype in (F16, F32):
            x = (-300.0 - torch.rand(T, E, generator=torch.Generator().manual_seed(E)) * 8).to(dtype)
            check_ids(env, x, k, n_group, topk_group, scorings=("sigmoid",), score_kinds=("max",))
        # moderately negative logits and a bias below -1: every key s + bias is negative
        bias = -1.0 - torch.rand(E, generator=torch.Generator().manual_seed(E + 1)) * 2
        for group_score in group_scores(E, n_group):
            x = draw_separated_limited(T, E, k, n_group, topk_group, F32, "sigmoid", bias, group_score, E + 2)
            x = -x.abs() - 1.0
            if not bool(L.separated_limited(x, k, n_group, topk_group, "sigmoid", bias, group_score, GAP).all()):
                continue
            assert bool((R.keys(x, "sigmoid", bias) < 0).all())
            check_ids(env, x, k, n_group, topk_group, scorings=("sigmoid",), bias=bias, score_kinds=(group_score,))


def test_an_allowed_expert_below_a_forbidden_one_is_still_chosen(env):
    x = torch.full((2, 64), -4.0)                                        # 4 groups of 16
    x[:, 5] = 10.0                                                       # group 0 wins on one expert; the rest of it is at -4
    x[:, 16:32] = 3.0                                                    # group 1: sixteen experts at 3, above group 0's -4
    x[:, 40] = 8.0                                                       # group 2: second by max
    check_ids(env, x, 3, 4, 1, [[5, 0, 1]] * 2, score_kinds=("max",))
    check_ids(env, x, 4, 4, 2, [[5, 40, 0, 1]] * 2, score_kinds=("max",))
    assert R.gate(x, 3)[0].tolist() == [[5, 40, 16]] * 2                 # the unlimited choice
    # by top2sum of sigmoids group 1 (two of 0.95) beats group 2 (1.00 + 0.02); of softmax scores e^8 beats 2 e^3
    check_ids(env, x, 3, 4, 2, [[5, 16, 17]] * 2, scorings=("sigmoid",), score_kinds=("top2sum",))
    check_ids(env, x, 3, 4, 2, [[5, 40, 0]] * 2, scorings=("softmax",), score_kinds=("top2sum",))
    # with a negative bias on everything the allowed keys are negative and the forbidden ones less so
    bias = torch.full((64,), -2.0)
    bias[16:32] = -1.0
    bias[5] = 0.5
    check_ids(env, x, 3, 4, 1, [[5, 0, 1]] * 2, scorings=("sigmoid",), bias=bias, score_kinds=("max",))


# ---- 3. every group allowed: bit for bit the unlimited kernels ---------------------------------------------------------------

@pytest.mark.parametrize("group_score", ["max", "top2sum"])
def test_every_group_allowed_is_moe_gate_bit_for_bit(env, group_score):
    d = env.dev
    for (T, E, k, n_group), dtype in (((37, 64, 8, 4), F16), ((3, 160, 6, 8), F32), ((2, 1000, 64, 8), BF16), ((5, 60, 4, 1), F32)):
        x = draw_logits(T, E, dtype, T + E).to(d)
        bias = draw_bias(E, 3).to(d)
        for scoring, renorm, b in (("softmax", True, None), ("softmax", False, bias), ("sigmoid", True, bias),
                                   ("sigmoid", False, None)):
            want = env.fa.moe_gate(x, k, scoring, renorm, b, 2.5)
            for got in (env.fa.moe_gate_limited(x, k, n_group, n_group, scoring, renorm, b, 2.5, group_score),
                        limited_abi(env, x, k, n_group, n_group, scoring, renorm, b, 2.5, group_score)):
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (T, E, k, n_group, scoring, renorm)
            want = env.fa.moe_gate_route(x, k, E, scoring, renorm, b, 2.5)
            for got in (env.fa.moe_gate_route_limited(x, k, n_group, n_group, E, scoring, renorm, b, 2.5, group_score),
                        limited_abi(env, x, k, n_group, n_group, scoring, renorm, b, 2.5, group_score, routed=True)):
                assert len(got) == len(want) == 7
                for i, (a, w) in enumerate(zip(got, want)):
                    assert same_bits(a, w), (T, E, k, n_group, scoring, renorm, i)


def test_no_tokens(env):
    d = env.dev
    x = torch.empty(0, 6, dtype=F16, device=d)
    ids, w = env.fa.moe_gate_limited(x, 2, 3, 1)
    assert ids.shape == (0, 2) and w.shape == (0, 2)
    out = env.fa.moe_gate_route_limited(x, 2, 3, 1, 6)
    assert out[2].tolist() == [0] * 7 and all(t.numel() == 0 for i, t in enumerate(out) if i != 2)
    assert limited_abi(env, x, 2, 3, 1, routed=True)[2].tolist() == [0] * 7         # the E + 1 zeros, nothing around them


# ---- 4. the masking identity -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,E,k,n_group,topk_group", [(1, 4, 2, 2, 1), (5, 60, 4, 6, 2), (3, 160, 6, 8, 3), (3, 256, 8, 8, 4),
                                                      (2, 1000, 16, 8, 2)])
def test_limited_is_moe_gate_with_minus_infinity_on_the_groups_left_out(env, T, E, k, n_group, topk_group):
    """For a sigmoid, moe_gate_limited(x, bias=b) = moe_gate(x, bias=b') in ids and weights, bit for bit, where b' is b (or
    zeros) with -infinity on the experts of the groups the reference did not choose - token by token, as the groups differ (a
    token's result depends neither on T nor on its row).  With and without renormalize, at any scale."""
    d = env.dev
    for dtype, with_bias, group_score in ((F32, True, "max"), (F16, False, "max"), (BF16, True, "top2sum"), (F32, False, "top2sum")):
        seed = 13 * T + E
        b = draw_bias(E, seed + 1) if with_bias else None
        zero_or_b = b if with_bias else torch.zeros(E)
        # separated with the keys moe_gate will see, s + b': without a bias they are the rounded s, not the logits
        x = draw_separated_limited(T, E, k, n_group, topk_group, dtype, "sigmoid", zero_or_b, group_score, seed, exact_too=True)
        allowed = L.allowed_mask(x, n_group, topk_group, "sigmoid", b, group_score)
        assert torch.equal(allowed, L.allowed_mask(x, n_group, topk_group, "sigmoid", zero_or_b, group_score))
        xd, bd = x.to(d), None if b is None else b.to(d)
        for renorm, scale in ((False, 1.0), (True, 2.5)):
            ids, w = env.fa.moe_gate_limited(xd, k, n_group, topk_group, "sigmoid", renorm, bd, scale, group_score)
            for t in range(T):
                masked = torch.where(allowed[t], zero_or_b, torch.full((E,), float("-inf"))).to(d)
                want = env.fa.moe_gate(xd[t:t + 1].contiguous(), k, "sigmoid", renorm, masked, scale)
                assert same_bits(ids[t:t + 1], want[0]) and same_bits(w[t:t + 1], want[1]), (T, E, dtype, group_score, renorm, t)


# ---- 5. the weights against fp64 ---------------------------------------------------------------------------------------------

WEIGHT_SHAPES = [(1, 4, 2, 2, 1), (5, 60, 4, 6, 2), (37, 64, 8, 4, 2), (3, 160, 6, 8, 3), (3, 256, 8, 8, 4), (2, 1000, 16, 8, 2),
                 (2, 1024, 64, 64, 4)]


@pytest.fixture(scope="module")
def weight_cases(env):
    """Every input of the weights test with its fp64 reference and the error of torch's own fp32 chain on the GPU, computed
    once: a list of dicts, and r[(scoring, renormalize)] = 4 x the worst relative error of the chain over all of them."""
    d = env.dev
    cases, worst = [], {}
    for T, E, k, n_group, topk_group in WEIGHT_SHAPES:
        for dtype in (F16, BF16, F32):
            for scoring in ("softmax", "sigmoid"):
                for with_bias, group_score in ((False, "max"), (True, "top2sum"), (False, "top2sum"), (True, "max")):
                    seed = 7 * T + E + k
                    bias = draw_bias(E, seed + 1) if with_bias else None
                    x = draw_separated_limited(T, E, k, n_group, topk_group, dtype, scoring, bias, group_score, seed)
                    if scoring == "softmax" and not with_bias and group_score == "max" and T > 1:
                        x[1::2] = (x[1::2].float() - 300.0).to(dtype)          # entirely negative rows (a sigmoid of -300 is 0)
                    xd = x.to(d)
                    for renorm in (False, True):
                        ids, w64 = L.gate_limited(x, k, n_group, topk_group, scoring, renorm, bias, 1.0, group_score)
                        xf = x.double()
                        if scoring == "softmax":                                # nothing chosen underflows
                            assert bool(((xf.gather(1, ids) - xf.max(1, keepdim=True).values) >= -20).all())
                        else:
                            assert bool((xf.gather(1, ids) >= -20).all())
                        s32 = torch.softmax(xd.float(), dim=1) if scoring == "softmax" else torch.sigmoid(xd.float())
                        w32 = s32.gather(1, ids.to(d))
                        if renorm:
                            w32 = w32 / w32.sum(dim=1, keepdim=True)
                        err = float(((w32.cpu().double() - w64).abs() / w64).max())
                        worst[(scoring, renorm)] = max(worst.get((scoring, renorm), 0.0), err)
                        cases.append(dict(shape=(T, E, k, n_group, topk_group), dtype=dtype, scoring=scoring, renorm=renorm, x=xd,
                                          ids=ids, w64=w64, group_score=group_score, bias=None if bias is None else bias.to(d)))
    return cases, {key: 4.0 * v for key, v in worst.items()}


def test_weights_against_fp64(env, weight_cases):
    cases, r = weight_cases
    kernel_worst = {}
    failures = []
    for c in cases:
        key = (c["scoring"], c["renorm"])
        T, E, k, n_group, topk_group = c["shape"]
        ids, w = env.fa.moe_gate_limited(c["x"], k, n_group, topk_group, c["scoring"], c["renorm"], c["bias"], 1.0, c["group_score"])
        what = (c["shape"], c["dtype"], c["scoring"], c["renorm"], c["bias"] is not None, c["group_score"])
        assert w.dtype == F32 and torch.equal(ids.cpu().long(), c["ids"]), what
        w_d = w.cpu().double()
        rel = (w_d - c["w64"]).abs() / c["w64"]
        kernel_worst[key] = max(kernel_worst.get(key, 0.0), float(rel.max()))
        if not bool((rel <= r[key]).all()):
            failures.append((what, float(rel.max()), r[key]))
        if c["renorm"]:
            off = float((w_d.sum(dim=1) - 1.0).abs().max())
            if not off <= k * r[key]:
                failures.append((what, "row sum", off, k * r[key]))
    for key in sorted(r):
        print("moe_gate_limited weights %s renormalize=%s: torch fp32 chain worst rel err %.3e (r = %.3e), kernel %.3e"
              % (key[0], key[1], r[key] / 4, r[key], kernel_worst[key]))
    assert all(v > 0 for v in r.values())
    assert not failures, failures


# ---- 6. equal bits -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scoring,renorm,with_bias,group_score", [("softmax", True, False, "top2sum"), ("softmax", False, True, "max"),
                                                                  ("sigmoid", True, True, "top2sum"), ("sigmoid", False, False, "max")])
def test_equal_bits(env, scoring, renorm, with_bias, group_score):
    d = env.dev
    # (5, 60, ...): E no multiple of 64, k = 4 <= 2 groups of 10; (3, 160, ...): groups of 20 straddle registers - with them the routed
    # entry point's group arguments are checked against moe_gate_limited + moe_route at topk_group < n_group for every form below
    for (T, E, k, n_group, topk_group), dtype in (((37, 64, 8, 4, 2), F16), ((37, 160, 6, 8, 3), F32), ((1030, 8, 2, 4, 2), BF16),
                                                  ((3, 1000, 16, 8, 2), F32), ((18, 256, 8, 8, 4), BF16), ((5, 60, 4, 6, 2), F16),
                                                  ((3, 160, 6, 8, 3), F16)):
        x = draw_logits(T, E, dtype, T + E).to(d)
        bias = draw_bias(E, 3).to(d) if with_bias else None
        args = (k, n_group, topk_group, scoring, renorm, bias, 1.5, group_score)
        ids, w = env.fa.moe_gate_limited(x, *args)
        again = env.fa.moe_gate_limited(x, *args)
        assert same_bits(ids, again[0]) and same_bits(w, again[1])                   # two calls
        assert bool(torch.isfinite(w).all())
        for row in sorted({0, 17 % T, T - 1}):                                       # a row alone = the row in its place
            alone = env.fa.moe_gate_limited(x[row:row + 1].contiguous(), *args)
            assert same_bits(alone[0], ids[row:row + 1]) and same_bits(alone[1], w[row:row + 1]), (T, E, k, row)
        for routed in (env.fa.moe_gate_route_limited(x, k, n_group, topk_group, E, scoring, renorm, bias, 1.5, group_score),
                       limited_abi(env, x, k, n_group, topk_group, scoring, renorm, bias, 1.5, group_score, routed=True)):
            rids, rw, offsets, rows, row_weight, pos, perm = routed
            assert same_bits(rids, ids) and same_bits(rw, w), (T, E, k, "the routed form's ids / weights are moe_gate_limited's")
            want = env.fa.moe_route(ids, w, E)                                       # (offsets, rows, row_weight, pos, perm)
            for name, a, b in zip(("offsets", "rows", "row_weight", "pos", "perm"), (offsets, rows, row_weight, pos, perm), want):
                assert same_bits(a, b), (T, E, k, name)
            h_off, h_perm, h_rows, h_pos = host_route(ids.reshape(-1).tolist(), k, E)
            assert offsets.tolist() == h_off and perm.tolist() == h_perm and rows.tolist() == h_rows
            assert pos.reshape(-1).tolist() == h_pos


# ---- 7. the module -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def router(env, top3_case):
    c = top3_case
    gen = torch.Generator().manual_seed(77)
    return (torch.randn(c["E"], c["K"], generator=gen) * 0.2).to(c["dtype"]).to(env.dev)


# E = 4 experts: two groups of two, the better one allowed, both of its experts taken
GATINGS = [dict(scoring="softmax", renormalize=True, bias=None, scale=1.0, group_score="max"),
           dict(scoring="sigmoid", renormalize=True, bias="draw", scale=2.5, group_score="top2sum")]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("native_routing", [True, False])
def test_forward_logits_limited_and_block_bit_for_bit(env, top3_case, router, fused, native_routing):
    """forward_logits_limited = forward(hidden, *moe_gate_limited(...)) and the block with n_group = 2 = forward_logits_limited
    on F.linear's output, bit for bit.  Top-2 (k = topk_group gs): also the only k at which the order of index_add_'s
    additions, and so the bits of the forward without native_routing, are defined."""
    c, moe = top3_case, env.moe
    experts = moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=fused, native_routing=native_routing)
    hidden, k, n_group, topk_group = c["hidden"], 2, 2, 1
    logits = torch.nn.functional.linear(hidden, router)
    for g in GATINGS:
        g = dict(g, bias=(draw_bias(c["E"], 5) * 0.25).to(env.dev) if g["bias"] is not None else None)   # small: both groups win somewhere
        ids, weights = env.fa.moe_gate_limited(logits, k, n_group, topk_group, g["scoring"], g["renormalize"], g["bias"],
                                               g["scale"], g["group_score"])
        assert bool(((ids // 2)[:, 0] == (ids // 2)[:, 1]).all())                    # both experts of one group
        assert len(set((ids // 2)[:, 0].tolist())) == 2                              # and both groups occur over the tokens
        want = experts(hidden, ids, weights)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        got = experts.forward_logits_limited(hidden, logits, k, n_group, topk_group, **g)
        assert got.shape == (c["T"], c["K"]) and got.dtype == c["dtype"]
        assert torch.equal(bits16(got), bits16(want)), (fused, native_routing, g["scoring"])
        block = moe.FluteSparseMoeBlock(router, experts, k, n_group=n_group, topk_group=topk_group, **g)
        assert torch.equal(bits16(block(hidden)), bits16(got)), (fused, native_routing, g["scoring"])
        unlimited = experts.forward_logits(hidden, logits, k, g["scoring"], g["renormalize"], g["bias"], g["scale"])
        assert not torch.equal(bits16(unlimited), bits16(got))                       # the limit changes the choice here


def test_limited_block_in_a_graph(env, top3_case, router):
    """The router GEMM, moe_gate_route_limited, the two fused launches and moe_combine captured once (capture raises if
    anything reads the routing on the host); a replay on other hidden states returns the bits of an eager call on them."""
    c = top3_case
    block = env.moe.FluteSparseMoeBlock(router, native(env, c, True), 2, scoring="sigmoid", renormalize=True,
                                        bias=draw_bias(c["E"], 5).to(env.dev), scale=2.5, n_group=2, topk_group=1,
                                        group_score="top2sum")
    hidden = c["hidden"].clone()
    first = block(hidden).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = block(hidden)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits16(y), bits16(first))
    other = (c["hidden"].flip(0) * 1.5).contiguous()
    hidden.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = block(other)
    assert torch.equal(bits16(y), bits16(eager))
    assert not torch.equal(bits16(eager), bits16(first))


@pytest.mark.parametrize("native_routing", [True, False])
def test_a_block_with_one_group_is_the_block_without(env, top3_case, router, native_routing):
    c, moe = top3_case, env.moe
    experts = moe.FluteExperts.from_linears(c["gates"], c["ups"], c["downs"], fused=True, native_routing=native_routing)
    k = c["k"] if native_routing else 2
    bias = draw_bias(c["E"], 5).to(env.dev)
    for g in (dict(renormalize=True), dict(scoring="sigmoid", bias=bias, scale=2.5)):
        want = moe.FluteSparseMoeBlock(router, experts, k, **g)(c["hidden"])
        for group_score in ("max", "top2sum"):
            one = moe.FluteSparseMoeBlock(router, experts, k, n_group=1, topk_group=1, group_score=group_score, **g)
            assert torch.equal(bits16(one(c["hidden"])), bits16(want))
        logits = torch.nn.functional.linear(c["hidden"], router)
        every = experts.forward_logits_limited(c["hidden"], logits, k, 2, 2, g.get("scoring", "softmax"), g.get("renormalize", False),
                                               g.get("bias"), g.get("scale", 1.0), "top2sum")
        assert torch.equal(bits16(every), bits16(want))                              # every group allowed: the same bits
