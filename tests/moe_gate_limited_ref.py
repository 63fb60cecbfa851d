"""The contract of flute_moe_gate_limited (include/flute_amd.h) in fp64 on the host, on tests/moe_gate_ref.py's functions -
the yardstick of tests/test_moe_gate_limited_*.py.

Group g is the contiguous experts g gs .. (g + 1) gs - 1, gs = E / n_group.  Its key is the largest expert key ("max") or
the sum of the two largest c = score (+ bias), a NaN c as -infinity ("top2sum"); a NaN group key ranks as -infinity.  The
topk_group best groups - a STABLE descending sort, so equal keys go to the lower group - are allowed, and the choice is
moe_gate_ref's stable sort over the experts of those groups only: an expert outside is never chosen, whatever its key."""
import torch

from tests import moe_gate_ref as R

NEG_INF = float("-inf")


def _no_nan(t):
    return torch.where(torch.isnan(t), torch.full_like(t, NEG_INF), t)


def group_keys(logits, n_group, scoring="softmax", bias=None, group_score="max"):
    """[T, n_group] fp64."""
    T, E = logits.shape
    assert E % n_group == 0
    gs = E // n_group
    if group_score == "max":
        return R.keys(logits, scoring, bias).view(T, n_group, gs).max(dim=2).values
    if group_score == "top2sum":
        assert gs >= 2
        c = R.scores(logits, scoring)
        if bias is not None:
            c = c + bias.detach().cpu().double()
        top2 = torch.sort(_no_nan(c).view(T, n_group, gs), dim=2, descending=True, stable=True).values[:, :, :2]
        return _no_nan(top2[:, :, 0] + top2[:, :, 1])
    raise ValueError(group_score)


def chosen_groups(gkey, topk_group):
    """[T, topk_group] int64: the groups by descending key, equal keys in ascending group index."""
    return torch.sort(gkey, dim=1, descending=True, stable=True).indices[:, :topk_group]


def allowed_mask(logits, n_group, topk_group, scoring="softmax", bias=None, group_score="max"):
    """[T, E] bool: the experts of the chosen groups."""
    T, E = logits.shape
    gs = E // n_group
    groups = chosen_groups(group_keys(logits, n_group, scoring, bias, group_score), topk_group)
    by_group = torch.zeros(T, n_group, dtype=torch.bool)
    by_group.scatter_(1, groups, torch.ones_like(groups, dtype=torch.bool))
    return by_group.repeat_interleave(gs, dim=1)


def gate_limited(logits, k, n_group, topk_group, scoring="softmax", renormalize=False, bias=None, scale=1.0,
                 group_score="max"):
    """(ids [T, k] int64, weights [T, k] fp64)."""
    T, E = logits.shape
    gs = E // n_group
    assert E % n_group == 0 and 1 <= topk_group <= n_group and 1 <= k <= topk_group * gs
    s = R.scores(logits, scoring)
    key = R.keys(logits, scoring, bias)
    allowed = allowed_mask(logits, n_group, topk_group, scoring, bias, group_score)
    # a stable sort by (allowed first, then key descending): an expert outside the chosen groups comes behind every allowed one,
    # also behind an allowed -infinity
    by_key = torch.sort(key, dim=1, descending=True, stable=True).indices
    by_allowed = torch.sort((~allowed.gather(1, by_key)).to(torch.int8), dim=1, stable=True).indices
    ids = by_key.gather(1, by_allowed)[:, :k].contiguous()
    assert bool(allowed.gather(1, ids).all())
    w = s.gather(1, ids)
    if renormalize:
        w = w / w.sum(dim=1, keepdim=True)
    return ids, w * scale


def separated_limited(logits, k, n_group, topk_group, scoring="softmax", bias=None, group_score="max", gap=2.0 ** -16,
                      exact_too=True):
    """[T] bool: no rounding of an fp32 key can change the choice or its order.  The 2^-16 condition on (a) the chosen expert
    keys and the best ALLOWED one left out (k - 1 gaps when k == topk_group gs: nothing is left out), and (b) the chosen
    group keys and the best group left out (not needed when topk_group == n_group: every group is chosen, in any order).
    Without a bias the expert keys - and with "max" the group keys too - are the logits' own values: nothing is rounded, the
    kernel has to reproduce even their ties, and `exact_too=False` leaves the condition off those."""
    T, E = logits.shape
    key = R.keys(logits, scoring, bias)
    allowed = allowed_mask(logits, n_group, topk_group, scoring, bias, group_score)
    ok = torch.ones(T, dtype=torch.bool)
    if exact_too or bias is not None:
        masked = torch.where(allowed, key, torch.full_like(key, NEG_INF))
        n_allowed = topk_group * (E // n_group)
        top = torch.sort(masked, dim=1, descending=True, stable=True).values[:, :min(k + 1, n_allowed)]
        if top.shape[1] >= 2:
            ok &= ((top[:, :-1] - top[:, 1:]) > gap).all(dim=1)
    if topk_group < n_group and (exact_too or bias is not None or group_score != "max"):
        gkey = group_keys(logits, n_group, scoring, bias, group_score)
        ok &= R.separated(gkey, topk_group, gap)
    return ok
