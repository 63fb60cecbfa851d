"""The contract of flute_moe_gate (include/flute_amd.h) in fp64 on the host - the yardstick of tests/test_moe_gate_*.py.

The choice is a STABLE descending sort of the keys, so equal keys come out in ascending expert index; it is not
`torch.topk`, whose order among equal values is undefined.  A NaN key ranks as -infinity."""
import torch


def scores(logits, scoring):
    """s [T, E] fp64: the softmax over all experts, or the sigmoid, of the logits' exact values."""
    x = logits.detach().cpu().double()
    if scoring == "softmax":
        u = torch.exp(x - x.max(dim=1, keepdim=True).values)
        return u / u.sum(dim=1, keepdim=True)
    if scoring == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    raise ValueError(scoring)


def keys(logits, scoring, bias=None):
    """The selection keys [T, E] fp64: the logits themselves, or score + bias."""
    if bias is None:
        key = logits.detach().cpu().double()
    else:
        key = scores(logits, scoring) + bias.detach().cpu().double()
    return torch.where(torch.isnan(key), torch.full_like(key, float("-inf")), key)


def gate(logits, k, scoring="softmax", renormalize=False, bias=None, scale=1.0):
    """(ids [T, k] int64, weights [T, k] fp64)."""
    s = scores(logits, scoring)
    order = torch.sort(keys(logits, scoring, bias), dim=1, descending=True, stable=True).indices
    ids = order[:, :k].contiguous()
    w = s.gather(1, ids)
    if renormalize:
        w = w / w.sum(dim=1, keepdim=True)
    return ids, w * scale


def separated(key, k, gap=2.0 ** -16):
    """[T] bool: the chosen keys differ pairwise, and from the best key left out, by more than `gap` - no rounding of a
    key computed in fp32 can then change the choice or its order."""
    top = torch.sort(key, dim=1, descending=True, stable=True).values[:, :min(k + 1, key.shape[1])]
    if top.shape[1] < 2:
        return torch.ones(key.shape[0], dtype=torch.bool)
    return ((top[:, :-1] - top[:, 1:]) > gap).all(dim=1)
