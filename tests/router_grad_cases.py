"""What the host and the GPU tests of the router's backward share (flute_moe_weight_grad, flute_moe_gate_grad): the gate-gradient
formula of include/flute_amd.h restated with torch ops in any precision, fp64 autograd of the gate formula, the default backward's
torch chain, the draws and the weight gradient's bound."""
import torch

from tests import exact_cases as XC
from tests.grouped_cases import gate_formula

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def gate_grad_formula(logits, ids, q, scoring, renormalize, scale, ftype=torch.float64):
    """d_logits of flute_moe_gate_grad, line by line, in `ftype`: q [T, k] is the incoming gradient of every slot (d_weights plus
    what pos folds in).  A slot whose id is outside [0, E) is skipped in every sum; slots that name one expert add."""
    x = logits.to(ftype)
    T, E = x.shape
    s = torch.softmax(x, dim=1) if scoring == "softmax" else torch.sigmoid(x)
    valid = (ids >= 0) & (ids < E)
    at = ids.clamp(0, E - 1).long()
    zero = torch.zeros((), dtype=ftype, device=x.device)
    sj = torch.where(valid, s.gather(1, at), zero)
    qj = torch.where(valid, q.to(ftype), zero)
    if renormalize:
        S = sj.sum(dim=1, keepdim=True)
        B = (qj * (sj / S)).sum(dim=1, keepdim=True)
        ds = scale * (qj - B) / S
    else:
        ds = scale * qj
    ds = torch.where(valid, ds, zero)
    dse = torch.zeros_like(s).scatter_add_(1, at, ds)
    if scoring == "sigmoid":
        return dse * s * (1 - s)
    return s * (dse - (dse * s).sum(dim=1, keepdim=True))


def gate_autograd(logits, ids, q, scoring, renormalize, scale, ftype=torch.float64):
    """torch.autograd.grad of the documented gate formula (grouped_cases.gate_formula) in `ftype`; the ids are inside [0, E)."""
    x = logits.detach().to(ftype).requires_grad_(True)
    (dx,) = torch.autograd.grad(gate_formula(x, ids, scoring, renormalize, scale), x, q.to(ftype))
    return dx


def gate_torch_chain(logits, ids, q, scoring, renormalize, scale):
    """The default backward of the gating ops, restated: fp32 autograd of the formula, rounded to the logits' type."""
    return gate_autograd(logits, ids, q, scoring, renormalize, scale, torch.float32).to(logits.dtype)


def fold_pos(d_weights, d_row_weight, pos):
    """q = d_weights + d_row_weight[pos], an entry of pos outside [0, T k) adding nothing; fp32, one addition."""
    P = d_row_weight.shape[0]
    inside = (pos >= 0) & (pos < P)
    add = torch.where(inside, d_row_weight[pos.clamp(0, P - 1).long()], torch.zeros((), device=pos.device))
    return add if d_weights is None else d_weights + add


def limited_groups(E, k):
    """(n_group, topk_group) of the group-limited draws: four groups, as few of them allowed as k admits (two at least)."""
    gs = E // 4
    return 4, max(2, -(-k // gs))


# ---- the weight gradient ---------------------------------------------------------------------------------------------

def weight_grad_bound(dhp, h):
    """(the fp64 row sums of the exact products, gamma_(K-1) * sum_k |dHp H|): the bound of any order of fp32 additions."""
    prod = dhp.double() * h.double()
    return prod.sum(dim=1), XC.gamma(dhp.shape[1] - 1) * prod.abs().sum(dim=1)


def draw_weight_operands(R, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    dhp = (torch.randn(R, K, generator=gen) / 4).to(dtype)
    h = torch.randn(R, K, generator=gen).to(dtype)
    rw = torch.rand(R, generator=gen) * 1.5 + 0.01
    return dhp, h, rw


def exact_weight_operands(R, K, dtype, seed):
    """Multiples of 1/8 in [-4, 4]: every product is a multiple of 1/64 of at most 16."""
    gen = torch.Generator().manual_seed(seed)
    draw = lambda: (torch.randint(-32, 33, (R, K), generator=gen).double() / 8).to(dtype)
    return draw(), draw()
