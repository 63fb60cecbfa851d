"""What the host and the GPU tests of the router's auxiliary losses share (flute_moe_aux_loss, flute_moe_aux_loss_grad,
moe_aux.hip): the definitions of include/flute_amd.h restated with torch ops in any float type, the gradient formula, fp64
autograd of the definitions, the fp32 torch chain a user would write (Hugging Face's load_balancing_loss_func restated, plus
the z-loss), the shapes and draws, the derived bounds, and the direct ABI calls with canary-padded outputs.

The bounds count roundings, gamma_n = n u / (1 - n u), u = 2^-24.  Every summand of the forward is non-negative, so they hold for
any order of fp32 additions:
    |importance_e - ref| <= gamma_(T + E + 8) ref_e
    |balance - ref|      <= gamma_(T + 2 E + 12) ref
    |z - ref|            <= 2 gamma_(T + E + 16) mean_t (|m_t| + log S_t)^2
    |d_logits - ref|     <= (1 + u_T) gamma_(E + 16) core + u_T |ref| + floor,
        core = p_te (|a_e| + sum_j |a_j| p_tj) + |g_z| (2 / T) (|m_t| + log S_t) sm_te,
        u_T = 2^-11 / 2^-8 / 2^-24 for fp16 / bf16 / fp32 logits, floor = 2^-25 for fp16 (half its subnormal spacing), else 0.
They do not count the conditioning of exp: the rounding of x - m puts up to u |x_e - m| of relative error into u_e.  Where T is
large that is averaged under gamma_(T + ...); the two shapes with T <= 5 and E = 8 - whose bounds are 17 u to 24 u - cannot absorb
|x - m| of 30 and more, so they draw a spread of 1 and 4, the others up to 10 (SHAPES' fourth entry)."""
import torch

from tests import exact_cases as XC
from tests.moe_cases import CANARY, DTYPE_CODE, F32, I32, SCORING_CODE, canary_padded, intact  # noqa: F401
from tests.moe_wide_cases import header_constant, poisoned_workspace

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16, F32]
SCORINGS = ["softmax", "sigmoid"]
U = 2.0 ** -24
UNIT = {F16: 2.0 ** -11, BF16: 2.0 ** -8, F32: 2.0 ** -24}
FLOOR = {F16: 2.0 ** -25, BF16: 0.0, F32: 0.0}

# (T, E, k, spread of the logits, forced chunk_tokens): the five NV classes (E <= 64 / 128 / 256 / 512 / 1024), E no multiple of 64,
# fewer tokens than waves, T one past a chunk edge (257 = 8 * 32 + 1, 513 = 16 * 32 + 1).  The forced chunk gives three chunks and
# a ragged last one wherever T admits three (T = 1 has one chunk whatever it is)
SHAPES = [(1, 8, 2, 1.0, 1), (5, 8, 2, 4.0, 2), (257, 64, 2, 10.0, 100), (300, 160, 6, 2.5, 128), (513, 256, 8, 10.0, 200),
          (130, 1000, 8, 7.5, 48)]
SHAPE_IDS = ["T%d_E%d_k%d" % s[:3] for s in SHAPES]


def auto_chunk(T):
    """flute_amd.h's automatic chunk_tokens, restated from its constants."""
    return max(header_constant("FLUTE_MOE_AUX_CHUNK_TOKENS"), -(-T // header_constant("FLUTE_MOE_AUX_AUTO_CHUNKS")))


def workspace_bytes(T, E, chunk_tokens):
    """C (2 E + 1) words: psum [C][E], pcnt [C][E], pz [C]."""
    ct = chunk_tokens or auto_chunk(T)
    return -(-T // ct) * (2 * E + 1) * 4


# ---- the definitions ---------------------------------------------------------------------------------------------------

def token_terms(logits, scoring, ftype=torch.float64):
    """Per token, in `ftype`: p [T, E], s [T, E] (the sigmoids; None for softmax), Z [T, 1] (what s is divided by), sm [T, E] (the
    softmax), m [T, 1], logS [T, 1]; lse = m + logS."""
    x = logits.to(ftype)
    m = x.max(dim=1, keepdim=True).values
    u = torch.exp(x - m)
    S = u.sum(dim=1, keepdim=True)
    sm = u / S
    if scoring == "softmax":
        return sm, None, None, sm, m, torch.log(S)
    s = 1 / (1 + torch.exp(-x))
    Z = s.sum(dim=1, keepdim=True)
    return s / Z, s, Z, sm, m, torch.log(S)


def load_of(ids, E):
    """The slots that name each expert; an id outside [0, E) counts nowhere.  int64 [E]."""
    flat = ids.reshape(-1).long()
    return torch.bincount(flat[(flat >= 0) & (flat < E)], minlength=E)


def aux_forward(logits, ids, scoring, ftype=torch.float64):
    """(balance, z, load, importance) by the header's definitions in `ftype` (load: int64)."""
    T, E = logits.shape
    p, _, _, _, m, logS = token_terms(logits, scoring, ftype)
    load = load_of(ids, E).to(logits.device)
    importance = p.sum(dim=0)
    balance = E * ((load.to(ftype) / T) * (importance / T)).sum()
    z = ((m + logS) ** 2).sum() / T
    return balance, z, load, importance


def aux_grad_formula(logits, load, g_b, g_z, scoring, ftype=torch.float64):
    """d_logits of flute_moe_aux_loss_grad, the header's two lines, in `ftype`."""
    T, E = logits.shape
    p, s, Z, sm, m, logS = token_terms(logits, scoring, ftype)
    a = g_b * E * load.to(ftype) / (T * T)
    D = (a * p).sum(dim=1, keepdim=True)
    zc = g_z * (2.0 / T) * (m + logS)
    if scoring == "softmax":
        return p * (a - D) + zc * p
    return s * (1 - s) * (a - D) / Z + zc * sm


def aux_autograd(logits, ids, g_b, g_z, scoring, ftype=torch.float64):
    """torch.autograd.grad of the definitions in `ftype`, load held constant."""
    x = logits.detach().to(ftype).requires_grad_(True)
    balance, z, _, _ = aux_forward(x, ids, scoring, ftype)
    (dx,) = torch.autograd.grad(g_b * balance + g_z * z, x)
    return dx


def torch_chain(logits, ids, scoring):
    """What a user writes today, in fp32: Hugging Face's load_balancing_loss_func without an attention mask, restated (the
    [T, k, E] int64 one-hot included; the ids are inside [0, E)), on the given picks, and the z-loss.  (balance, z), differentiable."""
    E = logits.shape[1]
    x = logits.float()
    if scoring == "softmax":
        routing = torch.softmax(x, dim=-1)
    else:
        s = torch.sigmoid(x)
        routing = s / s.sum(dim=-1, keepdim=True)
    expert_mask = torch.nn.functional.one_hot(ids.long(), E)
    tokens_per_expert = expert_mask.float().mean(dim=0)
    router_prob = routing.mean(dim=0)
    balance = (tokens_per_expert * router_prob.unsqueeze(0)).sum() * E
    z = torch.logsumexp(x, dim=-1).square().mean()
    return balance, z


# ---- the draws ---------------------------------------------------------------------------------------------------------

def draw(T, E, k, spread, dtype, seed):
    """(logits [T, E] in dtype, ids [T, k] int32: k different experts per token, as a gate picks them)."""
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, E, generator=gen) * spread).to(dtype)
    ids = torch.stack([torch.randperm(E, generator=gen)[:k] for _ in range(T)]).to(torch.int32)
    return logits, ids


def draw_grads(seed):
    """(g_b, g_z) of order one, either sign."""
    g = torch.randn(2, generator=torch.Generator().manual_seed(seed))
    return g + torch.sign(g) * 0.25


# ---- the bounds --------------------------------------------------------------------------------------------------------

def forward_bounds(logits, ids, scoring):
    """((balance, z, load, importance) in fp64, (bound of balance, of z, of importance [E]))."""
    T, E = logits.shape
    ref = aux_forward(logits, ids, scoring)
    _, _, _, _, m, logS = token_terms(logits, scoring)
    lse_abs = ((m.abs() + logS) ** 2).mean()
    return ref, (XC.gamma(T + 2 * E + 12) * ref[0], 2 * XC.gamma(T + E + 16) * lse_abs, XC.gamma(T + E + 8) * ref[3])


def backward_bound(logits, load, g_b, g_z, scoring):
    """(d_logits in fp64, the bound per element for a result in logits.dtype)."""
    T, E = logits.shape
    ref = aux_grad_formula(logits, load, g_b, g_z, scoring)
    p, _, _, sm, m, logS = token_terms(logits, scoring)
    a = (g_b * E * load.double() / (T * T)).abs()
    core = p * (a + (a * p).sum(dim=1, keepdim=True)) + abs(g_z) * (2.0 / T) * (m.abs() + logS) * sm
    ut = UNIT[logits.dtype]
    return ref, (1 + ut) * XC.gamma(E + 16) * core + ut * ref.abs() + FLOOR[logits.dtype]


def propagated_bound(d_logits_bound, d_logits_full, d_logits_out, hidden):
    """The block: router_weight.grad = d_logits^T hidden, torch's own F.linear backward on 16-bit operands with fp32 partial sums
    and one rounding to T.  The aux share of router_weight.grad is the difference of two such products - of `d_logits_full`, the
    gradient the logits get with the aux terms in the loss, and of `d_logits_out`, without - against (ref d_logits)^T hidden in fp64.
    Per element [e, j], where the aux share of d_logits is within `d_logits_bound` [T, E] of its reference and autograd's sum of the
    two shares costs one more rounding of the 16-bit type:
        sum_t (d_logits_bound + u_T |full| + floor)_te |h_tj|                           the operand's error, carried through
      + for each of the two products: gamma_T sum_t |d_te| |h_tj| + u_T |d^T h|_ej + floor      T fp32 additions, one rounding"""
    ut, floor = UNIT[hidden.dtype], FLOOR[hidden.dtype]
    h = hidden.double()
    bound = (d_logits_bound + ut * d_logits_full.double().abs() + floor).T @ h.abs()
    for dl in (d_logits_full.double(), d_logits_out.double()):
        bound = bound + XC.gamma(hidden.shape[0]) * (dl.abs().T @ h.abs()) + ut * (dl.T @ h).abs() + floor
    return bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound, an element with bound 0 counting 0 where it is exact and infinity where it is not."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    return float(ratio.max())


# ---- the direct calls ----------------------------------------------------------------------------------------------------

def aux_loss_abi(env, logits, ids, scoring, chunk_tokens=None, workspace=None):
    """flute_moe_aux_loss with every output in the middle of a larger buffer and the workspace poisoned:
    (balance, z, load, importance)."""
    d, lib = env.dev, env.lib
    (T, E), k = logits.shape, ids.shape[1]
    ct = 0 if chunk_tokens is None else chunk_tokens
    nbytes = lib.flute_moe_aux_loss_workspace(T, E, ct)
    assert nbytes == workspace_bytes(T, E, chunk_tokens)
    ws_buf, ws = poisoned_workspace(env, nbytes) if workspace is None else workspace
    assert ws.numel() * 4 >= nbytes
    bufs = dict(load=canary_padded(E, I32, d), importance=canary_padded(E, F32, d), losses=canary_padded(2, F32, d))
    for _, view in bufs.values():
        view.view(I32).fill_(0x7FC00000)                           # NaN bits: a word left unwritten shows
    with torch.cuda.device(d):
        rc = lib.flute_moe_aux_loss(DTYPE_CODE[logits.dtype], T, E, k, SCORING_CODE[scoring], ct, logits.data_ptr(), ids.data_ptr(),
                                    ws.data_ptr(), bufs["load"][1].data_ptr(), bufs["importance"][1].data_ptr(),
                                    bufs["losses"][1].data_ptr(), torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, n in (("load", E), ("importance", E), ("losses", 2)):
        assert intact(bufs[name][0], n), "canary around " + name
    assert intact(ws_buf, ws.numel()), "canary around the workspace"
    losses = bufs["losses"][1]
    return losses[0], losses[1], bufs["load"][1], bufs["importance"][1]


def aux_grad_abi(env, logits, load, grads, scoring):
    """flute_moe_aux_loss_grad with d_logits pre-filled with NaN bits in the middle of a larger buffer."""
    d, lib = env.dev, env.lib
    T, E = logits.shape
    words = T * E * logits.element_size() // 4
    assert words * 4 == T * E * logits.element_size()
    buf, view = canary_padded(words, logits.dtype, d)
    view.view(I32).fill_(-1)                                       # 0xFFFF / 0xFFFFFFFF: a NaN in every type
    with torch.cuda.device(d):
        rc = lib.flute_moe_aux_loss_grad(DTYPE_CODE[logits.dtype], T, E, SCORING_CODE[scoring], logits.data_ptr(), load.data_ptr(),
                                         grads.data_ptr(), view.data_ptr(), torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert intact(buf, words), "canary around d_logits"
    return view.view(T, E)
