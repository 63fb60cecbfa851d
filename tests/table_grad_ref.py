"""fp64 reference of the lookup-table gradient (a test helper module, not a conftest):

    dT2[c, e] = sum over (kappa, n) with idx(kappa, n) = c of G[2 kappa + e, n] * S[n, 2 kappa / g]
    G[k, n]   = sum_m X[m, k] * dY[m, n],   idx(kappa, n) = code(2 kappa, n) << b | code(2 kappa + 1, n)

With the codes fixed this is the gradient of the loss sum(dY * (X @ W_hat^T)), W_hat[n, k] = L[k, n] * S[n, k / g],
with respect to the 4^b x 2 pair codebook L looks up (scale_grad_ref.lut_of_codes).  `to_scalar` is the adjoint of
make_qmap2_from_qmap: the gradient of a scalar table."""
import torch


def pair_index(codes, bits):
    """idx [K / 2, N] from integer codes [K, N]."""
    W = codes.long()
    return (W[0::2] << bits) | W[1::2]


def table_grad(dY, X, codes, S, bits, g, absolute=False):
    """dT2 [4^b, 2] in fp64 (absolute: the same sum over |dY| |X| |S|, the size a componentwise bound needs)."""
    dY, X, S = dY.double(), X.double(), S.double()
    if absolute:
        dY, X, S = dY.abs(), X.abs(), S.abs()
    V = (X.T @ dY) * S.repeat_interleave(g, dim=1).T              # [K, N]: G[k, n] S[n, k / g]
    idx = pair_index(codes.to(V.device), bits).reshape(-1)
    out = torch.zeros(4 ** bits, 2, dtype=torch.float64, device=V.device)
    for e in range(2):
        out[:, e].index_add_(0, idx, V[e::2].reshape(-1))
    return out


def to_scalar(dT2, bits):
    """dtable[i] = sum_j dT2[i 2^b + j, 0] + sum_j dT2[j 2^b + i, 1]."""
    n = 2 ** bits
    d = dT2.reshape(n, n, 2)
    return d[:, :, 0].sum(1) + d[:, :, 1].sum(0)


def chain_depth(M):
    """The most fp32 roundings one term passes through in param_grad.hip (derived in its header): the mainloop's 32
    per 32-row step, the product with the scale, a wave's 2048 elements of one pair half, 8 waves, the rounding of
    the fp64 total over workgroups."""
    return 32 * -(-M // 32) + 1 + 2048 + 8 + 1
