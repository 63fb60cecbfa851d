"""fp64 reference of the scale gradient (a test helper module, not a conftest):

    dS[n, j] = sum_m sum_{k in [j g, (j + 1) g)} dY[m, n] * X[m, k] * L[k, n]

L[k, n] the value the forward multiplies by the scale.  With the codes fixed this is the gradient of the loss
sum(dY * (X @ W_hat^T)), W_hat[n, k] = L[k, n] * S[n, k / g], with respect to S (the reference's `absmax`
gradient through manual_nf4: the code index carries none)."""
import torch


def lut_of_codes(codes, pairs, bits):
    """L [K, N] fp64 from integer codes [K, N] and the 4^b x 2 pair codebook (row 2 kappa + e takes element e of
    pair W[2 kappa] << b | W[2 kappa + 1]), exactly as exact_cases.Layer.w_exact without the scale."""
    W = codes.long()
    K, N = W.shape
    idx = (W[0::2] << bits) | W[1::2]
    return pairs.to(W.device).double()[idx].permute(0, 2, 1).reshape(K, N)


def scale_grad(dY, X, L, g, absolute=False):
    """dS [N, K / g] in fp64 (absolute: the same sum over |dY| |X| |L|, the size a componentwise bound needs)."""
    dY, X, L = dY.double(), X.double(), L.double()
    if absolute:
        dY, X, L = dY.abs(), X.abs(), L.abs()
    G = dY.T @ X                                    # [N, K]
    N, K = G.shape
    return (G * L.T).reshape(N, K // g, g).sum(-1)
