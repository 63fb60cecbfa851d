"""Record the reference's learnable-scale gradient (run where the reference checkout exists):

    python tests/golden/make_scale_grad_golden.py

The reference learns scales on a dense layer: every forward rebuilds W_hat = manual_nf4(W, absmax, values, pivots)
= values[searchsorted(pivots, W / absmax)] * absmax and torch differentiates that with respect to absmax.  This
records, in float64 on the CPU: the dense W's codes, X and dY of a layer Y = X @ W_hat^T, the NF4 values and
pivots, absmax and the absmax gradient of sum(dY * Y).  tests/test_scale_grad_host.py checks the suite's fp64
formula against it; tests/test_scale_grad_gpu.py checks the kernel."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _load_reference import REF, load_reference  # noqa: E402


def main():
    load_reference()
    spec = importlib.util.spec_from_file_location("flute.nf_utils", os.path.join(REF, "flute", "nf_utils.py"))
    nf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(nf)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flute_amd.nf_utils import NF4_VALUES

    gen = torch.Generator().manual_seed(2024)
    M, N, K, g = 4, 128, 128, 64
    values = torch.tensor(NF4_VALUES, dtype=torch.float64)
    pivots = (values[1:] + values[:-1]) / 2
    W = torch.randn(N, K, generator=gen, dtype=torch.float64)
    absmax = W.reshape(-1, g).abs().max(dim=1, keepdim=True).values.requires_grad_()
    X = torch.randint(-4, 5, (M, K), generator=gen).double() / 4        # exact in fp16 and bf16
    dY = torch.randint(-4, 5, (M, N), generator=gen).double() / 4
    dqx, idx, _ = nf.manual_nf4(W, absmax=absmax, bits=4, blocksize=g, return_stats=True, values=values, pivots=pivots)
    ((X @ dqx.T) * dY).sum().backward()
    np.savez_compressed(
        os.path.join(HERE, "scale_grad", "manual_nf4_absmax_grad.npz"),
        codes=idx.reshape(N, K).numpy().astype(np.uint8), X=X.numpy(), dY=dY.numpy(),
        values=values.numpy(), pivots=pivots.numpy(), absmax=absmax.detach().reshape(N, K // g).numpy(),
        grad=absmax.grad.reshape(N, K // g).numpy(), group_size=np.int64(g))


if __name__ == "__main__":
    main()
