"""Record the reference's lookup-table gradient (run where the reference checkout exists):

    python tests/golden/make_table_grad_golden.py

The twin of make_scale_grad_golden.py: the reference rebuilds W_hat = manual_nf4(W, absmax, values, pivots)
= values[searchsorted(pivots, W / absmax)] * absmax every forward; here `values` requires grad as well, and torch
differentiates sum(dY * (X @ W_hat^T)) with respect to both.  Recorded in float64 on the CPU: the dense W's codes, X
and dY, the NF4 values and pivots, absmax, and the gradients of values and absmax.  tests/test_table_grad_host.py
checks the suite's fp64 formula against it; tests/test_table_grad_gpu.py checks the kernel."""
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

    gen = torch.Generator().manual_seed(2025)
    M, N, K, g = 4, 128, 128, 64
    values = torch.tensor(NF4_VALUES, dtype=torch.float64)
    pivots = (values[1:] + values[:-1]) / 2
    values.requires_grad_()
    W = torch.randn(N, K, generator=gen, dtype=torch.float64)
    absmax = W.reshape(-1, g).abs().max(dim=1, keepdim=True).values.requires_grad_()
    X = torch.randint(-4, 5, (M, K), generator=gen).double() / 4        # exact in fp16 and bf16
    dY = torch.randint(-4, 5, (M, N), generator=gen).double() / 4
    dqx, idx, _ = nf.manual_nf4(W, absmax=absmax, bits=4, blocksize=g, return_stats=True, values=values, pivots=pivots)
    ((X @ dqx.T) * dY).sum().backward()
    os.makedirs(os.path.join(HERE, "table_grad"), exist_ok=True)
    np.savez_compressed(
        os.path.join(HERE, "table_grad", "manual_nf4_values_grad.npz"),
        codes=idx.reshape(N, K).numpy().astype(np.uint8), X=X.numpy(), dY=dY.numpy(),
        values=values.detach().numpy(), pivots=pivots.numpy(), absmax=absmax.detach().reshape(N, K // g).numpy(),
        values_grad=values.grad.numpy(), absmax_grad=absmax.grad.reshape(N, K // g).numpy(), group_size=np.int64(g))


if __name__ == "__main__":
    main()
