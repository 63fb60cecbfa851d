"""Time flute_dequantize (HBM-cold hipGraph replays, as tools/time_cases.py) and the qgemm input gradient it serves.

    python tools/time_dequant.py [--steps 10] [--out FILE.jsonl]

One JSON line per case on stdout (appended to --out when given).
  kind "dequant":  median of 3 HBM-cold replays of `steps` launches (the chip-wide clock stamped inside the graph,
                   bench.time_graph) writing the dense weight of a K x N layer; GB/s counts the packed weight and the scales
                   read plus the dense weight written.
  kind "backward": torch.autograd.grad of a qgemm output w.r.t. its [M, K] input (dequantize in K chunks + hipBLASLt),
                   against torch.mm with the weight already dense; eager, HIP events over `steps` calls after warm-up,
                   fp16 GEMMs with their default reduction settings (compute-bound: the weight chunks are beyond the caches)."""
import argparse
import contextlib
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import flute_amd  # noqa: E402
from flute_amd import _lib, utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
d = torch.device("cuda:0")
num_sms = utils.get_device_num_sms(d)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)


def layer(bits, K, N, dtype, g=64):
    tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)
    Q = torch.randint(-32768, 32767, (bits * N // 16, K), dtype=torch.int16, device=d)   # any bits are valid codes
    S = (torch.randn(N, K // g, device=d) / 16).to(dtype)
    table = torch.linspace(-1, 1, 2 ** bits).to(dtype).to(d)
    return tid, Q, S, table, utils.make_qmap2_from_qmap(table)


class Dequant:
    def __init__(self, bits, K, N, dtype):
        self.bits, self.K, self.N, self.dtype = bits, K, N, dtype
        self.tid, self.Q, self.S, _, self.T2 = layer(bits, K, N, dtype)
        self.W = torch.empty(N, K, dtype=dtype, device=d)

    def step(self, i):
        rc = _lib.get().flute_dequantize(0 if self.dtype == torch.float16 else 1, self.bits, 64, self.N, self.K, self.Q.shape[0],
                                         0, self.K, self.Q.data_ptr(), self.S.data_ptr(), self.T2.data_ptr(), self.W.data_ptr(),
                                         self.tid, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        return self.W


class Step:
    def __init__(self, fn):
        self.step = lambda i: fn()


with (open(a.out, "a") if a.out else contextlib.nullcontext()) as f:
    def emit(rec):
        print(json.dumps(rec), flush=True)
        if f is not None:
            f.write(json.dumps(rec) + "\n")

    for K, N in ((8192, 28672), (28672, 8192), (4096, 11008)):
        for bits in (4, 2):
            for dtype in (torch.float16, torch.bfloat16):
                lay = Dequant(bits, K, N, dtype)
                ms = sorted(bench.time_graph(lay, a.steps, 3, torch.cuda.synchronize)[0] for _ in range(3))[1]
                us = ms / a.steps * 1e3
                nbytes = bits * N // 16 * K * 2 + N * (K // 64) * 2 + N * K * 2
                emit({"kind": "dequant", "bits": bits, "K": K, "N": N, "dtype": str(dtype)[6:], "us": round(us, 2),
                      "GBps": round(nbytes / us / 1e3, 1), "clock": bench.LAST_TIMING.get("clock")})
                del lay
                torch.cuda.empty_cache()

    for K, N in ((4096, 11008), (8192, 28672)):
        tid, Q, S, table, T2 = layer(4, K, N, torch.float16)
        ws = utils.get_workspace_streamk(d)
        Wd = flute_amd.dequantize(Q, S, T2, 4, 64, tid)
        for M in (512, 4096):
            x = torch.randn(M, K, dtype=torch.float16, device=d).requires_grad_()
            dY = torch.randn(M, N, dtype=torch.float16, device=d)
            y = flute_amd.qgemm(x, Q, S, table, T2, ws, 4, 64, tid, num_sms)
            bwd = Step(lambda: torch.autograd.grad(y, x, dY, retain_graph=True)[0])
            mm = Step(lambda: torch.mm(dY, Wd))
            t_bwd = min(bench.time_eager(bwd, a.steps, 3) for _ in range(3)) / a.steps * 1e3
            t_mm = min(bench.time_eager(mm, a.steps, 3) for _ in range(3)) / a.steps * 1e3
            emit({"kind": "backward", "bits": 4, "K": K, "N": N, "M": M, "dtype": "float16", "us": round(t_bwd, 1),
                  "mm_us": round(t_mm, 1), "ratio": round(t_bwd / t_mm, 3),
                  "TFLOPs": round(2.0 * M * N * K / t_bwd / 1e6, 1)})
            del x, dY, y
        del Q, S, T2, Wd
        torch.cuda.empty_cache()
