"""Time flute_amd.qgemm_scale_grad (param_grad.hip) against hipBLASLt and against the unfused composition.

    python tools/time_scale_grad.py [--steps 3] [--out FILE.jsonl]

One JSON line per case on stdout (appended to --out when given).  Every time is the median of 3 HBM-cold hipGraph
replays of `steps` launches, read from the chip-wide clock stamped inside the graph (bench.time_graph):
  us        the scale gradient dS [N, K / 64] of a K x N layer for dY [M, N] and X [M, K];
  mm_us     torch.mm(dY.t(), X) in the same dtype (hipBLASLt; the [N, K] product only, no lookup, no group sum);
  unfused_us what a user could compose without the kernel: dequantize with unit scales (the lookup L), hipBLASLt
            dY^T X with an fp32 result (aten mm.dtype), then (G * L) summed per group in torch - an N x K fp32
            intermediate in HBM.
TFLOPs = 2 M N K / us, pct_peak its share of 2.5 PF (MI355X dense fp16 / bf16)."""
import argparse
import contextlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import flute_amd  # noqa: E402
from flute_amd import utils  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
d = torch.device("cuda:0")
num_sms = utils.get_device_num_sms(d)
PEAK_TFLOPS = 2500.0
G_SIZE = 64
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)


class Step:
    def __init__(self, fn):
        self.step = lambda i: fn()


def timed(fn):
    return sorted(bench.time_graph(Step(fn), a.steps, 2, torch.cuda.synchronize)[0] for _ in range(3))[1] / a.steps * 1e3


CASES = []
for K, N in ((4096, 4096), (4096, 11008), (8192, 28672), (28672, 8192)):
    for M in (512, 2048, 8192):
        for dtype in (torch.float16, torch.bfloat16):
            CASES.append((4, K, N, M, dtype))
CASES += [(2, 8192, 28672, 2048, torch.bfloat16), (3, 8192, 28672, 2048, torch.float16)]

with (open(a.out, "a") if a.out else contextlib.nullcontext()) as f:
    def emit(rec):
        print(json.dumps(rec), flush=True)
        if f is not None:
            f.write(json.dumps(rec) + "\n")

    for bits, K, N, M, dtype in CASES:
        tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)
        Q = torch.randint(-32768, 32767, (bits * N // 16, K), dtype=torch.int16, device=d)   # any bits are valid codes
        table = torch.linspace(-1, 1, 2 ** bits).to(dtype).to(d)
        T2 = utils.make_qmap2_from_qmap(table)
        ones = torch.ones(N, K // G_SIZE, dtype=dtype, device=d)
        X = (torch.randn(M, K, device=d) / 4).to(dtype)
        dY = (torch.randn(M, N, device=d) / 4).to(dtype)

        t = timed(lambda: flute_amd.qgemm_scale_grad(dY, X, Q, T2, bits, G_SIZE, tid, num_sms))
        t_mm = timed(lambda: torch.mm(dY.t(), X))

        def unfused():
            L = flute_amd.dequantize(Q, ones, T2, bits, G_SIZE, tid)                   # [N, K]: the lookup alone
            G = torch.ops.aten.mm.dtype(dY.t(), X, torch.float32)                      # [N, K] fp32 in HBM
            return (G * L).view(N, K // G_SIZE, G_SIZE).sum(-1).to(dtype)
        t_un = timed(unfused)
        tf = 2.0 * M * N * K / t / 1e6
        emit({"bits": bits, "K": K, "N": N, "M": M, "dtype": str(dtype)[6:], "us": round(t, 1),
              "TFLOPs": round(tf, 1), "pct_peak": round(100 * tf / PEAK_TFLOPS, 1),
              "mm_us": round(t_mm, 1), "ratio_mm": round(t / t_mm, 3),
              "unfused_us": round(t_un, 1), "ratio_unfused": round(t / t_un, 3),
              "clock": bench.LAST_TIMING.get("clock")})
        del Q, X, dY, ones
        torch.cuda.empty_cache()
