"""Time flute_amd.qgemm_table_grad (param_grad.hip): the table gradient alone, fused with the scale gradient, and the
two kernels it would otherwise take, against hipBLASLt.

    python tools/time_table_grad.py [--steps 3] [--out profiles/table_grad/time_table_grad.jsonl] [--only K,N]

One JSON line per case on stdout, appended to --out (--out '' for stdout only).  Every time is the median of 3 HBM-cold hipGraph
replays of `steps` launches, read from the chip-wide clock stamped inside the graph (bench.time_graph), all four in
one process:
  table_only_us  dT2 [2^b, 2^b, 2] of a K x N layer for dY [M, N] and X [M, K] (the main launch + the reduce pass);
  fused_us       the same launch also writing dS [N, K / 64];
  scale_grad_us  flute_amd.qgemm_scale_grad alone (param_grad.hip);
  mm_us          torch.mm(dY.t(), X) in the same dtype (hipBLASLt; the [N, K] product only).
Fusing pays where fused_us < scale_grad_us + table_only_us; table_vs_scale = table_only_us / scale_grad_us shows what the
binning epilogue costs over the scale epilogue, fused_vs_mm = fused_us / mm_us what both gradients cost over the bare GEMM."""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "table_grad",
                                                "time_table_grad.jsonl"),
                help="appended to; '' for stdout only")
ap.add_argument("--only", default=None, help="K,N: one layer shape only")
a = ap.parse_args()
d = torch.device("cuda:0")
num_sms = utils.get_device_num_sms(d)
G_SIZE = 64
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)


class Step:
    def __init__(self, fn):
        self.step = lambda i: fn()


def timed(fn):
    return sorted(bench.time_graph(Step(fn), a.steps, 2, torch.cuda.synchronize)[0] for _ in range(3))[1] / a.steps * 1e3


SHAPES = ((4096, 4096), (4096, 11008), (8192, 8192), (8192, 28672))
if a.only:
    SHAPES = (tuple(int(v) for v in a.only.split(",")),)
CASES = []
for K, N in SHAPES:
    for M in (512, 2048, 4096, 8192):
        CASES += [(4, K, N, M, torch.float16), (4, K, N, M, torch.bfloat16), (3, K, N, M, torch.bfloat16)]

with (open(a.out, "a") if a.out else contextlib.nullcontext()) as f:
    def emit(rec):
        print(json.dumps(rec), flush=True)
        if f is not None:
            f.write(json.dumps(rec) + "\n")

    for bits, K, N, M, dtype in CASES:
        if bits == 3 and N % 512:
            N = N // 512 * 512                                                           # 3 bits pack 512 columns
        tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)
        Q = torch.randint(-32768, 32767, (bits * N // 16, K), dtype=torch.int16, device=d)   # any bits are valid codes
        table = torch.linspace(-1, 1, 2 ** bits).to(dtype).to(d)
        T2 = utils.make_qmap2_from_qmap(table)
        S = (torch.rand(N, K // G_SIZE, device=d) / 16 + 1 / 32).to(dtype)
        X = (torch.randn(M, K, device=d) / 4).to(dtype)
        dY = (torch.randn(M, N, device=d) / 4).to(dtype)

        t_tab = timed(lambda: flute_amd.qgemm_table_grad(dY, X, Q, S, bits, G_SIZE, tid, num_sms))
        t_fus = timed(lambda: flute_amd.qgemm_table_grad(dY, X, Q, S, bits, G_SIZE, tid, num_sms, table2=T2,
                                                         with_scale_grad=True))
        t_sg = timed(lambda: flute_amd.qgemm_scale_grad(dY, X, Q, T2, bits, G_SIZE, tid, num_sms))
        t_mm = timed(lambda: torch.mm(dY.t(), X))
        emit({"bits": bits, "K": K, "N": N, "M": M, "dtype": str(dtype)[6:],
              "table_only_us": round(t_tab, 1), "fused_us": round(t_fus, 1), "scale_grad_us": round(t_sg, 1),
              "mm_us": round(t_mm, 1), "fusing_pays": bool(t_fus < t_sg + t_tab), "table_le_fused": bool(t_tab <= t_fus),
              "table_vs_scale": round(t_tab / t_sg, 3), "fused_vs_mm": round(t_fus / t_mm, 3),
              "TFLOPs_fused": round(2.0 * M * N * K / t_fus / 1e6, 1), "clock": bench.LAST_TIMING.get("clock")})
        del Q, X, dY, S
        torch.cuda.empty_cache()
