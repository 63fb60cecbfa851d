"""Host time per call of the MoE ops behind ops._abi_call and of FluteExperts' forward, eager (no graph).

    python tools/host_time.py TREE OUT.json LABEL

TREE is the checkout whose `flute_amd` is imported (built), so that two commits can be timed alternately by one copy of this
file; LABEL names it in OUT.json (the path itself is not written).  Operands are small (8 experts, top-2, K = F = 512, 1 / 16 / 64 tokens) so that the launches queue faster than the
host issues them: wall time of 1000 back-to-back calls / 1000 is the host's cost per call, the queue drained after the clock
stops.  Median, minimum and maximum of 7 such thousands, after 300 calls of warm-up; one JSON line per (op, tokens)."""
import json
import sys
import time

sys.path.insert(0, sys.argv[1])
import torch  # noqa: E402
import flute_amd  # noqa: E402
from flute_amd.integrations import moe  # noqa: E402

assert flute_amd.__file__.startswith(sys.argv[1]), flute_amd.__file__
d = torch.device("cuda", 0)
E, TOPK, K, F, BITS, G = 8, 2, 512, 512, 4, 64
gen = torch.Generator(device=d).manual_seed(1)
tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == BITS and c["TileP"] == 32)


def grouped(Kin, N):
    m = moe.GroupedFluteLinear(E, Kin, N, BITS, G, tid, d, torch.float16)
    m.weight.copy_(torch.randint(-2 ** 15, 2 ** 15, tuple(m.weight.shape), dtype=torch.int16, device=d, generator=gen))
    m.scales.copy_((torch.rand(tuple(m.scales.shape), device=d, generator=gen) * 0.02 + 0.005).half())
    return m


experts = moe.FluteExperts(grouped(K, F), grouped(K, F), grouped(F, K), fused=True, native_routing=True)
rows = []
with torch.no_grad():
    for T in (1, 16, 64):
        hidden = torch.randn(T, K, device=d, generator=gen).half()
        logits = torch.randn(T, E, device=d, generator=gen).half()
        ids, weights = flute_amd.moe_gate(logits, TOPK, "softmax", True)
        offsets, r, rw, pos, _ = flute_amd.moe_route(ids, weights, E)
        y = torch.randn(T * TOPK, K, device=d, generator=gen).half()
        calls = {"moe_route": lambda: flute_amd.moe_route(ids, weights, E),
                 "moe_combine": lambda: flute_amd.moe_combine(y, pos, offsets),
                 "moe_gate_route": lambda: flute_amd.moe_gate_route(logits, TOPK, E, "softmax", True),
                 "moe_gather": lambda: flute_amd.moe_gather(hidden, r, offsets),
                 "experts.forward": lambda: experts(hidden, ids, weights),
                 "experts.forward_logits": lambda: experts.forward_logits(hidden, logits, TOPK, "softmax", True)}
        for name, call in calls.items():
            for _ in range(300):
                call()
            torch.cuda.synchronize()
            per = []
            for _ in range(7):
                t0 = time.perf_counter()
                for _ in range(1000):
                    call()
                t1 = time.perf_counter()          # the host's time to issue; the queue drains after
                torch.cuda.synchronize()
                per.append((t1 - t0) * 1e3)
            per.sort()
            rows.append(dict(op=name, tokens=T, host_us_median=round(per[3], 3), host_us_min=round(per[0], 3),
                             host_us_max=round(per[-1], 3)))
            print(json.dumps(rows[-1]), flush=True)
with open(sys.argv[2], "w") as f:
    json.dump({"tree": sys.argv[3], "device": torch.cuda.get_device_name(d), "rows": rows}, f, indent=1)
