"""Grouped qgemm against the per-expert loop on Mixtral-8x7B-shaped experts, timed the way bench.py times the headline.

    python tools/grouped_bench.py [--bits 4] [--steps 20] [--warmup 5] [--replays 5] [--out profiles/grouped_moe.json]
    python tools/grouped_bench.py --mode mlp [--out profiles/grouped_moe_fused.json]
    python tools/grouped_bench.py --mode step [--processes 3] [--out profiles/grouped_moe_routing.json]
    python tools/grouped_bench.py --mode gate [--processes 3] [--out profiles/grouped_moe_gate.json]
    python tools/grouped_bench.py --mode gate_limited [--out profiles/grouped_moe_gate_limited.json]
    python tools/grouped_bench.py --mode input_grad [--only-swiglu-grad] [--out profiles/grouped_moe_input_grad_blocks.json]
    python tools/grouped_bench.py --mode scale_grad [--processes 3] [--out profiles/grouped_moe_scale_grad.json]
    python tools/grouped_bench.py --mode table_grad [--processes 3] [--out profiles/grouped_moe_table_grad.json]
    python tools/grouped_bench.py --mode prefill [--out profiles/grouped_moe_prefill.json]
    python tools/grouped_bench.py --mode router_grad [--out profiles/grouped_moe_router_grad.json]
    python tools/grouped_bench.py --mode route_wide [--out profiles/grouped_moe_route_wide.json]

W4G64 fp16, E = 8, gate / up 4096 -> 14336 and down 14336 -> 4096, top-2 routing of 1, 4, 16 and 64 tokens; the expert of
every (token, slot) is drawn once from a fixed seed.  Both forms are captured in a hipGraph of `steps` launches between
two device-clock stamps (bench.time_graph: rotating weight copies larger than the Infinity Cache, caches flushed before
every timed replay, warm-up, the median of `replays` replays), alternately in the same process:

  grouped   one flute_amd.qgemm_grouped launch per step, row offsets on the device
  loop      the code before the grouped kernel: one flute_amd.qgemm call per expert that has rows, each with the
            shipped table's template for its row count, over the same fixed counts - captured in a graph, which is its
            best case (eager it also needs the counts on the host, i.e. a device synchronise per step)

Per shape: microseconds per step of both, their ratio, the bytes the algorithm needs (packed weights and scales of the
routed experts, X and Y), the GB/s and the share of 8 TB/s that follow, and the spread of the replays.  --bits 2 / 3 times
the projection at that bit width (same group size and dtype); where the shipped table holds no template for one of the
loop's (row count, shape) pairs at that width, the grouped form is timed alone and the row says so.

--mode mlp times a whole expert MLP step at the same shapes, token counts and routing, from the gather of the hidden
states through the down projection's weighted output (everything of FluteExperts.forward between sort_by_expert and
index_add_), by the same method, both forms alternating in one process:

  unfused   hidden[token], three qgemm_grouped launches, silu, the product, the weight gather and cast, the scaling and
            where(served): FluteExperts.forward as it is without `fused`
  fused     qgemm_grouped_glu reading hidden through the routing index, then qgemm_grouped_weighted: two launches
            (and the cast of the index and the gather of the weights, which the fused forward also runs)

--mode step times the WHOLE FluteExperts(fused=True).forward - routing, the two fused launches, the sum per token - at the
same shapes and token counts, with `native_routing` off (sort_by_expert and its glue, zeros_like + index_add_: the default
forward) and on (moe_route, moe_combine), by the same method, the two forms alternating twice in one process, in
`--processes` fresh processes one after the other.  One more pair of rows leaves the GEMMs out: moe_route + moe_combine
against sort_by_expert, perm // k, the cast, the weight gather and zeros_like + index_add_ at E = 64, top-8, N = 2048.

--mode gate times the step from the router's logits, by --mode step's method.  Gating alone: the torch chain models run
today (Mixtral's softmax -> topk -> renormalise at E = 8, top-2 and E = 64, top-8; DeepSeek-V3's sigmoid -> + bias -> topk ->
gather -> renormalise -> scale at E = 256, top-8) followed by moe_route - the best the code before moe_gate offers - against
one moe_gate_route launch, fp16 logits.  The whole block: the router GEMM, that chain and
FluteExperts(fused=True, native_routing=True).forward against FluteSparseMoeBlock on the same experts, at --mode step's shape.

--mode gate_limited times the group-limited gating alone at DeepSeek-V3's shape (E = 256, top-8, 8 groups, the best 4 by the
top-2 sum, sigmoid + bias, renormalised, scale 2.5, fp16 logits) by --mode gate's method, in one process: moe_gate_limited,
moe_gate at the same (E, k) - the difference is the cost of the group stage - and the torch-op chain for the same selection
(view / topk / sum / topk / scatter / masked_fill / topk / gather / sum / div).

--mode input_grad times the grouped input gradient, dX = dY @ W_e per expert in one launch, at training-sized row counts: its
slab form (qgemm_grouped_input_grad.h), its block form (qgemm_grouped_input_grad_blocks.h), the automatic rule, and the only
alternative there was: a per-expert loop of flute_amd.dequantize + torch.mm with the row counts known on the host (its best
case).  W4G64 fp16 at Mixtral's two projections (E = 8, K = 4096, F = 14336) with 512, 4096 and 8192 routed rows and an E = 64
2048 x 2048 stack at 4096 rows, one bf16, one 2-bit and two pair-form lines.  Same method: a hipGraph of steps between
device-clock stamps, rotating copies of the stacks, cold caches, the median of five replays, two alternating passes of each
contender, one process.  Reported: the times, blocks / slabs, blocks / loop, the achieved FLOP/s against 2.5 PFLOP/s, the
spread.  Then the threshold sweep - rows / E in 16 .. 256 on two E = 8 stacks and an E = 64 stack, slabs against blocks, even
counts and a routed draw - and one whole backward step of FluteExperts(fused=True, native_routing=True) at 512 and 4096 tokens
with its two input-gradient launches (down's with the routing weight in its epilogue, the pair form over gate and up) on the
slab form and on the automatic rule.  (profiles/grouped_moe_input_grad.json is the slab form's earlier record: three processes,
grouped against loop, and the step split into its launches.)  Its last section, which `--only-swiglu-grad` runs alone, is the
same step with `native_glu_grad` off and on (BackwardStep(native=...)): the gather in front of the recompute and the part
`elementwise_dg_du` as torch op chains - the default backward's arithmetic - against flute_amd.moe_gather and flute_amd.swiglu_grad,
per part and for the whole step at 512 and 4096 tokens, next to one yardstick of the same run: a `copy_` of a 16-bit tensor of
2.5 R F elements, the 10 bytes per element of [R, F] that swiglu_grad moves.  It goes to profiles/grouped_moe_swiglu_grad.json.

--mode scale_grad times the grouped scale-gradient kernel (param_grad.hip), dS [E, N, K / g] of a stack in one launch,
by --mode input_grad's method at its six shape / row-count lines, against a per-expert loop of flute_amd.qgemm_scale_grad on
row ranges the host knows - the loop's best case: inside FluteExperts the counts are not on the host.  FLOP = 2 rows N K.

--mode table_grad times the grouped table-gradient launch pair (param_grad.hip: the main launch and its reduce), by
--mode scale_grad's method at the same six lines: dT2 alone, dT2 + dS in one launch pair ("fused"), `qgemm_grouped_scale_grad`
followed by the dT2-only pair ("separate": what the fused form replaces), and a per-expert loop of the dense
flute_amd.qgemm_table_grad (dT2 only) on row ranges the host knows.  Passes per process: table, fused, separate, loop, twice.

--mode router_grad times the router's backward at Mixtral's shapes, 512 and 4096 tokens, top-2, by --mode input_grad's method in one
process: the weighted launch's chain behind the unweighted input gradient (torch ops against flute_amd.moe_weight_grad, with a copy_
of 1.5 R K 16-bit elements as the yardstick of the same traffic), the gate's backward (torch ops against flute_amd.moe_gate_grad) for
an E = 8 top-2 softmax router and an E = 256 top-8 group-limited sigmoid router, moe_combine's backward (the torch chain against
flute_amd.moe_gather), and one whole backward step of FluteSparseMoeBlock with the router training, native_router_grad off and on.

--mode route_wide times the routing at prefill and training token counts - 16 .. 16384 tokens - for three routers (E = 8 top-2 softmax,
E = 64 top-8 softmax, E = 256 top-8 sigmoid + bias with 8 groups / best 4 / top-2 sum, scale 2.5; fp16 logits, renormalised), by
--mode gate_limited's method in one process, every contender timed twice, alternating: (a) moe_gate_route[_limited], one workgroup,
what the modules run by default; (b) moe_gate[_limited] then moe_route, the two-call sequence; (c) moe_gate_route_wide on its
automatic chunk; (d) ungated, moe_route against moe_route_wide on the ids and weights (a) wrote.  Then the chunk_tokens sweep at 1024
and 4096 tokens - 16 .. 256 tokens for (c), the tokens of 512 .. 4096 pairs for (d) - and one forward of
FluteSparseMoeBlock(fused=True, native_routing=True) at Mixtral's shapes, 512 and 4096 tokens, wide_routing off against "auto".
Every row carries each contender's own spread over its ten replays.

--mode aux_loss times the router's auxiliary losses (flute_amd.moe_aux_loss: load-balance loss, z-loss, load, importance; moe_aux.hip)
at 512, 4096 and 16384 tokens of bf16 logits for an E = 8 top-2 softmax router and an E = 256 top-8 sigmoid router, by --mode router_grad's
method in one process, contenders alternating: the forward alone and forward + backward to the logits, each against the torch fp32
chain of tests/moe_aux_cases.py (Hugging Face's load_balancing_loss_func restated, plus the z-loss), which runs no kernel of
moe_aux.hip; and one training step of FluteSparseMoeBlock at Mixtral's shapes, 512 and 4096 tokens, with aux_loss on against the
same step with the torch chain bolted on (the router GEMM and a top-k again, as a user without the block's ids writes it).

--mode prefill times the grouped FORWARD at prefill and training row counts, where the block form (qgemm_grouped_blocks.h) meets
the row form (qgemm_grouped.h): W4G64 fp16 at Mixtral's two projections with 512, 4096 and 8192 routed rows (the counts of
--mode projection at rows / 2 tokens, so its grouped figure from a build of the parent is the row form's here), the many-expert
pair of --mode input_grad (which the block form does not serve: 1408 columns, 22 scale groups) and an E = 64 2048 x 2048 stack
at 4096 rows, one bf16 and one 2-bit line, the weighted down projection, and the gate / up pair read through the routing index as
three GLU contenders - the fused launch on its row form (qgemm_grouped_glu), on its block form (qgemm_grouped_glu_blocks) and the
unfused sequence: gather, two plain launches on the automatic form, silu and the product - at Mixtral's pair with 512, 4096 and
8192 rows, an E = 64 2048 x 2048 pair, one bf16 and one 2-bit line; then the GLU threshold sweep (rows / E in 16 .. 128, row
form against block form, on two pairs that fill the chip and one that does not) and one forward and one forward + backward
step of FluteExperts(fused=True, native_routing=True) with glu_blocks False against "auto".  `--only` runs some of the sections
(profiles/grouped_moe_glu_blocks.json: --only glu glu_sweep glu_module).  Contenders, alternating in one process, each timed twice by the
tool's method: form="rows", form="blocks", the automatic rule, and a per-expert loop of flute_amd.qgemm on row ranges the host
knows (the stack's template; the planner picks each call's kernel).  Then the threshold sweep - rows / E in 16 .. 256 on two E = 8 stacks and
an E = 64 stack, rows against blocks - and the backward step of --mode input_grad at 512 and 4096 tokens with the recompute of
gate and up on the row form (the code before the block form) and on the automatic rule.
"""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

BITS, G, E, TOPK, DTYPE = 4, 64, 8, 2, torch.float16
PEAK = 8.0e12


def routing(tokens, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.rand(tokens, E, generator=gen).topk(TOPK, dim=1).indices
    return torch.bincount(ids.reshape(-1), minlength=E).tolist()


class Experts:
    """`copies` stacks of E packed layers [N, K]; step(i) runs one projection of all routed rows on copy i."""

    def __init__(self, N, K, counts, copies, device, grouped, bits=BITS, form=None):
        import flute_amd
        from flute_amd import tune, utils
        self.fa, self.N, self.K, self.counts, self.grouped, self.bits = flute_amd, N, K, counts, grouped, bits
        self.form = form
        self.num_sms = utils.get_device_num_sms(device)
        self.ws = utils.get_workspace_streamk(device)
        T = sum(counts)
        gen = torch.Generator(device=device).manual_seed(1)
        P = bits * N // 16
        self.Q = torch.randint(-2 ** 15, 2 ** 15, (copies, E, P, K), dtype=torch.int16, device=device, generator=gen)
        self.S = torch.randn(copies, E, N, K // G, device=device, generator=gen).to(DTYPE)
        self.table = torch.randn(2 ** bits, device=device, generator=gen).sort().values.to(DTYPE)
        self.table2 = utils.make_qmap2_from_qmap(self.table)
        self.tables2 = self.table2.repeat(E, 1, 1, 1)
        self.X = (torch.randn(T, K, device=device, generator=gen) / 100).to(DTYPE)
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        self.off_host = off
        self.offsets = torch.tensor(off, dtype=torch.int32, device=device)
        self.tid_grouped = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)
        # the loop's template per row count: the shipped table's (random bits are a valid packed matrix in either layout);
        # a shape the table does not hold is no on-device tuning run: LookupError, and the caller times the grouped form alone
        self.tid_loop = {}
        for m in (() if grouped else sorted(set(c for c in counts if c))):
            tid = tune.lookup_tuned(m, N, K, bits, G, self.num_sms, DTYPE)
            if tid is None:
                raise LookupError(f"no shipped template for M={m} N={N} K={K} W{bits}G{G} on {self.num_sms} CUs")
            self.tid_loop[m] = tid

    def step(self, i):
        c = i % self.Q.shape[0]
        if self.grouped:
            return self.fa.qgemm_grouped(self.X, self.offsets, self.Q[c], self.S[c], self.tables2, self.bits, G,
                                         self.tid_grouped, self.num_sms, form=self.form)
        # the per-expert outputs are kept as they come: no copy into one [T, N] tensor (the grouped form has none either)
        ys = []
        for e, m in enumerate(self.counts):
            if m:
                r0, r1 = self.off_host[e], self.off_host[e + 1]
                ys.append(self.fa.qgemm(self.X[r0:r1], self.Q[c, e], self.S[c, e], self.table, self.table2, self.ws,
                                        self.bits, G, self.tid_loop[m], self.num_sms))
        return ys

    def bytes(self):
        routed = sum(1 for c in self.counts if c)
        per_expert = (self.bits * self.N // 16) * self.K * 2 + self.N * (self.K // G) * 2
        return routed * per_expert + sum(self.counts) * (self.K + self.N) * 2


class Mlp:
    """`copies` sets of gate / up [F, K] and down [K, F] stacks; step(i) runs one MLP step of all routed rows on set i."""

    def __init__(self, counts, tokens, copies, device, fused):
        import flute_amd
        from flute_amd import utils
        self.fa, self.fused, self.counts = flute_amd, fused, counts
        self.num_sms = utils.get_device_num_sms(device)
        K, F = 4096, 14336
        self.K, self.F = K, F
        gen = torch.Generator(device=device).manual_seed(1)

        def stack(N, Kin):
            Q = torch.randint(-2 ** 15, 2 ** 15, (copies, E, BITS * N // 16, Kin), dtype=torch.int16, device=device, generator=gen)
            S = (torch.rand(copies, E, N, Kin // G, device=device, generator=gen) * 0.02 + 0.005).to(DTYPE)
            return Q, S
        self.gate, self.up, self.down = stack(F, K), stack(F, K), stack(K, F)
        table = torch.randn(2 ** BITS, device=device, generator=gen).sort().values.to(DTYPE)
        self.tables2 = utils.make_qmap2_from_qmap(table).repeat(E, 1, 1, 1)
        self.tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == BITS and c["TileP"] == 32)
        T = sum(counts)
        self.hidden = torch.randn(tokens, K, device=device, generator=gen).to(DTYPE)
        # what sort_by_expert hands the forward: the token of every sorted row, the sorted rows' weights' places, the offsets
        self.token = torch.randint(0, tokens, (T,), device=device, generator=gen)
        self.perm = torch.randperm(T, device=device, generator=gen)
        self.topk_weights = torch.rand(T, device=device, generator=gen).to(DTYPE)
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        self.offsets = torch.tensor(off, dtype=torch.int32, device=device)

    def step(self, i):
        c = i % self.gate[0].shape[0]
        fa, off, t2, a = self.fa, self.offsets, self.tables2, (BITS, G, self.tid, self.num_sms)
        (Qg, Sg), (Qu, Su), (Qd, Sd) = self.gate, self.up, self.down
        if self.fused:
            h = fa.qgemm_grouped_glu(self.hidden, off, Qg[c], Sg[c], t2, Qu[c], Su[c], t2, *a, rows=self.token.to(torch.int32))
            return fa.qgemm_grouped_weighted(h, off, Qd[c], Sd[c], t2, self.topk_weights[self.perm].float(), *a)
        x = self.hidden[self.token]
        h = torch.nn.functional.silu(fa.qgemm_grouped(x, off, Qg[c], Sg[c], t2, *a)) * fa.qgemm_grouped(x, off, Qu[c], Su[c], t2, *a)
        y = fa.qgemm_grouped(h, off, Qd[c], Sd[c], t2, *a) * self.topk_weights[self.perm].to(DTYPE)[:, None]
        served = torch.arange(y.shape[0], device=y.device) < off[-1]
        return torch.where(served[:, None], y, torch.zeros_like(y))

    def bytes(self):
        routed = sum(1 for c in self.counts if c)
        per_expert = 3 * ((BITS * self.F // 16) * self.K * 2 + self.F * (self.K // G) * 2)
        return routed * per_expert + sum(self.counts) * 2 * self.K * 2


def main_mlp(args, device):
    rows = []
    per_copy = 3 * E * ((BITS * 14336 // 16) * 4096 * 2 + 14336 * (4096 // G) * 2)
    copies = max(2, bench.L3_BYTES // per_copy + 2)
    for tokens in args.tokens:
        counts = routing(tokens, seed=tokens)
        unfused = Mlp(counts, tokens, copies, device, fused=False)
        fused = Mlp(counts, tokens, copies, device, fused=True)
        a, b = unfused.step(0).float(), fused.step(0).float()
        torch.cuda.synchronize()
        # two passes of each, alternating; the figure is the mean of each form's two medians
        m = [measure(layer, args) for layer in (unfused, fused, unfused, fused)]
        u_us, f_us = (m[0]["us"] + m[2]["us"]) / 2, (m[1]["us"] + m[3]["us"]) / 2
        nbytes = fused.bytes()
        row = {"tokens": tokens, "rows": sum(counts), "counts": counts, "weight_copies": copies,
               "unfused_us": round(u_us, 3), "fused_us": round(f_us, 3), "fused_over_unfused": round(f_us / u_us, 4),
               "bytes": nbytes, "fused_GBps": round(nbytes / f_us * 1e-3, 1), "unfused_GBps": round(nbytes / u_us * 1e-3, 1),
               "max_abs_diff_fused_vs_unfused": float((a - b).abs().max()), "max_abs_unfused": float(a.abs().max()),
               "passes": m}
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "passes"}), flush=True)
        del unfused, fused
        torch.cuda.empty_cache()
    out = {"what": "expert MLP step (gather .. weighted down-projection output): three grouped launches + torch ops vs the two "
                   "fused launches, hipGraph replays, device-clock stamps, cold caches",
           "config": {"bits": BITS, "group_size": G, "experts": E, "top_k": TOPK, "dtype": "float16", "K": 4096, "F": 14336,
                      "steps": args.steps, "warmup": args.warmup, "replays": args.replays,
                      "device": torch.cuda.get_device_name(device)},
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


class Step:
    """`copies` FluteExperts(fused=True) on random stacks of the --mode mlp shapes; step(i) is one whole forward on set i."""

    def __init__(self, stacks, tokens, device, native):
        from flute_amd.integrations import moe
        self.experts = [moe.FluteExperts(g, u, d, fused=True, native_routing=native) for g, u, d in stacks]
        gen = torch.Generator(device=device).manual_seed(tokens)
        self.hidden = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE)
        self.ids = torch.rand(tokens, E, generator=torch.Generator().manual_seed(tokens)).topk(TOPK, dim=1).indices.to(device)
        w = torch.rand(tokens, TOPK, device=device, generator=gen)
        self.weights = (w / w.sum(1, keepdim=True)).to(DTYPE)

    def step(self, i):
        return self.experts[i % len(self.experts)](self.hidden, self.ids, self.weights)


def step_stacks(copies, device):
    """`copies` sets of gate / up [F, K] and down [K, F] GroupedFluteLinear with random packed bits, shared by both forms."""
    import flute_amd
    from flute_amd import utils
    from flute_amd.integrations import moe
    K, F = 4096, 14336
    gen = torch.Generator(device=device).manual_seed(1)
    tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == BITS and c["TileP"] == 32)
    table = torch.randn(2 ** BITS, device=device, generator=gen).sort().values.to(DTYPE)
    t2 = utils.make_qmap2_from_qmap(table).repeat(E, 1, 1, 1)

    def grouped(Kin, N):
        m = moe.GroupedFluteLinear(E, Kin, N, BITS, G, tid, device, DTYPE)
        m.weight.copy_(torch.randint(-2 ** 15, 2 ** 15, tuple(m.weight.shape), dtype=torch.int16, device=device, generator=gen))
        m.scales.copy_((torch.rand(tuple(m.scales.shape), device=device, generator=gen) * 0.02 + 0.005).to(DTYPE))
        m.tables.copy_(table.repeat(E, 1))
        m.tables2.copy_(t2)
        return m
    return [(grouped(K, F), grouped(K, F), grouped(F, K)) for _ in range(copies)]


R_E, R_TOPK, R_N = 64, 8, 2048          # the routing-only rows


class RoutingOnly:
    """The routing around the launches without them: Y [T k, N] stands for the down projection's output."""

    def __init__(self, tokens, device, native):
        import flute_amd
        from flute_amd.integrations import moe
        self.fa, self.moe, self.native = flute_amd, moe, native
        gen = torch.Generator(device=device).manual_seed(tokens)
        self.ids = torch.rand(tokens, R_E, generator=torch.Generator().manual_seed(tokens)).topk(R_TOPK, dim=1).indices.to(device)
        w = torch.rand(tokens, R_TOPK, device=device, generator=gen)
        self.weights = (w / w.sum(1, keepdim=True)).to(DTYPE)
        self.hidden = torch.randn(tokens, R_N, device=device, generator=gen).to(DTYPE)
        self.y = torch.randn(tokens * R_TOPK, R_N, device=device, generator=gen).to(DTYPE)

    def step(self, i):
        if self.native:
            offsets, rows, row_weight, pos, _ = self.fa.moe_route(self.ids, self.weights, R_E)
            return self.fa.moe_combine(self.y, pos, offsets)
        # FluteExperts.forward / _forward_fused around the two launches, as it is by default
        perm, offsets = self.moe.sort_by_expert(self.ids, R_E)
        token = perm // R_TOPK
        rows, row_weight = token.to(torch.int32), self.weights.reshape(-1)[perm].float()
        return torch.zeros_like(self.hidden).index_add_(0, token, self.y)


def step_row(off, on, args, **head):
    a, b = off.step(0).float(), on.step(0).float()
    torch.cuda.synchronize()
    # two passes of each, alternating; the figure is the mean of each form's two medians
    m = [measure(layer, args) for layer in (off, on, off, on)]
    off_us, on_us = (m[0]["us"] + m[2]["us"]) / 2, (m[1]["us"] + m[3]["us"]) / 2
    row = dict(head, torch_routing_us=round(off_us, 3), native_routing_us=round(on_us, 3),
               native_over_torch=round(on_us / off_us, 4), spread=max(p["spread"] for p in m),
               max_abs_diff_native_vs_torch=float((a - b).abs().max()), max_abs_torch=float(a.abs().max()), passes=m)
    print(json.dumps({k: v for k, v in row.items() if k != "passes"}), flush=True)
    return row


def child_step(args, device):
    """One process's rows, written to args.out."""
    rows = []
    per_copy = 3 * E * ((BITS * 14336 // 16) * 4096 * 2 + 14336 * (4096 // G) * 2)
    copies = max(2, bench.L3_BYTES // per_copy + 2)
    stacks = step_stacks(copies, device)
    for tokens in args.tokens:
        off, on = Step(stacks, tokens, device, native=False), Step(stacks, tokens, device, native=True)
        rows.append(step_row(off, on, args, what="forward", tokens=tokens, rows=tokens * TOPK, experts=E, top_k=TOPK,
                             weight_copies=copies))
    del stacks, off, on
    torch.cuda.empty_cache()
    for tokens in args.routing_tokens:
        off, on = RoutingOnly(tokens, device, native=False), RoutingOnly(tokens, device, native=True)
        rows.append(step_row(off, on, args, what="routing only", tokens=tokens, rows=tokens * R_TOPK, experts=R_E,
                             top_k=R_TOPK, N=R_N))
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(device), "rows": rows}, f)


def main_step(args):
    """`--processes` fresh child processes one after the other; per row the median of the processes' figures, and the
    spread: the largest (max - min) / median among the replays of any pass of the row, in any process."""
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(args.processes):
            path = os.path.join(tmp, "p%d.json" % i)
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", args.mode, "--child", "--out", path, "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--replays", str(args.replays), "--tokens", *map(str, args.tokens),
                   "--routing-tokens", *map(str, args.routing_tokens)]
            subprocess.run(cmd, check=True)
            with open(path) as f:
                runs.append(json.load(f))
    median = lambda v: sorted(v)[len(v) // 2]
    rows = []
    for i, first in enumerate(runs[0]["rows"]):
        per = [r["rows"][i] for r in runs]
        off_us, on_us = median([p["torch_routing_us"] for p in per]), median([p["native_routing_us"] for p in per])
        spread = max(p["spread"] for p in per)
        row = {k: first[k] for k in first if k in ("what", "tokens", "rows", "experts", "top_k", "N", "weight_copies", "scoring",
                                                   "bias")}
        row.update(torch_routing_us=off_us, native_routing_us=on_us, saved_us=round(off_us - on_us, 3),
                   native_over_torch=round(on_us / off_us, 4), spread=spread,
                   faster_by_more_than_spread=bool(1 - on_us / off_us > spread),
                   per_process_torch_us=[p["torch_routing_us"] for p in per],
                   per_process_native_us=[p["native_routing_us"] for p in per],
                   max_abs_diff_native_vs_torch=max(p["max_abs_diff_native_vs_torch"] for p in per),
                   max_abs_torch=first["max_abs_torch"],
                   replays_us=[[q["replays_us"] for q in p["passes"]] for p in per])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
    what = {"step": "FluteExperts(fused=True).forward, native_routing off (sort_by_expert + torch glue + zeros_like + index_add_) vs on "
                    "(moe_route + moe_combine); and the routing alone without the GEMMs; hipGraph replays, device-clock stamps, cold "
                    "caches; passes per process: off, on, off, on",
            "gate": "from router logits: 'torch' = the models' torch gating chain (softmax / sigmoid, topk, renormalise) + moe_route, "
                    "'native' = one moe_gate_route launch; and the whole block (router GEMM, gating, "
                    "FluteExperts(fused=True, native_routing=True)) with the chain vs FluteSparseMoeBlock; hipGraph replays, "
                    "device-clock stamps, cold caches; passes per process: torch, native, torch, native"}[args.mode]
    out = {"what": what,
           "config": {"bits": BITS, "group_size": G, "dtype": "float16", "K": 4096, "F": 14336, "steps": args.steps,
                      "warmup": args.warmup, "replays": args.replays, "processes": args.processes, "device": runs[0]["device"]},
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


GATE_SHAPES = [(8, 2, "softmax", False, 1.0), (64, 8, "softmax", False, 1.0), (256, 8, "sigmoid", True, 2.5)]


def torch_gate(logits, k, scoring, bias, scale):
    """The gating chain of the models' own code, with renormalisation: softmax (Mixtral, Qwen-MoE) or sigmoid with the
    selection bias (DeepSeek-V3)."""
    if scoring == "softmax":
        w, ids = torch.topk(torch.softmax(logits, dim=1, dtype=torch.float32), k, dim=1)
    else:
        s = torch.sigmoid(logits.float())
        ids = torch.topk(s if bias is None else s + bias, k, dim=1).indices
        w = s.gather(1, ids)
    w = w / w.sum(dim=1, keepdim=True)
    return ids, (w if scale == 1.0 else w * scale)


class GateOnly:
    """From logits [T, E] fp16 to the routing arrays; step(i) returns `offsets`."""

    def __init__(self, tokens, shape, device, native):
        import flute_amd
        self.fa, self.native = flute_amd, native
        self.E, self.k, self.scoring, with_bias, self.scale = shape
        gen = torch.Generator(device=device).manual_seed(tokens + self.E)
        self.logits = (torch.randn(tokens, self.E, device=device, generator=gen) * 2).to(DTYPE)
        self.bias = torch.randn(self.E, device=device, generator=gen) * 0.1 if with_bias else None

    def step(self, i):
        if self.native:
            return self.fa.moe_gate_route(self.logits, self.k, self.E, self.scoring, True, self.bias, self.scale)[2]
        ids, w = torch_gate(self.logits, self.k, self.scoring, self.bias, self.scale)
        return self.fa.moe_route(ids, w, self.E)[0]


class Block:
    """The whole sparse-MoE block on `copies` FluteExperts(fused=True, native_routing=True): router GEMM, gating, experts."""

    def __init__(self, stacks, tokens, device, native):
        from flute_amd.integrations import moe
        self.native = native
        gen = torch.Generator(device=device).manual_seed(tokens)
        self.hidden = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE)
        self.router = (torch.randn(E, 4096, device=device, generator=gen) * 0.02).to(DTYPE)
        self.experts = [moe.FluteExperts(g, u, d, fused=True, native_routing=True) for g, u, d in stacks]
        self.blocks = [moe.FluteSparseMoeBlock(self.router, x, TOPK, renormalize=True) for x in self.experts]

    def step(self, i):
        c = i % len(self.experts)
        if self.native:
            return self.blocks[c](self.hidden)
        logits = torch.nn.functional.linear(self.hidden, self.router)
        ids, w = torch_gate(logits, TOPK, "softmax", None, 1.0)
        return self.experts[c](self.hidden, ids, w)


def child_gate(args, device):
    """One process's rows, written to args.out."""
    rows = []
    for shape in GATE_SHAPES:
        for tokens in args.routing_tokens:
            off, on = GateOnly(tokens, shape, device, native=False), GateOnly(tokens, shape, device, native=True)
            rows.append(step_row(off, on, args, what="gating + routing", tokens=tokens, rows=tokens * shape[1], experts=shape[0],
                                 top_k=shape[1], scoring=shape[2], bias=shape[3]))
    per_copy = 3 * E * ((BITS * 14336 // 16) * 4096 * 2 + 14336 * (4096 // G) * 2)
    copies = max(2, bench.L3_BYTES // per_copy + 2)
    stacks = step_stacks(copies, device)
    for tokens in args.tokens:
        off, on = Block(stacks, tokens, device, native=False), Block(stacks, tokens, device, native=True)
        rows.append(step_row(off, on, args, what="block", tokens=tokens, rows=tokens * TOPK, experts=E, top_k=TOPK,
                             scoring="softmax", bias=False, weight_copies=copies))
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(device), "rows": rows}, f)


LIMITED_SHAPE = dict(E=256, k=8, n_group=8, topk_group=4, scoring="sigmoid", scale=2.5, group_score="top2sum")


def torch_gate_limited(logits, bias, E, k, n_group, topk_group, scale):
    """DeepSeek-V3's group-limited gating as a torch-op chain, with the -infinity mask."""
    T = logits.shape[0]
    s = torch.sigmoid(logits.float())
    c = s + bias
    group_scores = c.view(T, n_group, E // n_group).topk(2, dim=-1).values.sum(dim=-1)
    group_idx = torch.topk(group_scores, topk_group, dim=-1).indices
    group_mask = torch.zeros_like(group_scores).scatter_(1, group_idx, 1.0)
    score_mask = group_mask.unsqueeze(-1).expand(T, n_group, E // n_group).reshape(T, E)
    ids = torch.topk(c.masked_fill(score_mask == 0, float("-inf")), k, dim=-1).indices
    w = s.gather(1, ids)
    w = w / w.sum(dim=-1, keepdim=True)
    return ids, w * scale


class GateLimited:
    """From logits [T, 256] fp16 to (ids, weights); step(i) returns the weights.  form: "limited", "unlimited" or "torch"."""

    def __init__(self, tokens, device, form):
        import flute_amd
        self.fa, self.form = flute_amd, form
        gen = torch.Generator(device=device).manual_seed(tokens + LIMITED_SHAPE["E"])
        self.logits = (torch.randn(tokens, LIMITED_SHAPE["E"], device=device, generator=gen) * 2).to(DTYPE)
        self.bias = torch.randn(LIMITED_SHAPE["E"], device=device, generator=gen) * 0.1

    def step(self, i):
        c = LIMITED_SHAPE
        if self.form == "limited":
            return self.fa.moe_gate_limited(self.logits, c["k"], c["n_group"], c["topk_group"], c["scoring"], True, self.bias,
                                            c["scale"], c["group_score"])[1]
        if self.form == "unlimited":
            return self.fa.moe_gate(self.logits, c["k"], c["scoring"], True, self.bias, c["scale"])[1]
        return torch_gate_limited(self.logits, self.bias, c["E"], c["k"], c["n_group"], c["topk_group"], c["scale"])[1]


def main_gate_limited(args, device):
    rows = []
    for tokens in args.tokens:
        forms = {f: GateLimited(tokens, device, f) for f in ("limited", "unlimited", "torch")}
        ids = forms["limited"].fa.moe_gate_limited(forms["limited"].logits, 8, 8, 4, "sigmoid", True, forms["limited"].bias, 2.5,
                                                   "top2sum")[0]
        want = torch_gate_limited(forms["torch"].logits, forms["torch"].bias, 256, 8, 8, 4, 2.5)[0]
        diff = float((forms["limited"].step(0) - forms["torch"].step(0)).abs().max())
        torch.cuda.synchronize()
        # two passes of each, alternating; the figure is the mean of each form's two medians
        order = ("limited", "unlimited", "torch") * 2
        m = [measure(forms[f], args) for f in order]
        us = {f: (m[i]["us"] + m[i + 3]["us"]) / 2 for i, f in enumerate(order[:3])}
        row = dict(LIMITED_SHAPE, tokens=tokens, bias=True, renormalize=True, moe_gate_limited_us=round(us["limited"], 3),
                   moe_gate_us=round(us["unlimited"], 3), torch_chain_us=round(us["torch"], 3),
                   group_stage_us=round(us["limited"] - us["unlimited"], 3),
                   limited_over_torch=round(us["limited"] / us["torch"], 4), spread=max(p["spread"] for p in m),
                   ids_equal_torch_chain=bool(torch.equal(ids.long(), want)), max_abs_weight_diff_vs_torch=diff,
                   replays_us={f: [m[i]["replays_us"], m[i + 3]["replays_us"]] for i, f in enumerate(order[:3])})
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
        rows.append(row)
    out = {"what": "group-limited gating alone at DeepSeek-V3's shape, fp16 logits [T, 256] -> (ids, weights): one moe_gate_limited "
                   "launch; one moe_gate launch at the same (E, k) (no group stage); the torch-op chain for the same selection. "
                   "hipGraph replays of `steps` calls between device-clock stamps, cold caches, median of `replays`; passes: "
                   "limited, unlimited, torch, twice",
           "config": {"steps": args.steps, "warmup": args.warmup, "replays": args.replays, "dtype": "float16",
                      "device": torch.cuda.get_device_name(device)},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


# ---- --mode input_grad ------------------------------------------------------------------------------------------------
PEAK_FLOPS = 2.5e15
IG_SHAPES = [("mixtral gate_up", 8, 14336, 4096, 512), ("mixtral gate_up", 8, 14336, 4096, 4096),
             ("mixtral down", 8, 4096, 14336, 512), ("mixtral down", 8, 4096, 14336, 4096),
             ("many-expert gate_up", 64, 1408, 2048, 4096), ("many-expert down", 64, 2048, 1408, 4096)]


def ig_counts(rows, experts, seed):
    """Row counts of `rows` routed rows over `experts` experts, drawn as a top-2 router would spread them."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.rand(rows // 2, experts, generator=gen).topk(2, dim=1).indices
    return torch.bincount(ids.reshape(-1), minlength=experts).tolist()


class InputGrad:
    """`copies` stacks of `experts` packed layers [N, K] (`pair`: two of them, and two dY); step(i) is dX [R, K] = dY [R, N] @ W_e on
    copy i: one grouped launch - `how` = "slabs" / "blocks" / "auto" - or, "loop", the per-expert loop of dequantize + mm on row
    ranges the host knows.  `weights`: another InputGrad of the same stack whose weight copies are shared."""

    def __init__(self, experts, N, K, counts, copies, device, how, bits=BITS, dtype=DTYPE, pair=False, weights=None):
        import flute_amd
        from flute_amd import utils
        self.fa, self.N, self.K, self.counts, self.how, self.bits, self.pair = flute_amd, N, K, counts, how, bits, pair
        self.num_sms = utils.get_device_num_sms(device)
        gen = torch.Generator(device=device).manual_seed(1)
        nst = 2 if pair else 1
        if weights is None:
            self.Q = [torch.randint(-2 ** 15, 2 ** 15, (copies, experts, bits * N // 16, K), dtype=torch.int16, device=device,
                                    generator=gen) for _ in range(nst)]
            self.S = [(torch.rand(copies, experts, N, K // G, device=device, generator=gen) * 0.02 + 0.005).to(dtype)
                      for _ in range(nst)]
            table = torch.randn(2 ** bits, device=device, generator=gen).sort().values.to(dtype)
            self.table2 = utils.make_qmap2_from_qmap(table)
            self.tables2 = self.table2.repeat(experts, 1, 1, 1)
        else:
            self.Q, self.S, self.table2, self.tables2 = weights.Q, weights.S, weights.table2, weights.tables2
        gen_y = torch.Generator(device=device).manual_seed(2)    # (its own generator: contenders that share weights share dY too)
        self.dY = [torch.randn(sum(counts), N, device=device, generator=gen_y).to(dtype) for _ in range(nst)]
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        self.off_host = off
        self.offsets = torch.tensor(off, dtype=torch.int32, device=device)
        self.tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)

    def step(self, i):
        c = i % self.Q[0].shape[0]
        if self.how != "loop":
            second = dict(grad_output2=self.dY[1], weight2=self.Q[1][c], scales2=self.S[1][c], table22=self.tables2) if self.pair else {}
            return self.fa.qgemm_grouped_input_grad(self.dY[0], self.offsets, self.Q[0][c], self.S[0][c], self.tables2, self.bits, G,
                                                    self.tid, self.num_sms, form=None if self.how == "auto" else self.how, **second)
        out = []
        for e, m in enumerate(self.counts):
            if m:
                r0, r1 = self.off_host[e], self.off_host[e + 1]
                W = self.fa.dequantize(self.Q[0][c, e], self.S[0][c, e], self.table2, self.bits, G, self.tid)     # [N, K]
                dx = torch.mm(self.dY[0][r0:r1], W)
                if self.pair:
                    W = self.fa.dequantize(self.Q[1][c, e], self.S[1][c, e], self.table2, self.bits, G, self.tid)
                    dx = torch.addmm(dx, self.dY[1][r0:r1], W)
                out.append(dx)
        return out

    def flops(self):
        return 2.0 * sum(self.counts) * self.N * self.K * len(self.Q)


class BackwardStep:
    """The launches of one backward step of FluteExperts(fused=True, native_routing=True) at `tokens` tokens (top-2, Mixtral's
    shapes), by hand, so that each can be timed alone: `part` selects one, None runs them in the backward's order."""
    PARTS = ("down_input_grad", "recompute_gate_up", "elementwise_dg_du", "pair_input_grad", "moe_combine")

    def __init__(self, stacks, tokens, device, part=None, form=None, ig_form=None, native=False):
        import flute_amd
        from flute_amd import utils
        self.fa, self.part, self.form = flute_amd, part, form   # form: of the recompute's two plain launches (None: automatic)
        self.native = native                                       # the ops' native_glu_grad: moe_gather and swiglu_grad for the torch chains
        self.ig_form = ig_form                                     # ... of the two input-gradient launches (None: automatic)
        self.stacks = stacks                                       # step_stacks: (gate, up, down) GroupedFluteLinear per copy
        self.num_sms = utils.get_device_num_sms(device)
        K, F = 4096, 14336
        gen = torch.Generator(device=device).manual_seed(2)
        ids = torch.rand(tokens, E, device=device, generator=gen).topk(TOPK, dim=1).indices
        weights = torch.rand(tokens, TOPK, device=device, generator=gen)
        self.offsets, self.rows, self.row_weight, self.pos, _ = flute_amd.moe_route(ids, weights, E)
        R = tokens * TOPK
        self.hidden = torch.randn(tokens, K, device=device, generator=gen).to(DTYPE)
        self.x = self.hidden[self.rows.long()]
        self.dY = torch.randn(R, K, device=device, generator=gen).to(DTYPE)
        self.dH = torch.randn(R, F, device=device, generator=gen).to(DTYPE)
        self.g = torch.randn(R, F, device=device, generator=gen).to(DTYPE)
        self.u = torch.randn(R, F, device=device, generator=gen).to(DTYPE)
        self.dx = torch.randn(R, K, device=device, generator=gen).to(DTYPE)

    def step(self, i):
        gate, up, down = self.stacks[i % len(self.stacks)]
        fa, off, t2, a = self.fa, self.offsets, gate.tables2, (BITS, G, gate.template_id, self.num_sms)
        (Qg, Sg), (Qu, Su), (Qd, Sd) = (gate.weight, gate.scales), (up.weight, up.scales), (down.weight, down.scales)
        run = lambda name: self.part in (None, name)
        dH, g, u, dx = self.dH, self.g, self.u, self.dx
        if run("down_input_grad"):
            dH = fa.qgemm_grouped_input_grad(self.dY, off, Qd, Sd, t2, *a, row_weight=self.row_weight, form=self.ig_form)
        if run("recompute_gate_up"):
            if self.part is not None:
                x = self.x
            elif self.native:
                x = fa.moe_gather(self.hidden, self.rows, off)
            else:
                x = self.hidden[self.rows.long()]
            g, u = (fa.qgemm_grouped(x, off, Qg, Sg, t2, *a, form=self.form),
                    fa.qgemm_grouped(x, off, Qu, Su, t2, *a, form=self.form))
        if run("elementwise_dg_du") and self.native:
            dg, du = fa.swiglu_grad(g, u, dH, off)
        elif run("elementwise_dg_du"):
            gf, uf, dh = g.float(), u.float(), dH.float()
            sig = torch.sigmoid(gf)
            dg, du = (dh * uf * sig * (1 + gf * (1 - sig))).to(DTYPE), (dh * (gf * sig)).to(DTYPE)
        else:
            dg, du = self.g, self.u
        if run("pair_input_grad"):
            dx = fa.qgemm_grouped_input_grad(dg, off, Qg, Sg, t2, *a, grad_output2=du, weight2=Qu, scales2=Su, table22=t2,
                                             form=self.ig_form)
        if run("moe_combine"):
            dx = fa.moe_combine(dx, self.pos, off)
        return dx


class ScaleGrad:
    """`copies` stacks of `experts` packed layers [N, K]; step(i) is dS [E, N, K / g] from dY [R, N] and X [R, K] on copy i: one
    grouped launch, or the per-expert loop of the dense qgemm_scale_grad on row ranges the host knows."""

    def __init__(self, experts, N, K, counts, copies, device, grouped):
        import flute_amd
        from flute_amd import utils
        self.fa, self.N, self.K, self.counts, self.grouped = flute_amd, N, K, counts, grouped
        self.num_sms = utils.get_device_num_sms(device)
        gen = torch.Generator(device=device).manual_seed(1)
        self.Q = torch.randint(-2 ** 15, 2 ** 15, (copies, experts, BITS * N // 16, K), dtype=torch.int16, device=device, generator=gen)
        table = torch.randn(2 ** BITS, device=device, generator=gen).sort().values.to(DTYPE)
        self.table2 = utils.make_qmap2_from_qmap(table)
        self.tables2 = self.table2.repeat(experts, 1, 1, 1)
        self.dY = (torch.randn(sum(counts), N, device=device, generator=gen) / 16).to(DTYPE)
        self.X = (torch.randn(sum(counts), K, device=device, generator=gen) / 16).to(DTYPE)
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        self.off_host = off
        self.offsets = torch.tensor(off, dtype=torch.int32, device=device)
        self.tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == BITS and c["TileP"] == 32)

    def step(self, i):
        c = i % self.Q.shape[0]
        if self.grouped:
            return self.fa.qgemm_grouped_scale_grad(self.dY, self.X, self.offsets, self.Q[c], self.tables2, BITS, G, self.tid,
                                                    self.num_sms)
        out = []
        for e, m in enumerate(self.counts):
            if m:
                r0, r1 = self.off_host[e], self.off_host[e + 1]
                out.append(self.fa.qgemm_scale_grad(self.dY[r0:r1], self.X[r0:r1], self.Q[c, e], self.table2, BITS, G, self.tid,
                                                    self.num_sms))
        return out

    def flops(self):
        return 2.0 * sum(self.counts) * self.N * self.K


def child_scale_grad(args, device):
    rows = []
    for name, experts, N, K, nrows in IG_SHAPES:
        counts = ig_counts(nrows, experts, seed=nrows + experts)
        per_copy = experts * (BITS * N // 16) * K * 2
        copies = max(2, bench.L3_BYTES // per_copy + 2)
        grouped = ScaleGrad(experts, N, K, counts, copies, device, grouped=True)
        loop = ScaleGrad(experts, N, K, counts, copies, device, grouped=False)
        a = torch.stack([grouped.step(0)[e] for e, m in enumerate(counts) if m])
        b = torch.stack(loop.step(0))
        torch.cuda.synchronize()
        diff, ref = float((a.float() - b.float()).abs().max()), float(b.float().abs().max())
        m = [measure(layer, args) for layer in (grouped, loop, grouped, loop)]
        g_us, l_us = (m[0]["us"] + m[2]["us"]) / 2, (m[1]["us"] + m[3]["us"]) / 2
        row = {"what": "scale_grad", "shape": name, "experts": experts, "N": N, "K": K, "rows": sum(counts), "counts_min_max":
               [min(counts), max(counts)], "weight_copies": copies, "grouped_us": round(g_us, 3), "loop_us": round(l_us, 3),
               "grouped_over_loop": round(g_us / l_us, 4), "flop": grouped.flops(),
               "spread": max(p["spread"] for p in m), "max_abs_diff_grouped_vs_loop": diff, "max_abs_loop": ref, "passes": m}
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "passes"}), flush=True)
        del grouped, loop, a, b
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(device), "rows": rows}, f)


class TableGrad(ScaleGrad):
    """`copies` stacks of `experts` packed layers [N, K]; step(i) on copy i is, by `form`: "table" dT2 [E, 2^b, 2^b, 2] from the
    grouped launch pair; "fused" dT2 and dS from it; "separate" the grouped scale gradient and then "table"; "loop" the per-expert
    loop of the dense qgemm_table_grad (dT2 only) on row ranges the host knows.  `as_form` gives another form on the same
    tensors: the forms of a line share one set of weight copies."""

    def __init__(self, experts, N, K, counts, copies, device, form):
        super().__init__(experts, N, K, counts, copies, device, grouped=form != "loop")
        self.form = form
        gen = torch.Generator(device=device).manual_seed(3)
        self.S = (torch.rand(experts, N, K // G, device=device, generator=gen) * 0.02 + 0.005).to(DTYPE)

    def step(self, i):
        c = i % self.Q.shape[0]
        fa, a = self.fa, (BITS, G, self.tid, self.num_sms)
        if self.form == "loop":
            out = []
            for e, m in enumerate(self.counts):
                if m:
                    r0, r1 = self.off_host[e], self.off_host[e + 1]
                    out.append(fa.qgemm_table_grad(self.dY[r0:r1], self.X[r0:r1], self.Q[c, e], self.S[e], *a))
            return out
        if self.form == "fused":
            return fa.qgemm_grouped_table_grad(self.dY, self.X, self.offsets, self.Q[c], self.S, *a, table2=self.tables2,
                                               with_scale_grad=True)
        dT2 = fa.qgemm_grouped_table_grad(self.dY, self.X, self.offsets, self.Q[c], self.S, *a)
        if self.form == "separate":
            return dT2, fa.qgemm_grouped_scale_grad(self.dY, self.X, self.offsets, self.Q[c], self.tables2, *a)
        return dT2

    def as_form(self, form):
        other = copy.copy(self)
        other.form = form
        return other


TG_FORMS = ("table", "fused", "separate", "loop")


def child_table_grad(args, device):
    rows = []
    for name, experts, N, K, nrows in IG_SHAPES:
        counts = ig_counts(nrows, experts, seed=nrows + experts)
        per_copy = experts * (BITS * N // 16) * K * 2
        copies = max(2, bench.L3_BYTES // per_copy + 2)
        base = TableGrad(experts, N, K, counts, copies, device, TG_FORMS[0])
        layers = {f: base.as_form(f) for f in TG_FORMS}
        a = torch.stack([layers["table"].step(0)[e] for e, m in enumerate(counts) if m])
        b = torch.stack(layers["loop"].step(0))
        fused = layers["fused"].step(0)
        sep = layers["separate"].step(0)
        torch.cuda.synchronize()
        diff, ref = float((a - b).abs().max()), float(b.abs().max())
        assert torch.equal(fused[0], sep[0]) and torch.equal(fused[1], sep[1])
        m = [measure(layers[f], args) for f in TG_FORMS + TG_FORMS]
        us = {f: (m[i]["us"] + m[i + len(TG_FORMS)]["us"]) / 2 for i, f in enumerate(TG_FORMS)}
        row = {"what": "table_grad", "shape": name, "experts": experts, "N": N, "K": K, "rows": sum(counts), "counts_min_max":
               [min(counts), max(counts)], "weight_copies": copies, "flop": layers["table"].flops(),
               "scratch_bytes": experts * (N // 128) * -(-K // 256) * 2 * 4 ** BITS * 4}
        row.update({f + "_us": round(us[f], 3) for f in TG_FORMS})
        row.update(table_over_loop=round(us["table"] / us["loop"], 4), fused_over_separate=round(us["fused"] / us["separate"], 4),
                   spread=max(p["spread"] for p in m), max_abs_diff_grouped_vs_loop=diff, max_abs_loop=ref, passes=m)
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "passes"}), flush=True)
        del base, layers, a, b, fused, sep
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(device), "rows": rows}, f)


class Forward:
    """`copies` stacks of `experts` packed layers [N, K]; step(i) is one forward over all routed rows on copy i, by `how`:
    "rows" / "blocks" / "auto" - one grouped launch of that form (mode "plain" or "weighted") -, "loop" - flute_amd.qgemm per expert
    on row ranges the host knows.  (The GLU contenders: GluForward.)"""

    def __init__(self, experts, N, K, counts, copies, device, how, mode="plain", bits=BITS, dtype=DTYPE):
        import flute_amd
        from flute_amd import utils
        self.fa, self.N, self.K, self.counts, self.how, self.mode, self.bits = flute_amd, N, K, counts, how, mode, bits
        self.num_sms = utils.get_device_num_sms(device)
        self.ws = utils.get_workspace_streamk(device)
        gen = torch.Generator(device=device).manual_seed(1)
        nst = 1
        self.Q = [torch.randint(-2 ** 15, 2 ** 15, (copies, experts, bits * N // 16, K), dtype=torch.int16, device=device,
                                generator=gen) for _ in range(nst)]
        self.S = [(torch.rand(copies, experts, N, K // G, device=device, generator=gen) * 0.02 + 0.005).to(dtype) for _ in range(nst)]
        self.table = torch.randn(2 ** bits, device=device, generator=gen).sort().values.to(dtype)
        self.table2 = utils.make_qmap2_from_qmap(self.table)
        self.tables2 = self.table2.repeat(experts, 1, 1, 1)
        self.X = torch.randn(sum(counts), K, device=device, generator=gen).to(dtype)
        self.w = torch.rand(sum(counts), device=device, generator=gen)
        off = [0]
        for c in counts:
            off.append(off[-1] + c)
        self.off_host = off
        self.offsets = torch.tensor(off, dtype=torch.int32, device=device)
        self.tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)

    def step(self, i):
        c = i % self.Q[0].shape[0]
        fa, a = self.fa, (self.bits, G, self.tid, self.num_sms)
        Q, S, t2 = self.Q[0][c], self.S[0][c], self.tables2
        if self.how == "loop":
            ys = []
            for e, m in enumerate(self.counts):
                if m:
                    r0, r1 = self.off_host[e], self.off_host[e + 1]
                    ys.append(fa.qgemm(self.X[r0:r1], Q[e], S[e], self.table, self.table2, self.ws, *a))
            return ys
        form = None if self.how == "auto" else self.how
        if self.mode == "weighted":
            return fa.qgemm_grouped_weighted(self.X, self.offsets, Q, S, t2, self.w, *a, form=form)
        return fa.qgemm_grouped(self.X, self.offsets, Q, S, t2, *a, form=form)

    def flops(self):
        return 2.0 * sum(self.counts) * self.N * self.K * len(self.Q)


class GluForward:
    """`copies` pairs of gate / up stacks of `experts` packed layers [F, K] and `rows` sorted rows read out of rows / 2 source rows
    through an index (top-2 routing); step(i) is silu(gate) * up on copy i, by `how`: "rows" - the fused launch, flute_amd.qgemm_grouped_glu
    (the row form at every count) -, "blocks" - flute_amd.qgemm_grouped_glu_blocks -, "unfused" - the gather, two plain grouped
    launches on the automatic form, silu and the product.  `weights`: another GluForward whose stacks and activations are shared."""

    def __init__(self, experts, F, K, counts, copies, device, how, bits=BITS, dtype=DTYPE, weights=None):
        import flute_amd
        from flute_amd import utils
        self.fa, self.F, self.K, self.counts, self.how, self.bits, self.experts = flute_amd, F, K, counts, how, bits, experts
        self.num_sms = utils.get_device_num_sms(device)
        if weights is None:
            gen = torch.Generator(device=device).manual_seed(1)
            R = sum(counts)
            self.Q = [torch.randint(-2 ** 15, 2 ** 15, (copies, experts, bits * F // 16, K), dtype=torch.int16, device=device,
                                    generator=gen) for _ in range(2)]
            self.S = [(torch.rand(copies, experts, F, K // G, device=device, generator=gen) * 0.02 + 0.005).to(dtype) for _ in range(2)]
            table = torch.randn(2 ** bits, device=device, generator=gen).sort().values.to(dtype)
            self.tables2 = utils.make_qmap2_from_qmap(table).repeat(experts, 1, 1, 1)
            self.hidden = torch.randn(max(1, R // TOPK), K, device=device, generator=gen).to(dtype)
            self.rows = torch.randint(0, self.hidden.shape[0], (R,), device=device, generator=gen).to(torch.int32)
            off = [0]
            for c in counts:
                off.append(off[-1] + c)
            self.offsets = torch.tensor(off, dtype=torch.int32, device=device)
        else:
            for name in ("Q", "S", "tables2", "hidden", "rows", "offsets"):
                setattr(self, name, getattr(weights, name))
        self.tid = min(t for (b, t), c in flute_amd.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == 32)

    def step(self, i):
        c = i % self.Q[0].shape[0]
        fa, a, t2, off = self.fa, (self.bits, G, self.tid, self.num_sms), self.tables2, self.offsets
        if self.how == "unfused":
            x = self.hidden[self.rows.long()]
            return torch.nn.functional.silu(fa.qgemm_grouped(x, off, self.Q[0][c], self.S[0][c], t2, *a)) * \
                fa.qgemm_grouped(x, off, self.Q[1][c], self.S[1][c], t2, *a)
        op = fa.qgemm_grouped_glu_blocks if self.how == "blocks" else fa.qgemm_grouped_glu
        return op(self.hidden, off, self.Q[0][c], self.S[0][c], t2, self.Q[1][c], self.S[1][c], t2, *a, rows=self.rows)

    def flops(self):
        return 2.0 * sum(self.counts) * self.F * self.K * 2


class ModuleStep:
    """One forward and one backward step of FluteExperts(fused=True, native_routing=True, glu_blocks=...) at `tokens` tokens (top-2)
    on copy i of step_stacks: the gradient reaches the hidden states (the experts' parameters are frozen)."""

    def __init__(self, stacks, tokens, device, glu_blocks, backward):
        from flute_amd.integrations import moe
        self.experts = [moe.FluteExperts(g, u, d, fused=True, native_routing=True, glu_blocks=glu_blocks) for g, u, d in stacks]
        self.backward = backward
        gen = torch.Generator(device=device).manual_seed(tokens)
        self.hidden = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE).requires_grad_(backward)
        self.ids = torch.rand(tokens, E, generator=torch.Generator().manual_seed(tokens)).topk(TOPK, dim=1).indices.to(device)
        w = torch.rand(tokens, TOPK, device=device, generator=gen)
        self.weights = (w / w.sum(1, keepdim=True)).to(DTYPE)
        self.dOut = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE)

    def step(self, i):
        y = self.experts[i % len(self.experts)](self.hidden, self.ids, self.weights)
        if not self.backward:
            return y
        return torch.autograd.grad(y, self.hidden, self.dOut)[0]


def even_counts(rows, experts):
    """`rows` rows spread as evenly as they go."""
    return [rows // experts + (e < rows % experts) for e in range(experts)]


# (name, experts, N, K, routed rows, bits, dtype, mode); the first six are --mode projection's shapes and counts at rows / 2 tokens
PREFILL_LINES = [("mixtral gate_up", 8, 14336, 4096, r, 4, "float16", "plain") for r in (512, 4096, 8192)] + \
                [("mixtral down", 8, 4096, 14336, r, 4, "float16", "plain") for r in (512, 4096, 8192)] + \
                [("many-expert gate_up", 64, 1408, 2048, 4096, 4, "float16", "plain"),
                 ("many-expert down", 64, 2048, 1408, 4096, 4, "float16", "plain"),
                 ("many-expert 2048 x 2048", 64, 2048, 2048, 4096, 4, "float16", "plain"),
                 ("mixtral gate_up", 8, 14336, 4096, 4096, 4, "bfloat16", "plain"),
                 ("mixtral gate_up", 8, 14336, 4096, 4096, 2, "float16", "plain"),
                 ("mixtral down", 8, 4096, 14336, 4096, 4, "float16", "weighted"),
                 ("mixtral down", 8, 4096, 14336, 8192, 4, "float16", "weighted")]
SWEEP_MEANS = (16, 32, 48, 64, 96, 128, 192, 256)
# (name, experts, F, K, routed rows, bits, dtype): the fused GLU launch on its two forms against the unfused sequence
GLU_LINES = [("mixtral gate_up pair", 8, 14336, 4096, r, 4, "float16") for r in (512, 4096, 8192)] + \
            [("many-expert 2048 x 2048 pair", 64, 2048, 2048, 4096, 4, "float16"),
             ("mixtral gate_up pair", 8, 14336, 4096, 4096, 4, "bfloat16"),
             ("mixtral gate_up pair", 8, 14336, 4096, 4096, 2, "float16")]
GLU_SWEEP_MEANS = (16, 32, 48, 64, 96, 128)
GLU_SWEEP_STACKS = [("mixtral gate_up pair", 8, 14336, 4096), ("many-expert 2048 x 2048 pair", 64, 2048, 2048),   # fill the chip
                    ("E 8 4096 x 4096 pair", 8, 4096, 4096)]                                                       # 128 workgroups: does not
PREFILL_SECTIONS = ("forward", "glu", "sweep", "backward", "glu_sweep", "glu_module")
SWEEP_STACKS = [("mixtral gate_up", 8, 14336, 4096), ("mixtral down", 8, 4096, 14336), ("many-expert 2048 x 2048", 64, 2048, 2048)]


def prefill_copies(experts, N, K, bits, stacks=1):
    per_copy = stacks * experts * ((bits * N // 16) * K * 2 + N * (K // G) * 2)
    return max(2, bench.L3_BYTES // per_copy + 2)


def time_forms(layers, args):
    """Two alternating passes over `layers` {name: layer}: {name: mean of its two medians}, the largest spread, the passes."""
    for layer in layers.values():
        layer.step(0)
    torch.cuda.synchronize()
    order = list(layers) * 2
    m = [measure(layers[n], args) for n in order]
    us = {n: round(sum(p["us"] for o, p in zip(order, m) if o == n) / 2, 3) for n in layers}
    return us, max(p["spread"] for p in m), {n: [p["replays_us"] for o, p in zip(order, m) if o == n] for n in layers}


def main_prefill(args, device):
    from flute_amd import dev
    rows = []
    tid = None

    def emit(row):
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
        with open(args.out, "w") as f:                # (rewritten after every line: a long run that is cut short keeps its lines)
            json.dump({"what": "grouped forward at prefill / training row counts: row form, block form, the automatic rule and a "
                               "per-expert loop of flute_amd.qgemm with host-known counts; hipGraph replays, device-clock stamps, "
                               "cold caches, median of the replays, two alternating passes of each form in one process",
                       "config": {"group_size": G, "steps": args.steps, "warmup": args.warmup, "replays": args.replays,
                                  "device": torch.cuda.get_device_name(device)}, "rows": rows}, f, indent=1)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    want = lambda section: args.only is None or section in args.only
    for name, experts, N, K, nrows, bits, dt, mode in (PREFILL_LINES if want("forward") else ()):
        dtype = getattr(torch, dt)
        counts = routing(nrows // 2, seed=nrows // 2) if experts == E else ig_counts(nrows, experts, seed=nrows + experts)
        copies = prefill_copies(experts, N, K, bits)
        mk = lambda how: Forward(experts, N, K, counts, copies, device, how, mode, bits, dtype)
        layers = {"rows": mk("rows"), "auto": mk("auto")}
        auto_form = dev.grouped_form(mode, experts, sum(counts), N, K, bits, G, layers["rows"].tid, layers["rows"].num_sms, dtype)
        try:
            layers["blocks"] = mk("blocks")
            layers["blocks"].step(0)
        except RuntimeError:
            layers.pop("blocks")                      # the block form does not serve this stack
        if mode == "plain":
            layers["loop"] = mk("loop")
        us, spread, replays = time_forms(layers, args)
        flop = layers["rows"].flops()
        row = {"what": "forward", "shape": name, "mode": mode, "bits": bits, "dtype": dt, "experts": experts, "N": N, "K": K,
               "rows": sum(counts), "counts_min_max": [min(counts), max(counts)], "weight_copies": copies, "auto_form": auto_form,
               "us": us, "TFLOPs": {n: round(flop / v * 1e-6, 1) for n, v in us.items()}, "spread": spread, "flop": flop}
        if "blocks" in us:
            nblk = sum(-(-c // 128) for c in counts) * (N // 256)
            num_sms = layers["rows"].num_sms
            row.update(blocks_over_rows=round(us["blocks"] / us["rows"], 4), row_blocks=sum(-(-c // 128) for c in counts),
                       workgroups_with_rows=nblk, rounds_of_256_CUs=round(nblk / num_sms, 2),
                       us_per_block_round_at_K4096=round(us["blocks"] / max(1.0, nblk / num_sms) * 4096 / K, 2))
        row["replays_us"] = replays
        emit(row)
        del layers
        torch.cuda.empty_cache()
    # the fused GLU launch through the routing index: its row form, its block form (flute_amd.qgemm_grouped_glu_blocks) and the
    # unfused sequence - gather, two plain automatic launches, silu and the product
    def glu_layers(experts, F, K, counts, bits=BITS, dtype=DTYPE):
        copies = prefill_copies(experts, F, K, bits, stacks=2)
        first = GluForward(experts, F, K, counts, copies, device, "rows", bits, dtype)
        layers = {"rows": first}
        for how in ("blocks", "unfused"):
            layers[how] = GluForward(experts, F, K, counts, copies, device, how, bits, dtype, weights=first)
        return layers, copies

    for name, experts, F, K, nrows, bits, dt in (GLU_LINES if want("glu") else ()):
        dtype = getattr(torch, dt)
        counts = routing(nrows // 2, seed=nrows // 2) if experts == E else ig_counts(nrows, experts, seed=nrows + experts)
        layers, copies = glu_layers(experts, F, K, counts, bits, dtype)
        first = layers["rows"]
        a, b = layers["blocks"].step(0).float(), first.step(0).float()
        diff, ref = float((a - b).abs().max()), float(b.abs().max())
        us, spread, replays = time_forms(layers, args)
        flop = first.flops()
        emit({"what": "glu", "shape": name, "bits": bits, "dtype": dt, "experts": experts, "F": F, "K": K, "rows": sum(counts),
              "source_rows": first.hidden.shape[0], "counts_min_max": [min(counts), max(counts)], "weight_copies": copies,
              "auto_form": dev.grouped_glu_blocks_form(experts, sum(counts), first.hidden.shape[0], F, K, bits, G, first.tid,
                                                       first.num_sms, dtype),
              "us": us, "blocks_over_rows": round(us["blocks"] / us["rows"], 4),
              "blocks_over_unfused": round(us["blocks"] / us["unfused"], 4),
              "TFLOPs": {n: round(flop / v * 1e-6, 1) for n, v in us.items()}, "spread": spread, "flop": flop,
              "max_abs_diff_blocks_vs_rows": diff, "max_abs_rows": ref, "replays_us": replays})
        del layers, first, a, b
        torch.cuda.empty_cache()
    # the GLU threshold sweep: rows / E on both sides of the rule, the row form against the block form, even counts and a routed draw
    for name, experts, F, K in (GLU_SWEEP_STACKS if want("glu_sweep") else ()):
        for mean in GLU_SWEEP_MEANS:
            for spread_name, counts in (("even", even_counts(mean * experts, experts)),
                                        ("routed", ig_counts(mean * experts, experts, seed=mean + experts))):
                layers, copies = glu_layers(experts, F, K, counts)
                layers.pop("unfused")
                first = layers["rows"]
                us, spread, replays = time_forms(layers, args)
                emit({"what": "glu threshold sweep", "shape": name, "experts": experts, "F": F, "K": K, "mean_rows_per_expert": mean,
                      "counts": spread_name, "counts_min_max": [min(counts), max(counts)], "rows": sum(counts), "us": us,
                      "fills_the_chip": bool(experts * (F // 256) >= first.num_sms),
                      "blocks_over_rows": round(us["blocks"] / us["rows"], 4), "spread": spread,
                      "auto_form": dev.grouped_glu_blocks_form(experts, sum(counts), first.hidden.shape[0], F, K, BITS, G, first.tid,
                                                               first.num_sms), "replays_us": replays})
                del layers, first
                torch.cuda.empty_cache()
    # one forward and one forward + backward step of FluteExperts(fused=True, native_routing=True): glu_blocks False against "auto"
    if want("glu_module"):
        copies = prefill_copies(E, 14336, 4096, BITS, stacks=3)
        stacks = step_stacks(copies, device)
        for tokens in (512, 4096):
            layers = {}
            for backward in (False, True):
                for glu_blocks in (False, "auto"):
                    layers[("forward+backward" if backward else "forward") + (" auto" if glu_blocks else " rows")] = \
                        ModuleStep(stacks, tokens, device, glu_blocks, backward)
            us, spread, replays = time_forms(layers, args)
            emit({"what": "glu module step", "tokens": tokens, "rows": tokens * TOPK, "experts": E, "top_k": TOPK,
                  "weight_copies": copies, "us": us, "forward_auto_over_rows": round(us["forward auto"] / us["forward rows"], 4),
                  "step_auto_over_rows": round(us["forward+backward auto"] / us["forward+backward rows"], 4), "spread": spread,
                  "replays_us": replays})
            del layers
        del stacks
        torch.cuda.empty_cache()
    # the threshold sweep: rows / E on both sides of the rule, rows against blocks, even counts and a routed draw
    for name, experts, N, K in (SWEEP_STACKS if want("sweep") else ()):
        copies = prefill_copies(experts, N, K, BITS)
        for mean in SWEEP_MEANS:
            for spread_name, counts in (("even", even_counts(mean * experts, experts)),
                                        ("routed", ig_counts(mean * experts, experts, seed=mean + experts))):
                layers = {how: Forward(experts, N, K, counts, copies, device, how) for how in ("rows", "blocks", "auto")}
                us, spread, replays = time_forms(layers, args)
                emit({"what": "threshold sweep", "shape": name, "experts": experts, "N": N, "K": K, "mean_rows_per_expert": mean,
                      "counts": spread_name, "counts_min_max": [min(counts), max(counts)], "rows": sum(counts), "us": us,
                      "blocks_over_rows": round(us["blocks"] / us["rows"], 4),
                      "auto_over_best": round(us["auto"] / min(us["rows"], us["blocks"]), 4), "spread": spread,
                      "auto_form": dev.grouped_form("plain", experts, sum(counts), N, K, BITS, G, layers["rows"].tid,
                                                    layers["rows"].num_sms), "replays_us": replays})
                del layers
                torch.cuda.empty_cache()
    # one backward step of FluteExperts(fused=True, native_routing=True): the recompute on the row form and on the automatic rule
    if not want("backward"):
        print("wrote", args.out)
        return
    copies = prefill_copies(E, 14336, 4096, BITS, stacks=3)
    stacks = step_stacks(copies, device)
    for tokens in (512, 4096):
        layers = {}
        for part in (None, "recompute_gate_up"):
            for form in ("rows", None):
                layers[("whole" if part is None else part) + (" rows" if form else " auto")] = BackwardStep(stacks, tokens, device, part, form)
        us, spread, replays = time_forms(layers, args)
        emit({"what": "backward step", "tokens": tokens, "rows": tokens * TOPK, "experts": E, "top_k": TOPK, "weight_copies": copies,
              "us": us, "recompute_share_rows": round(us["recompute_gate_up rows"] / us["whole rows"], 4),
              "recompute_share_auto": round(us["recompute_gate_up auto"] / us["whole auto"], 4), "spread": spread,
              "replays_us": replays})
    print("wrote", args.out)


# (name, experts, N, K, routed rows, bits, dtype, pair): dX [rows, K] = dY [rows, N] @ W_e; the counts are --mode scale_grad's draws
IG_LINES = [("mixtral gate_up", 8, 14336, 4096, r, 4, "float16", False) for r in (512, 4096, 8192)] + \
           [("mixtral down", 8, 4096, 14336, r, 4, "float16", False) for r in (512, 4096, 8192)] + \
           [("many-expert 2048 x 2048", 64, 2048, 2048, 4096, 4, "float16", False),
            ("mixtral gate_up", 8, 14336, 4096, 4096, 4, "bfloat16", False),
            ("mixtral gate_up", 8, 14336, 4096, 4096, 2, "float16", False),
            ("mixtral gate_up pair", 8, 14336, 4096, 512, 4, "float16", True),
            ("mixtral gate_up pair", 8, 14336, 4096, 4096, 4, "float16", True)]
IG_FORMS = ("slabs", "blocks", "auto")


def main_input_grad_forms(args, device):
    """--mode input_grad: the two forms of the grouped input gradient, the automatic rule and the per-expert loop, in one process."""
    from flute_amd import dev
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
        with open(args.out, "w") as f:                # (rewritten after every line: a long run that is cut short keeps its lines)
            json.dump({"what": "grouped input gradient at training row counts: slab form, block form, the automatic rule and a "
                               "per-expert loop of flute_amd.dequantize + torch.mm with host-known counts; hipGraph replays, "
                               "device-clock stamps, cold caches, median of the replays, two alternating passes of each contender "
                               "in one process; then the threshold sweep and one backward step of FluteExperts(fused=True, "
                               "native_routing=True) with its two input-gradient launches on the slab form and on the automatic rule",
                       "config": {"group_size": G, "steps": args.steps, "warmup": args.warmup, "replays": args.replays,
                                  "device": torch.cuda.get_device_name(device)}, "rows": rows}, f, indent=1)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name, experts, N, K, nrows, bits, dt, pair in IG_LINES:
        dtype = getattr(torch, dt)
        counts = ig_counts(nrows, experts, seed=nrows + experts)
        copies = prefill_copies(experts, N, K, bits, stacks=2 if pair else 1)
        first = InputGrad(experts, N, K, counts, copies, device, "slabs", bits, dtype, pair)
        layers = {"slabs": first}
        for how in ("blocks", "auto", "loop"):
            layers[how] = InputGrad(experts, N, K, counts, copies, device, how, bits, dtype, pair, weights=first)
        a, b = layers["blocks"].step(0), torch.cat(layers["loop"].step(0))
        torch.cuda.synchronize()
        equal = bool(torch.equal(a.view(torch.int16), layers["slabs"].step(0).view(torch.int16)))
        diff, ref = float((a.float() - b.float()).abs().max()), float(b.float().abs().max())
        us, spread, replays = time_forms(layers, args)
        flop = first.flops()
        emit({"what": "input_grad", "shape": name, "bits": bits, "dtype": dt, "pair": pair, "experts": experts, "N": N, "K": K,
              "rows": sum(counts), "counts_min_max": [min(counts), max(counts)], "weight_copies": copies,
              "auto_form": dev.grouped_input_grad_form(experts, sum(counts), N, K, bits, G, first.tid, first.num_sms, dtype, pair),
              "us": us, "blocks_over_slabs": round(us["blocks"] / us["slabs"], 4), "blocks_over_loop": round(us["blocks"] / us["loop"], 4),
              "TFLOPs": {n: round(flop / v * 1e-6, 1) for n, v in us.items()},
              "share_of_2.5PFLOPs": {n: round(flop / (v * 1e-6) / PEAK_FLOPS, 4) for n, v in us.items()},
              "row_blocks": sum(-(-c // 128) for c in counts), "workgroups_with_rows": sum(-(-c // 128) for c in counts) * (K // 256),
              "spread": spread, "flop": flop, "blocks_bits_equal_slabs": equal, "max_abs_diff_blocks_vs_loop": diff,
              "max_abs_loop": ref, "replays_us": replays})
        del layers, first, a, b
        torch.cuda.empty_cache()
    # the threshold sweep: rows / E on both sides of the rule, slabs against blocks, even counts and a routed draw
    for name, experts, N, K in SWEEP_STACKS:
        copies = prefill_copies(experts, N, K, BITS)
        first = None
        for mean in SWEEP_MEANS:
            for spread_name, counts in (("even", even_counts(mean * experts, experts)),
                                        ("routed", ig_counts(mean * experts, experts, seed=mean + experts))):
                layers = {}
                for how in IG_FORMS:
                    layers[how] = InputGrad(experts, N, K, counts, copies, device, how, weights=first)
                    first = first or layers[how]
                us, spread, replays = time_forms(layers, args)
                emit({"what": "threshold sweep", "shape": name, "experts": experts, "N": N, "K": K, "mean_rows_per_expert": mean,
                      "counts": spread_name, "counts_min_max": [min(counts), max(counts)], "rows": sum(counts), "us": us,
                      "blocks_over_slabs": round(us["blocks"] / us["slabs"], 4),
                      "auto_over_best": round(us["auto"] / min(us["slabs"], us["blocks"]), 4), "spread": spread,
                      "auto_form": dev.grouped_input_grad_form(experts, sum(counts), N, K, BITS, G, first.tid, first.num_sms),
                      "replays_us": replays})
                del layers
        del first
        torch.cuda.empty_cache()
    # one backward step of FluteExperts(fused=True, native_routing=True): the input gradients on the slab form (the code before
    # the block form) and on the automatic rule
    copies = prefill_copies(E, 14336, 4096, BITS, stacks=3)
    stacks = step_stacks(copies, device)
    for tokens in (512, 4096):
        layers = {}
        for part in (None, "down_input_grad", "pair_input_grad"):
            for form in ("slabs", None):
                layers[("whole" if part is None else part) + (" slabs" if form else " auto")] = \
                    BackwardStep(stacks, tokens, device, part, ig_form=form)
        us, spread, replays = time_forms(layers, args)
        emit({"what": "backward step", "tokens": tokens, "rows": tokens * TOPK, "experts": E, "top_k": TOPK, "weight_copies": copies,
              "us": us, "whole_auto_over_slabs": round(us["whole auto"] / us["whole slabs"], 4), "spread": spread,
              "replays_us": replays})
    print("wrote", args.out)
    main_swiglu_grad(args, device, stacks, copies)


class CopyYardstick:
    """`copy_` of a 16-bit tensor of 2.5 R F elements: 5 R F bytes read and 5 R F written, the 10 bytes per element of [R, F]
    that swiglu_grad moves (g, u, dh in; dg, du out)."""

    def __init__(self, R, F, device):
        n = 5 * R * F // 2
        self.src = torch.randn(n, device=device, dtype=torch.float32).to(DTYPE)
        self.dst = torch.empty_like(self.src)

    def step(self, i):
        return self.dst.copy_(self.src)


class Gather:
    """The gather in front of the recompute alone: the default backward's index_select on the clamped int64 index, or moe_gather."""

    def __init__(self, step, native):
        self.fa, self.hidden, self.rows, self.offsets, self.native = step.fa, step.hidden, step.rows, step.offsets, native

    def step(self, i):
        if self.native:
            return self.fa.moe_gather(self.hidden, self.rows, self.offsets)
        return self.hidden.index_select(0, self.rows.clamp(0, self.hidden.shape[0] - 1).long())


def main_swiglu_grad(args, device, stacks=None, copies=None):
    """The backward step with native_glu_grad off and on - the gather and `elementwise_dg_du` alone, and the whole step - and the
    copy_ yardstick, all in one run."""
    out = os.path.join(ROOT, "profiles", "grouped_moe_swiglu_grad.json")
    F = 14336
    if stacks is None:
        copies = prefill_copies(E, F, 4096, BITS, stacks=3)
        stacks = step_stacks(copies, device)
    rows = []
    for tokens in (512, 4096):
        layers = {}
        for part in (None, "elementwise_dg_du"):
            for native in (False, True):
                layers[("whole" if part is None else part) + (" native" if native else " torch")] = \
                    BackwardStep(stacks, tokens, device, part, native=native)
        layers["gather torch"], layers["gather native"] = Gather(layers["whole torch"], False), Gather(layers["whole torch"], True)
        layers["copy_ yardstick"] = CopyYardstick(tokens * TOPK, F, device)
        us, spread, replays = time_forms(layers, args)
        part = "elementwise_dg_du"
        rows.append({"what": "backward step, native_glu_grad off / on", "tokens": tokens, "rows": tokens * TOPK, "F": F, "experts": E,
                     "top_k": TOPK, "weight_copies": copies, "us": us,
                     "elementwise_torch_over_native": round(us[part + " torch"] / us[part + " native"], 3),
                     "elementwise_native_over_copy": round(us[part + " native"] / us["copy_ yardstick"], 3),
                     "elementwise_native_TBps": round(10.0 * tokens * TOPK * F / us[part + " native"] * 1e-6, 3),
                     "copy_TBps": round(10.0 * tokens * TOPK * F / us["copy_ yardstick"] * 1e-6, 3),
                     "gather_torch_over_native": round(us["gather torch"] / us["gather native"], 3),
                     "whole_native_over_torch": round(us["whole native"] / us["whole torch"], 4),
                     "whole_torch_minus_native_us": round(us["whole torch"] - us["whole native"], 3),
                     "whole_replay_range_us": {n: [round(min(min(p) for p in replays[n]), 3), round(max(max(p) for p in replays[n]), 3)]
                                               for n in ("whole torch", "whole native")},
                     "spread": spread, "replays_us": replays})
        print(json.dumps({k: v for k, v in rows[-1].items() if k != "replays_us"}), flush=True)
        del layers
        torch.cuda.empty_cache()
        with open(out, "w") as f:
            json.dump({"what": "one backward step of FluteExperts(fused=True, native_routing=True) at Mixtral's shapes (E = 8, top-2, K = 4096, "
                               "F = 14336, W4G64 fp16) by hand, with the gather and the SwiGLU derivative as torch op chains (the default "
                               "backward's arithmetic) and as flute_amd.moe_gather + flute_amd.swiglu_grad (native_glu_grad=True): the two "
                               "parts alone and the whole step, and a copy_ of 2.5 R F 16-bit elements as the yardstick of the same "
                               "traffic; hipGraph replays, device-clock stamps, cold caches, median of the replays, two alternating "
                               "passes of every contender in one process",
                       "config": {"group_size": G, "steps": args.steps, "warmup": args.warmup, "replays": args.replays,
                                  "device": torch.cuda.get_device_name(device)}, "rows": rows}, f, indent=1)
    print("wrote", out)


# ---- --mode router_grad -----------------------------------------------------------------------------------------------

class WeightChain:
    """What follows the unweighted input gradient when row_weight trains: `_grouped_weighted_backward`'s torch lines, or one
    moe_weight_grad launch.  dHp and h [R, K] stand for the input gradient and the weighted launch's input."""

    def __init__(self, R, K, device, native):
        import flute_amd
        self.fa, self.native, self.R = flute_amd, native, R
        gen = torch.Generator(device=device).manual_seed(R)
        self.dhp = (torch.randn(R, K, device=device, generator=gen) / 4).to(DTYPE)
        self.h = torch.randn(R, K, device=device, generator=gen).to(DTYPE)
        self.rw = torch.rand(R, device=device, generator=gen)
        ends = torch.tensor(even_counts(R - 3, E)).cumsum(0)               # three rows no expert serves
        self.offsets = torch.cat([torch.zeros(1, dtype=ends.dtype), ends]).int().to(device)

    def step(self, i):
        if self.native:
            return self.fa.moe_weight_grad(self.dhp, self.h, self.rw, self.offsets)
        R, dev = self.R, self.h.device
        dh = self.dhp.float()
        served = torch.arange(R, device=dev) < self.offsets[-1].clamp(0, R)
        d_weight = torch.where(served, (dh * self.h.float()).sum(dim=1), torch.zeros((), device=dev))
        return d_weight, (self.rw[:, None] * dh).to(self.h.dtype)


class Copy16:
    """`copy_` of `n` 16-bit elements: 2 n bytes read and 2 n written."""

    def __init__(self, n, device):
        self.src = torch.randn(n, device=device, dtype=torch.float32).to(DTYPE)
        self.dst = torch.empty_like(self.src)

    def step(self, i):
        return self.dst.copy_(self.src)


class GateBackward:
    """The backward of a gate-route launch on fp16 logits: `_MoeGateFunction.backward`'s torch lines, or one moe_gate_grad launch."""

    def __init__(self, tokens, shape, device, native):
        import flute_amd
        self.fa, self.native = flute_amd, native
        self.E, self.k, self.scoring, self.renorm, self.scale, groups = shape
        gen = torch.Generator(device=device).manual_seed(tokens)
        self.logits = torch.randn(tokens, self.E, device=device, generator=gen).to(DTYPE)
        if groups is None:
            outs = flute_amd.moe_gate_route(self.logits, self.k, self.E, self.scoring, self.renorm, None, self.scale)
        else:
            outs = flute_amd.moe_gate_route_limited(self.logits, self.k, *groups, self.E, self.scoring, self.renorm, None, self.scale)
        self.ids, self.pos = outs[0], outs[5]
        self.d_weights = torch.zeros(tokens, self.k, device=device)            # (autograd hands zeros for the unused `weights`)
        self.d_row_weight = torch.randn(tokens * self.k, device=device, generator=gen)

    def step(self, i):
        if self.native:
            return self.fa.moe_gate_grad(self.logits, self.ids, self.d_weights, self.scoring, self.renorm, self.scale,
                                         grad_row_weight=self.d_row_weight, pos=self.pos)
        d_weights = self.d_weights + self.d_row_weight.index_select(0, self.pos.reshape(-1).long()).view_as(self.d_weights)
        with torch.enable_grad():
            x = self.logits.detach().float().requires_grad_(True)
            s = torch.softmax(x, dim=1) if self.scoring == "softmax" else torch.sigmoid(x)
            w = s.gather(1, self.ids.long())
            if self.renorm:
                w = w / w.sum(dim=1, keepdim=True)
            (dx,) = torch.autograd.grad(w * self.scale, x, d_weights)
        return dx.to(self.logits.dtype)


class CombineBackward:
    """moe_combine's backward on dOut [T, N]: `_MoeCombineFunction.backward`'s torch lines, or one moe_gather launch on `rows`."""

    def __init__(self, tokens, N, device, native):
        import flute_amd
        self.fa, self.native = flute_amd, native
        ids = torch.rand(tokens, E, generator=torch.Generator().manual_seed(tokens)).topk(TOPK, dim=1).indices.to(device)
        self.offsets, self.rows, _, self.pos, _ = flute_amd.moe_route(ids, None, E)
        self.dOut = torch.randn(tokens, N, device=device, generator=torch.Generator(device=device).manual_seed(tokens)).to(DTYPE)

    def step(self, i):
        if self.native:
            return self.fa.moe_gather(self.dOut, self.rows, self.offsets)
        pos, offsets = self.pos, self.offsets
        T, k = pos.shape
        R, dev = T * k, pos.device
        p = pos.reshape(-1).long()
        inside = (p >= 0) & (p < R)
        token = torch.arange(T, device=dev).repeat_interleave(k)
        rows = torch.full((R + 1,), T, dtype=torch.long, device=dev).scatter_(0, torch.where(inside, p, R), token)[:R]
        named = (rows < T) & (torch.arange(R, device=dev) < offsets[-1].clamp(0, R))
        return self.dOut.index_select(0, rows.clamp(max=T - 1)).masked_fill_(~named[:, None], 0)


class BlockBackward:
    """One forward and backward step of FluteSparseMoeBlock (softmax top-2, renormalised) on copy i of step_stacks with the router
    training: the gradient reaches the hidden states and the router's weight."""

    def __init__(self, stacks, tokens, device, native):
        from flute_amd.integrations import moe
        gen = torch.Generator(device=device).manual_seed(tokens)
        router = (torch.randn(E, 4096, device=device, generator=gen) * 0.02).to(DTYPE)
        self.blocks = [moe.FluteSparseMoeBlock(router.clone(), moe.FluteExperts(g, u, d, fused=True, native_routing=True,
                                                                                native_router_grad=native), TOPK, renormalize=True)
                       for g, u, d in stacks]
        for b in self.blocks:
            b.router_weight.requires_grad_()
        self.hidden = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE).requires_grad_()
        self.dOut = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE)

    def step(self, i):
        block = self.blocks[i % len(self.blocks)]
        return torch.autograd.grad(block(self.hidden), (self.hidden, block.router_weight), self.dOut)


ROUTERS = {"E8 top2 softmax": (8, 2, "softmax", False, 1.0, None),
           "E256 top8 sigmoid n_group8 topk_group4": (256, 8, "sigmoid", True, 2.5, (8, 4))}


def main_router_grad(args, device):
    K, F = 4096, 14336
    copies = prefill_copies(E, F, K, BITS, stacks=3)
    stacks = step_stacks(copies, device)
    rows = []
    for tokens in (512, 4096):
        R = tokens * TOPK
        layers = {"weight chain torch": WeightChain(R, F, device, False), "weight chain native": WeightChain(R, F, device, True),
                  "copy_ yardstick": Copy16(3 * R * F // 2, device),
                  "combine backward torch": CombineBackward(tokens, K, device, False),
                  "combine backward native": CombineBackward(tokens, K, device, True),
                  "block backward off": BlockBackward(stacks, tokens, device, False),
                  "block backward on": BlockBackward(stacks, tokens, device, True)}
        for name, shape in ROUTERS.items():
            layers["gate backward torch, " + name] = GateBackward(tokens, shape, device, False)
            layers["gate backward native, " + name] = GateBackward(tokens, shape, device, True)
        us, spread, replays = time_forms(layers, args)
        row = {"what": "router backward, native_router_grad off / on", "tokens": tokens, "rows": R, "K": K, "F": F, "experts": E,
               "top_k": TOPK, "weight_copies": copies, "us": us,
               "weight_chain_torch_over_native": round(us["weight chain torch"] / us["weight chain native"], 3),
               "weight_chain_native_over_copy": round(us["weight chain native"] / us["copy_ yardstick"], 3),
               "weight_chain_native_TBps": round(6.0 * R * F / us["weight chain native"] * 1e-6, 3),
               "copy_TBps": round(6.0 * R * F / us["copy_ yardstick"] * 1e-6, 3),
               "combine_backward_torch_over_native": round(us["combine backward torch"] / us["combine backward native"], 3),
               "block_on_over_off": round(us["block backward on"] / us["block backward off"], 4),
               "block_off_minus_on_us": round(us["block backward off"] - us["block backward on"], 3),
               "block_replay_range_us": {n: [round(min(min(p) for p in replays[n]), 3), round(max(max(p) for p in replays[n]), 3)]
                                         for n in ("block backward off", "block backward on")},
               "spread": spread, "replays_us": replays}
        for name in ROUTERS:
            row["gate_backward_torch_over_native, " + name] = round(us["gate backward torch, " + name] /
                                                                    us["gate backward native, " + name], 3)
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
        del layers
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "the router's backward at Mixtral's shapes (E = 8, top-2, K = 4096, F = 14336, W4G64 fp16): the weighted "
                               "launch's chain behind the unweighted input gradient as torch ops and as flute_amd.moe_weight_grad, with "
                               "a copy_ of 1.5 R F 16-bit elements as the yardstick of the same traffic; the gate's backward as torch "
                               "ops and as flute_amd.moe_gate_grad for two routers; moe_combine's backward as its torch chain and as "
                               "flute_amd.moe_gather; one whole forward + backward step of FluteSparseMoeBlock(fused=True, "
                               "native_routing=True) with the router training, native_router_grad off and on; hipGraph replays, "
                               "device-clock stamps, cold caches, median of the replays, two alternating passes of every contender in "
                               "one process",
                       "config": {"group_size": G, "steps": args.steps, "warmup": args.warmup, "replays": args.replays,
                                  "device": torch.cuda.get_device_name(device)}, "rows": rows}, f, indent=1)
    print("wrote", args.out)


# ---- --mode aux_loss --------------------------------------------------------------------------------------------------
AUX_ROUTERS = {"E8 top2 softmax": (8, 2, "softmax"), "E256 top8 sigmoid": (256, 8, "sigmoid")}
AUX_TOKENS = (512, 4096, 16384)
AUX_DTYPE = torch.bfloat16                          # what a training router's GEMM hands on (fp16 loses the gradients to subnormals)
AUX_ALPHA, AUX_BETA = 0.01, 0.001


class AuxLoss:
    """The auxiliary losses of `tokens` tokens: flute_amd.moe_aux_loss, or the torch fp32 chain of tests/moe_aux_cases.py; with
    `backward` also the gradient of alpha balance + beta z to the logits."""

    def __init__(self, tokens, shape, device, native, backward):
        import flute_amd
        from tests import moe_aux_cases
        self.fa, self.chain, self.native, self.backward = flute_amd, moe_aux_cases.torch_chain, native, backward
        E_, k, self.scoring = shape
        gen = torch.Generator(device=device).manual_seed(tokens + E_)
        self.logits = (torch.randn(tokens, E_, device=device, generator=gen) * 2).to(AUX_DTYPE)
        self.ids, _ = flute_amd.moe_gate(self.logits, k, self.scoring, True)
        if backward:
            self.logits.requires_grad_()

    def losses(self):
        if self.native:
            return self.fa.moe_aux_loss(self.logits, self.ids, self.scoring)[:2]
        return self.chain(self.logits, self.ids, self.scoring)

    def step(self, i):
        if not self.backward:
            with torch.no_grad():
                return self.losses()
        balance, z = self.losses()
        return torch.autograd.grad(AUX_ALPHA * balance + AUX_BETA * z, self.logits)


class AuxBlock:
    """One training step of FluteSparseMoeBlock (softmax top-2, renormalised) on copy i of step_stacks with the router training and
    alpha balance + beta z in the loss: the block's own aux_loss, or the torch chain bolted on."""

    def __init__(self, stacks, tokens, device, native):
        from flute_amd.integrations import moe
        from tests import moe_aux_cases
        self.chain, self.native = moe_aux_cases.torch_chain, native
        gen = torch.Generator(device=device).manual_seed(tokens)
        router = (torch.randn(E, 4096, device=device, generator=gen) * 0.02).to(DTYPE)
        self.blocks = [moe.FluteSparseMoeBlock(router.clone(), moe.FluteExperts(g, u, d, fused=True, native_routing=True), TOPK,
                                               renormalize=True) for g, u, d in stacks]
        for b in self.blocks:
            b.router_weight.requires_grad_()
            b.aux_loss = native
        self.hidden = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE).requires_grad_()
        self.dOut = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE)
        self.one = torch.ones((), device=device)

    def step(self, i):
        block = self.blocks[i % len(self.blocks)]
        out = block(self.hidden)
        if self.native:
            balance, z = block.aux.balance, block.aux.z
            del block.aux       # it holds this step's autograd graph, as a kept loss does: let go of it before the next step, which
            #                     may run on another stream (a capture) than the one the graph's leaf accumulators were made on
        else:
            logits = torch.nn.functional.linear(self.hidden, block.router_weight)
            balance, z = self.chain(logits, logits.topk(TOPK, dim=1).indices, "softmax")
        loss = AUX_ALPHA * balance + AUX_BETA * z
        del balance, z
        return torch.autograd.grad((out, loss), (self.hidden, block.router_weight), (self.dOut, self.one))


def main_aux_loss(args, device):
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "the router's auxiliary losses (load-balance loss, z-loss) on bf16 logits: flute_amd.moe_aux_loss against "
                               "the torch fp32 chain of tests/moe_aux_cases.py (Hugging Face's load_balancing_loss_func restated, plus "
                               "the z-loss), forward alone and forward + backward to the logits; one training step of "
                               "FluteSparseMoeBlock(fused=True, native_routing=True) at Mixtral's shapes with aux_loss on against the "
                               "same step with the torch chain bolted on.  hipGraph replays of `steps` calls between device-clock "
                               "stamps, cold caches, median of `replays`, every contender timed twice, alternating, one process; "
                               "spread: (max - min) / median over a contender's replays",
                       "config": {"steps": args.steps, "warmup": args.warmup, "replays": args.replays, "logits": "bfloat16",
                                  "alpha": AUX_ALPHA, "beta": AUX_BETA, "device": torch.cuda.get_device_name(device)}, "rows": rows},
                      f, indent=1)

    for name, shape in AUX_ROUTERS.items():
        for tokens in AUX_TOKENS:
            layers = {"%s %s" % (what, who): AuxLoss(tokens, shape, device, who == "native", what == "forward+backward")
                      for what in ("forward", "forward+backward") for who in ("torch", "native")}
            us, spread, replays = time_each(layers, args)
            emit({"what": "aux losses", "router": name, "tokens": tokens, "us": us, "spread": spread,
                  "forward_torch_over_native": round(us["forward torch"] / us["forward native"], 3),
                  "forward_backward_torch_over_native": round(us["forward+backward torch"] / us["forward+backward native"], 3),
                  "replays_us": replays})
            del layers
    copies = prefill_copies(E, 14336, 4096, BITS, stacks=3)
    stacks = step_stacks(copies, device)
    for tokens in (512, 4096):
        layers = {"block step, torch chain": AuxBlock(stacks, tokens, device, False), "block step, aux_loss": AuxBlock(stacks, tokens, device, True)}
        us, spread, replays = time_each(layers, args)
        emit({"what": "FluteSparseMoeBlock training step with the auxiliary losses, Mixtral shapes", "tokens": tokens, "experts": E,
              "top_k": TOPK, "us": us, "spread": spread, "weight_copies": copies,
              "aux_loss_over_torch_chain": round(us["block step, aux_loss"] / us["block step, torch chain"], 4),
              "torch_chain_minus_aux_loss_us": round(us["block step, torch chain"] - us["block step, aux_loss"], 3),
              "replays_us": replays})
        del layers
        torch.cuda.empty_cache()
    print("wrote", args.out)


# ---- --mode route_wide ------------------------------------------------------------------------------------------------
WIDE_ROUTERS = {"E8 top2 softmax": dict(E=8, k=2, scoring="softmax", bias=False, scale=1.0, groups=None),
                "E64 top8 softmax": dict(E=64, k=8, scoring="softmax", bias=False, scale=1.0, groups=None),
                "E256 top8 sigmoid bias n_group8 topk_group4 top2sum": dict(E=256, k=8, scoring="sigmoid", bias=True, scale=2.5,
                                                                            groups=(8, 4, "top2sum"))}
WIDE_TOKENS = (16, 64, 256, 1024, 4096, 16384)
WIDE_SWEEP_TOKENS = (1024, 4096)
WIDE_GATED_CHUNKS = (16, 32, 64, 128, 256)
WIDE_UNGATED_PAIRS = (512, 1024, 2048, 4096)


class WideRouting:
    """One routing of `tokens` tokens for a router of WIDE_ROUTERS; step(i) returns `pos`.  form: "one" (a), "two" (b), "wide" (c),
    "route" / "route_wide" (d); chunk_tokens: the wide forms' (None: automatic)."""

    def __init__(self, tokens, router, device, form, chunk_tokens=None):
        import flute_amd
        self.fa, self.r, self.form, self.chunk = flute_amd, router, form, chunk_tokens
        gen = torch.Generator(device=device).manual_seed(tokens + router["E"])
        self.logits = (torch.randn(tokens, router["E"], device=device, generator=gen) * 2).to(DTYPE)
        self.bias = torch.randn(router["E"], device=device, generator=gen) * 0.1 if router["bias"] else None
        if form in ("route", "route_wide"):
            self.ids, self.weights = self.gate(routed=False)

    def gate(self, routed, wide=False):
        r, fa = self.r, self.fa
        tail = (r["scoring"], True, self.bias, r["scale"])
        if wide:
            return fa.moe_gate_route_wide(self.logits, r["k"], r["E"], *tail, *(r["groups"] or (1, 1, "max")), chunk_tokens=self.chunk)
        if r["groups"] is None:
            return fa.moe_gate_route(self.logits, r["k"], r["E"], *tail) if routed else fa.moe_gate(self.logits, r["k"], *tail)
        n_group, topk_group, group_score = r["groups"]
        if routed:
            return fa.moe_gate_route_limited(self.logits, r["k"], n_group, topk_group, r["E"], *tail, group_score)
        return fa.moe_gate_limited(self.logits, r["k"], n_group, topk_group, *tail, group_score)

    def step(self, i):
        if self.form == "one":
            return self.gate(routed=True)[5]
        if self.form == "wide":
            return self.gate(routed=True, wide=True)[5]
        if self.form == "two":
            return self.fa.moe_route(*self.gate(routed=False), self.r["E"])[3]
        if self.form == "route":
            return self.fa.moe_route(self.ids, self.weights, self.r["E"])[3]
        return self.fa.moe_route_wide(self.ids, self.weights, self.r["E"], chunk_tokens=self.chunk)[3]


class WideBlock:
    """One forward of FluteSparseMoeBlock (softmax top-2, renormalised) on copy i of step_stacks."""

    def __init__(self, stacks, tokens, device, wide_routing):
        from flute_amd.integrations import moe
        gen = torch.Generator(device=device).manual_seed(tokens)
        router = (torch.randn(E, 4096, device=device, generator=gen) * 0.02).to(DTYPE)
        self.blocks = [moe.FluteSparseMoeBlock(router, moe.FluteExperts(g, u, d, fused=True, native_routing=True,
                                                                        wide_routing=wide_routing), TOPK, renormalize=True)
                       for g, u, d in stacks]
        self.hidden = torch.randn(tokens, 4096, device=device, generator=gen).to(DTYPE)

    def step(self, i):
        with torch.no_grad():
            return self.blocks[i % len(self.blocks)](self.hidden)


def time_each(layers, args):
    """time_forms with every contender's own spread: ({name: mean of its two medians}, {name: (max - min) / median over its ten
    replays}, the passes)."""
    us, _, replays = time_forms(layers, args)
    spread = {}
    for n, passes in replays.items():
        flat = sorted(r for p in passes for r in p)
        spread[n] = round((flat[-1] - flat[0]) / flat[len(flat) // 2], 4)
    return us, spread, replays


def main_route_wide(args, device):
    from flute_amd import dev
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "the MoE routing at prefill and training token counts, fp16 logits, renormalised: (a) one = "
                               "moe_gate_route[_limited], one workgroup; (b) two = moe_gate[_limited] + moe_route; (c) wide = "
                               "moe_gate_route_wide, automatic chunk; (d) route / route_wide = moe_route against moe_route_wide on "
                               "given ids and weights; the chunk_tokens sweeps; one forward of FluteSparseMoeBlock(fused=True, "
                               "native_routing=True) at Mixtral's shapes, wide_routing off against auto.  hipGraph replays of `steps` "
                               "calls between device-clock stamps, cold caches, median of `replays`, every contender timed twice, "
                               "alternating, one process; spread: (max - min) / median over a contender's replays",
                       "config": {"steps": args.steps, "warmup": args.warmup, "replays": args.replays, "dtype": "float16",
                                  "device": torch.cuda.get_device_name(device)}, "rows": rows}, f, indent=1)

    for name, router in WIDE_ROUTERS.items():
        for tokens in WIDE_TOKENS:
            layers = {f: WideRouting(tokens, router, device, f) for f in ("one", "two", "wide", "route", "route_wide")}
            same = all(torch.equal(a, b) for a, b in zip(layers["one"].gate(True), layers["wide"].gate(True, wide=True)))
            us, spread, replays = time_each(layers, args)
            best = min(us["one"], us["two"])
            emit({"what": "routing", "router": name, "tokens": tokens, "pairs": tokens * router["k"], "us": us, "spread": spread,
                  "wide_equals_one_bitwise": same, "wide_over_best_of_one_two": round(us["wide"] / best, 4),
                  "route_wide_over_route": round(us["route_wide"] / us["route"], 4),
                  "rule_gated": dev.moe_route_form(tokens, router["k"], router["E"], gated=True),
                  "rule_ungated": dev.moe_route_form(tokens, router["k"], router["E"], gated=False), "replays_us": replays})
    for name, router in WIDE_ROUTERS.items():
        for tokens in WIDE_SWEEP_TOKENS:
            layers = {"wide chunk %d" % c: WideRouting(tokens, router, device, "wide", c) for c in WIDE_GATED_CHUNKS}
            layers.update({"route_wide pairs %d" % p: WideRouting(tokens, router, device, "route_wide", max(1, p // router["k"]))
                           for p in WIDE_UNGATED_PAIRS})
            us, spread, replays = time_each(layers, args)
            emit({"what": "chunk sweep", "router": name, "tokens": tokens, "us": us, "spread": spread, "replays_us": replays})
    copies = prefill_copies(E, 14336, 4096, BITS, stacks=3)
    stacks = step_stacks(copies, device)
    for tokens in (512, 4096):
        layers = {"wide_routing off": WideBlock(stacks, tokens, device, False), "wide_routing auto": WideBlock(stacks, tokens, device, "auto")}
        same = torch.equal(layers["wide_routing off"].step(0), layers["wide_routing auto"].step(0))
        us, spread, replays = time_each(layers, args)
        emit({"what": "FluteSparseMoeBlock forward, Mixtral shapes", "tokens": tokens, "experts": E, "top_k": TOPK, "us": us,
              "spread": spread, "rule": dev.moe_route_form(tokens, TOPK, E, gated=True), "auto_equals_off_bitwise": same,
              "auto_over_off": round(us["wide_routing auto"] / us["wide_routing off"], 4), "weight_copies": copies,
              "replays_us": replays})
    print("wrote", args.out)


def main_input_grad(args):
    """`--processes` fresh child processes one after the other; per row the median of the processes' figures and the largest
    spread of any pass in any process."""
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(args.processes):
            path = os.path.join(tmp, "p%d.json" % i)
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", args.mode, "--child", "--out", path, "--steps",
                   str(args.steps), "--warmup", str(args.warmup), "--replays", str(args.replays)]
            subprocess.run(cmd, check=True)
            with open(path) as f:
                runs.append(json.load(f))
    median = lambda v: sorted(v)[len(v) // 2]
    rows = []
    for i, first in enumerate(runs[0]["rows"]):
        per = [r["rows"][i] for r in runs]
        if first["what"] == "table_grad":
            us = {f: median([p[f + "_us"] for p in per]) for f in TG_FORMS}
            row = {k: first[k] for k in ("what", "shape", "experts", "N", "K", "rows", "counts_min_max", "weight_copies", "flop",
                                         "scratch_bytes")}
            row.update({f + "_us": us[f] for f in TG_FORMS})
            row.update(table_over_loop=round(us["table"] / us["loop"], 4),
                       fused_over_separate=round(us["fused"] / us["separate"], 4),
                       fused_over_table=round(us["fused"] / us["table"], 4),
                       table_TFLOPs=round(first["flop"] / us["table"] * 1e-6, 1), loop_TFLOPs=round(first["flop"] / us["loop"] * 1e-6, 1),
                       spread=max(p["spread"] for p in per),
                       per_process_us={f: [p[f + "_us"] for p in per] for f in TG_FORMS},
                       max_abs_diff_grouped_vs_loop=max(p["max_abs_diff_grouped_vs_loop"] for p in per),
                       max_abs_loop=first["max_abs_loop"], replays_us=[[q["replays_us"] for q in p["passes"]] for p in per])
        elif first["what"] == "scale_grad":
            g_us, l_us = median([p["grouped_us"] for p in per]), median([p["loop_us"] for p in per])
            row = {k: first[k] for k in ("what", "shape", "experts", "N", "K", "rows", "counts_min_max", "weight_copies", "flop")}
            row.update(grouped_us=g_us, loop_us=l_us, grouped_over_loop=round(g_us / l_us, 4),
                       grouped_TFLOPs=round(first["flop"] / g_us * 1e-6, 1), loop_TFLOPs=round(first["flop"] / l_us * 1e-6, 1),
                       grouped_share_of_2_5_PFLOPs=round(first["flop"] / (g_us * 1e-6) / PEAK_FLOPS, 4),
                       loop_share_of_2_5_PFLOPs=round(first["flop"] / (l_us * 1e-6) / PEAK_FLOPS, 4),
                       spread=max(p["spread"] for p in per), per_process_grouped_us=[p["grouped_us"] for p in per],
                       per_process_loop_us=[p["loop_us"] for p in per],
                       max_abs_diff_grouped_vs_loop=max(p["max_abs_diff_grouped_vs_loop"] for p in per),
                       max_abs_loop=first["max_abs_loop"], replays_us=[[q["replays_us"] for q in p["passes"]] for p in per])
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "replays_us"}), flush=True)
    what = {"scale_grad": "grouped scale gradient (one launch) vs a per-expert loop of the dense qgemm_scale_grad with host-known row "
                          "counts; hipGraph replays, device-clock stamps, cold caches; passes per process: grouped, loop, grouped, loop",
            "table_grad": "grouped table gradient (main launch + reduce): dT2 alone (table), dT2 + dS in the same launch pair (fused), "
                          "qgemm_grouped_scale_grad followed by the dT2-only pair (separate), and a per-expert loop of the dense "
                          "qgemm_table_grad with host-known row counts (loop, dT2 only); hipGraph replays, device-clock stamps, cold "
                          "caches; passes per process: table, fused, separate, loop, twice"}
    out = {"what": what[args.mode],
           "config": {"bits": BITS, "group_size": G, "dtype": "float16", "steps": args.steps, "warmup": args.warmup,
                      "replays": args.replays, "processes": args.processes, "device": runs[0]["device"]},
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


def measure(layer, args):
    us, _ = bench.time_graph(layer, args.steps, args.warmup, torch.cuda.synchronize, cold=True, replays=args.replays)
    t = dict(bench.LAST_TIMING)
    per = [r * 1e3 / args.steps for r in t["replays_ms"]]
    return {"us": us * 1e3 / args.steps, "replays_us": [round(p, 3) for p in per],
            "spread": round((max(per) - min(per)) / (us * 1e3 / args.steps), 4), "clock": t["clock"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--tokens", type=int, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--bits", type=int, choices=[2, 3, 4], default=BITS, help="--mode projection: the bit width")
    ap.add_argument("--mode", choices=["projection", "mlp", "step", "gate", "gate_limited", "input_grad", "scale_grad", "table_grad",
                                       "prefill", "router_grad", "route_wide", "aux_loss"],
                    default="projection")
    ap.add_argument("--routing-tokens", type=int, nargs="*", default=[1, 16, 64], help="--mode step / gate: the rows without the GEMMs")
    ap.add_argument("--processes", type=int, default=3, help="--mode step / gate: fresh processes, one after the other")
    ap.add_argument("--child", action="store_true", help="--mode step / gate: one of those processes (internal)")
    ap.add_argument("--only", nargs="*", choices=PREFILL_SECTIONS, default=None,
                    help="--mode prefill: the sections to run (default: all) - " + ", ".join(PREFILL_SECTIONS))
    ap.add_argument("--only-swiglu-grad", action="store_true",
                    help="--mode input_grad: its last section alone, the backward step with native_glu_grad off and on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"projection": "grouped_moe.json", "mlp": "grouped_moe_fused.json",
                                                   "step": "grouped_moe_routing.json", "gate": "grouped_moe_gate.json",
                                                   "gate_limited": "grouped_moe_gate_limited.json",
                                                   "input_grad": "grouped_moe_input_grad_blocks.json",
                                                   "scale_grad": "grouped_moe_scale_grad.json",
                                                   "table_grad": "grouped_moe_table_grad.json",
                                                   "prefill": "grouped_moe_prefill.json",
                                                   "router_grad": "grouped_moe_router_grad.json",
                                                   "route_wide": "grouped_moe_route_wide.json",
                                                   "aux_loss": "grouped_moe_aux_loss.json"}[args.mode])
    if args.mode in ("scale_grad", "table_grad"):
        if not args.child:
            return main_input_grad(args)             # the parent never opens the GPU
        device = torch.device("cuda", 0)
        torch.cuda.set_device(device)
        child = {"scale_grad": child_scale_grad, "table_grad": child_table_grad}
        return child[args.mode](args, device)
    if args.mode in ("step", "gate") and not args.child:
        return main_step(args)                       # the parent never opens the GPU
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    if args.mode == "step":
        return child_step(args, device)
    if args.mode == "gate":
        return child_gate(args, device)
    if args.mode == "gate_limited":
        return main_gate_limited(args, device)
    if args.mode == "mlp":
        return main_mlp(args, device)
    if args.mode == "prefill":
        return main_prefill(args, device)
    if args.mode == "router_grad":
        return main_router_grad(args, device)
    if args.mode == "route_wide":
        return main_route_wide(args, device)
    if args.mode == "aux_loss":
        return main_aux_loss(args, device)
    if args.mode == "input_grad":
        return main_swiglu_grad(args, device) if args.only_swiglu_grad else main_input_grad_forms(args, device)
    rows = []
    bits = args.bits
    for name, N, K in (("gate_up", 14336, 4096), ("down", 4096, 14336)):
        per_copy = E * ((bits * N // 16) * K * 2 + N * (K // G) * 2)
        copies = max(2, bench.L3_BYTES // per_copy + 2)
        for tokens in args.tokens:
            counts = routing(tokens, seed=tokens)
            grouped = Experts(N, K, counts, copies, device, grouped=True, bits=bits)
            try:
                loop, no_loop = Experts(N, K, counts, copies, device, grouped=False, bits=bits), None
            except LookupError as err:
                loop, no_loop = None, str(err)
            nbytes = grouped.bytes()
            row = {"projection": name, "bits": bits, "N": N, "K": K, "tokens": tokens, "rows": sum(counts), "counts": counts,
                   "weight_copies": copies}
            if loop is None:
                # the grouped form alone, the same two passes
                grouped.step(0)
                torch.cuda.synchronize()
                m = [measure(grouped, args) for _ in range(2)]
                g_us = (m[0]["us"] + m[1]["us"]) / 2
                row.update({"grouped_us": round(g_us, 3), "loop_us": None, "loop_not_timed": no_loop, "bytes": nbytes,
                            "grouped_GBps": round(nbytes / g_us * 1e-3, 1),
                            "grouped_share_of_8TBps": round(nbytes / (g_us * 1e-6) / PEAK, 4), "passes": m})
            else:
                a = torch.cat([grouped.step(0)[grouped.off_host[e]:grouped.off_host[e + 1]] for e in range(E)])
                b = torch.cat(loop.step(0))
                torch.cuda.synchronize()
                # two passes of each, alternating; the figure is the mean of each form's two medians
                m = [measure(layer, args) for layer in (grouped, loop, grouped, loop)]
                g_us, l_us = (m[0]["us"] + m[2]["us"]) / 2, (m[1]["us"] + m[3]["us"]) / 2
                row.update({"grouped_us": round(g_us, 3), "loop_us": round(l_us, 3),
                            "grouped_over_loop": round(g_us / l_us, 4), "bytes": nbytes,
                            "grouped_GBps": round(nbytes / g_us * 1e-3, 1), "loop_GBps": round(nbytes / l_us * 1e-3, 1),
                            "grouped_share_of_8TBps": round(nbytes / (g_us * 1e-6) / PEAK, 4),
                            "loop_share_of_8TBps": round(nbytes / (l_us * 1e-6) / PEAK, 4),
                            "loop_launches": sum(1 for c in counts if c), "loop_templates": loop.tid_loop,
                            "max_abs_diff_grouped_vs_loop": float((a.float() - b.float()).abs().max()),
                            "passes": m})
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "passes"}), flush=True)
            del grouped, loop
            torch.cuda.empty_cache()
    out = {"what": "grouped qgemm vs per-expert qgemm loop, hipGraph replays, device-clock stamps, cold caches",
           "config": {"bits": bits, "group_size": G, "experts": E, "top_k": TOPK, "dtype": "float16",
                      "steps": args.steps, "warmup": args.warmup, "replays": args.replays,
                      "device": torch.cuda.get_device_name(device)},
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
