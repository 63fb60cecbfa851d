"""What the tests of the multi-workgroup routing (flute_moe_route_wide / flute_moe_gate_route_wide, moe_route_wide.hip) share:
the list of shapes, the header's constants and the automatic chunk restated from them, a numpy model of the three launches
with the kernel's own range arithmetic, and the direct ABI calls with every output and the workspace canary-padded and
the workspace poisoned."""
import itertools
import os
import re

import numpy as np
import torch

from tests.moe_cases import (CANARY, DTYPE_CODE, F32, I32, SCORING_CODE, canary_padded, draw_bias, draw_logits,  # noqa: F401
                             host_route, intact, same_bits)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")
WAVES, STEP = 16, 64                    # moe_route_sort.h: kRouteWaves, the pairs a wave takes per step
ID_CODE = {torch.int32: 0, torch.int64: 1}
GROUP_SCORE_CODE = {"max": 0, "top2sum": 1}

# (T, k, E, chunk_tokens); None: the automatic chunk
ROUTE_WIDE_CASES = [
    (2, 1, 1, 1),                       # two chunks of one pair
    (37, 2, 4, 16),                     # three chunks, a ragged last one, an expert never chosen
    (33, 3, 3, 1),                      # 33 chunks smaller than one wave step, k not a power of two
    (261, 8, 256, 16),                  # 17 chunks
    (300, 8, 8, 160),                   # 1280 pairs per chunk: the waves walk their range twice
    (40, 4, 1024, 16),                  # LDS above 64 KB
    (1030, 2, 8, None),                 # the automatic chunk
    (37, 2, 4, 64),                     # C = 1: the delegated launch
    (5, 2, 0, 2),                       # no experts
    (0, 2, 6, 4),                       # no tokens: the zeros
]
# (T, E, k, chunk_tokens) of the gated form
GATE_WIDE_CASES = [(5, 60, 4, 2), (37, 64, 8, 16), (3, 256, 8, 1), (2, 1000, 64, 1), (1030, 8, 2, None)]


def header_constant(name):
    with open(HEADER) as f:
        return int(re.search(r"#define %s (\d+)" % name, f.read()).group(1))


def auto_chunk(gated, T, k):
    """flute_amd.h's automatic chunk_tokens, restated from its constants."""
    want = header_constant("FLUTE_MOE_GATE_ROUTE_WIDE_TOKENS") if gated else -(-header_constant("FLUTE_MOE_ROUTE_WIDE_PAIRS") // max(k, 1))
    return max(want, -(-T // header_constant("FLUTE_MOE_ROUTE_MAX_CHUNKS")))


def draw_wide_ids(T, k, E, chunk_tokens, seed):
    """Random ids with some outside [0, E) in it; (37, 2, 4): expert 2 is never chosen."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, max(E, 1), (T, k), generator=gen)
    if (T, k, E) == (37, 2, 4):
        ids = torch.tensor([0, 1, 3])[torch.randint(0, 3, (T, k), generator=gen)]
    if T * k >= 2:
        ids.view(-1)[0], ids.view(-1)[-1] = -1, E
    if T * k > 40:
        ids.view(-1)[torch.randperm(T * k, generator=gen)[:T * k // 20]] = E + 3
    return ids


def wave_range(lo, hi, w):
    """route_wave_range: wave w's share of the chunk [lo, hi)."""
    per = ((-(-(hi - lo) // WAVES) + STEP - 1) // STEP) * STEP
    begin = lo + w * per
    return begin, max(begin, min(hi, begin + per))


def model_route_wide(ids, T, k, E, chunk_tokens):
    """The three launches on the flattened ids (Python ints): per chunk and wave the count, the column scan over the chunks,
    then the place with row = tot[b] + hist[c][b] + cnt[w][b] + rank.  Returns offsets, perm, rows, pos as lists."""
    B, P = E + 1, T * k
    bucket = np.array([v if 0 <= v < E else E for v in ids], dtype=np.int64)
    C = -(-T // chunk_tokens)
    chunks = [(c * chunk_tokens * k, min(T, (c + 1) * chunk_tokens) * k) for c in range(C)]
    # launch 1: hist[c][b], from the per-wave counts
    cnt = np.zeros((C, WAVES, B), dtype=np.int64)
    for c, (lo, hi) in enumerate(chunks):
        for w in range(WAVES):
            begin, end = wave_range(lo, hi, w)
            np.add.at(cnt[c, w], bucket[begin:end], 1)
    hist = cnt.sum(axis=1)
    assert int(hist.sum()) == P, "every pair is in exactly one wave's range"
    # launch 2: the exclusive prefix of every column over the chunks, and the totals
    total = hist.sum(axis=0)
    before = np.cumsum(hist, axis=0) - hist
    # launch 3: the bucket scan, the waves' prefix started at before[c][b], the place
    tot = np.cumsum(total) - total
    perm, pos = [-1] * P, [-1] * P
    for c, (lo, hi) in enumerate(chunks):
        run = before[c] + np.cumsum(cnt[c], axis=0) - cnt[c]                   # [WAVES, B]
        for w in range(WAVES):
            begin, end = wave_range(lo, hi, w)
            for s in range(begin, end, STEP):
                step = bucket[s:min(end, s + STEP)]
                for lane, b in enumerate(step):
                    rank = int((step[:lane] == b).sum())
                    i = int(tot[b] + run[w, b] + rank)
                    assert perm[i] == -1, "two pairs on one row"
                    perm[i], pos[s + lane] = s + lane, i
                for b, n in zip(*np.unique(step, return_counts=True)):
                    run[w, b] += n
    return tot.tolist(), perm, [p // k for p in perm], pos


_poison = itertools.cycle((-1, 0x5A5A5A5A))         # 0xFF bytes on one call, 0x5A on the next


def poisoned_workspace(env, nbytes):
    """(buffer, view): nbytes (a multiple of 4) of workspace between canaries, every word poisoned so that a word the launches
    read without having written it shows in the outputs."""
    buf, view = canary_padded(nbytes // 4, I32, env.dev)
    view.fill_(next(_poison))
    return buf, view


def route_wide_abi(env, ids, weights, E, chunk_tokens, workspace=None):
    """flute_moe_route_wide with every output in the middle of a larger buffer: (offsets, rows, row_weight, pos, perm)."""
    d, lib = env.dev, env.lib
    T, k = ids.shape
    P = T * k
    sizes = dict(offsets=E + 1, perm=P, rows=P, row_weight=P, pos=P)
    bufs = {n: canary_padded(s, F32 if n == "row_weight" else I32, d) for n, s in sizes.items()}
    ptr = lambda n: bufs[n][1].data_ptr() if sizes[n] else None
    ct = 0 if chunk_tokens is None else chunk_tokens
    nbytes = lib.flute_moe_route_wide_workspace(T, k, E, ct)
    assert nbytes > 0 and nbytes % 4 == 0
    ws_buf, ws = poisoned_workspace(env, nbytes) if workspace is None else workspace
    assert ws.numel() * 4 >= nbytes
    with torch.cuda.device(d):
        rc = lib.flute_moe_route_wide(
            ID_CODE[ids.dtype], 0 if weights is None else DTYPE_CODE[weights.dtype], T, k, E, ids.data_ptr() or None,
            None if weights is None else weights.data_ptr(), bufs["offsets"][1].data_ptr(), ptr("perm"), ptr("rows"),
            None if weights is None else ptr("row_weight"), ptr("pos"), ws.data_ptr(), nbytes, ct,
            torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for n, s in sizes.items():
        assert intact(bufs[n][0], s), "canary around " + n
    assert intact(ws_buf, ws.numel()), "canary around the workspace"
    if weights is None:
        assert bool(torch.all(bufs["row_weight"][0] == CANARY)), "row_weight written without weights"
    out = {n: bufs[n][1] for n in sizes}
    return out["offsets"], out["rows"], None if weights is None else out["row_weight"], out["pos"].view(T, k), out["perm"]


def gate_route_wide_abi(env, logits, k, chunk_tokens, scoring="softmax", renormalize=False, bias=None, scale=1.0, n_group=1,
                        topk_group=1, group_score="max"):
    """flute_moe_gate_route_wide with every output in the middle of a larger buffer: (ids, weights, offsets, rows, row_weight,
    pos, perm)."""
    d, lib = env.dev, env.lib
    T, E = logits.shape
    P = T * k
    sizes = dict(ids=P, weights=P, offsets=E + 1, perm=P, rows=P, row_weight=P, pos=P)
    bufs = {n: canary_padded(s, F32 if n in ("weights", "row_weight") else I32, d) for n, s in sizes.items()}
    ct = 0 if chunk_tokens is None else chunk_tokens
    nbytes = lib.flute_moe_route_wide_workspace(T, k, E, ct)
    assert nbytes > 0 and nbytes % 4 == 0
    ws_buf, ws = poisoned_workspace(env, nbytes)
    with torch.cuda.device(d):
        rc = lib.flute_moe_gate_route_wide(
            DTYPE_CODE[logits.dtype], T, E, k, n_group, topk_group, GROUP_SCORE_CODE[group_score], SCORING_CODE[scoring],
            int(renormalize), float(scale), logits.data_ptr(), None if bias is None else bias.data_ptr(),
            *(bufs[n][1].data_ptr() for n in ("ids", "weights", "offsets", "perm", "rows", "row_weight", "pos")),
            ws.data_ptr(), nbytes, ct, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for n, s in sizes.items():
        assert intact(bufs[n][0], s), "canary around " + n
    assert intact(ws_buf, ws.numel()), "canary around the workspace"
    out = {n: bufs[n][1] for n in sizes}
    return (out["ids"].view(T, k), out["weights"].view(T, k), out["offsets"], out["rows"], out["row_weight"],
            out["pos"].view(T, k), out["perm"])
