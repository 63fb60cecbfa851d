"""Seeded launches of the lean decode kernel (flute_amd/csrc/qgemm_fast.h), one per instantiated shape.

Every (waves, waves per unit row, pieces per wave) x rows per pass the library instantiates, both dtypes and both TileP, with the
group size cycling through 64 / 128 / 256.  The inputs are built from integers on the host (numpy's seeded generator, then exact
or round-to-nearest conversions), so every host builds the same bits.  The table is NF4: partial sums round, so the kernel's output
depends on the order of its fp32 arithmetic, and a stored output pins that order.

tests/golden/make_fast_loop.py stores the outputs (tests/golden/fast_loop/fast_loop.npz); tests/test_fast_loop_gpu.py compares."""
import numpy as np
import torch

# (waves, kw, pieces per wave, rows per pass): inst_oneshot_fast_b4.hip's FLUTE_FAST_SHAPES
SHAPES = [(4, 1, 4, 1), (4, 1, 8, 1), (8, 2, 4, 1), (8, 2, 8, 1), (4, 1, 7, 1),
          (4, 1, 4, 2), (4, 1, 8, 2), (8, 2, 4, 2), (8, 2, 8, 2), (4, 1, 7, 2),
          (4, 1, 4, 4), (4, 1, 8, 4), (8, 2, 4, 4), (4, 1, 7, 4)]
N = 512


def cases():
    """(name, dtype, tile_p, waves, kw, depth, mb, M, K, g, seed)"""
    out = []
    i = 0
    for dtype in (torch.float16, torch.bfloat16):
        for tile_p in (32, 64):
            for (w, kw, d, mb) in SHAPES:
                for M in ((3, 4) if mb == 4 else (mb,)):
                    K = 512 * d * kw
                    g = (64, 128, 256)[i % 3]
                    name = f"{'f16' if dtype == torch.float16 else 'bf16'}_tp{tile_p}_w{w}_kw{kw}_d{d}_mb{mb}_m{M}_g{g}"
                    out.append((name, dtype, tile_p, w, kw, d, mb, M, K, g, 1000 + i))
                    i += 1
    return out


def template_id(fa, tile_p):
    return min(t for (b, t), c in fa.TEMPLATE_CONFIGS.items() if b == 4 and c["TileP"] == tile_p)


def inputs(fa, utils, O, dtype, tile_p, M, K, g, seed, num_sms):
    """Host tensors (X, Q, S, table, table2) of one case."""
    rng = np.random.default_rng(seed)
    codes = torch.from_numpy(rng.integers(0, 16, (K, N), dtype=np.int64).astype(np.uint8))
    smag = rng.integers(512, 2048, (N, K // g))
    ssgn = rng.integers(0, 2, (N, K // g)) * 2 - 1
    S = torch.from_numpy(smag * ssgn / 16384.0).to(dtype)
    X = torch.from_numpy(rng.integers(-30000, 30001, (M, K)) / 8192.0).to(dtype)
    table = torch.tensor(O.NF4_VALUES, dtype=dtype)
    table2 = utils.make_qmap2_from_qmap(table)
    Q = utils.pack(codes, 4, [template_id(fa, tile_p)], num_sms)
    return X, Q, S, table, table2


def overrides(dev, waves):
    return dev.Overrides(family=0, one_shot=4, waves=waves)


def run(fa, dev, utils, O, case, num_sms, ws, device, ovr=None):
    """The kernel's output [M, N] of one case (the lean kernel unless `ovr` says otherwise), on the host."""
    (name, dtype, tile_p, w, kw, d, mb, M, K, g, seed) = case
    X, Q, S, table, table2 = inputs(fa, utils, O, dtype, tile_p, M, K, g, seed, num_sms)
    tid = template_id(fa, tile_p)
    o = ovr if ovr is not None else overrides(dev, w)
    if ovr is None:
        plan = dev.get_plan(M, N, K, 4, g, tid, num_sms, dtype, o)
        assert (plan["family"], plan["one_shot"], plan["waves"], plan["kw"], plan["ring_depth"], plan["m_block"]) == (0, 4, w, kw, d, mb), (name, plan)
    return dev.qgemm_planned(X.to(device), Q.to(device), S.to(device), table.to(device), table2.to(device), ws, 4, g, tid,
                             num_sms, o).cpu()
