"""GPU parity tests: the HIP path (through torch.ops.flute.* -> C ABI) against the
CPU oracle, the committed golden fixtures, and size-independent properties at
BASELINE.json's full shapes.  Mirrors the reference's own tests
(tests/kernel.py::test_integer, tests/higgs.py::test_vector_dequantize).

Tolerances: rel-Frobenius < 1e-3 for fp16 (north_star) and < 4e-3 for bf16
(one bf16 ulp is 2^-8; the reference accepts 1.1e-2, tests/kernel.py:13);
identity input must reproduce round_T(table*scale) exactly.
"""
import os

import numpy as np
import pytest
import torch

from tests import exact_cases as XC
from tests.support import env, norm_rel_err  # noqa: F401

pytestmark = pytest.mark.gpu

FP16_TOL = 1e-3
BF16_TOL = 4e-3


def tol_of(dtype):
    return FP16_TOL if dtype == torch.float16 else BF16_TOL


def template_ids_for(fa, bits, tile_p, limit=None):
    ids = [t for (b, t), c in sorted(fa.TEMPLATE_CONFIGS.items()) if b == bits and c["TileP"] == tile_p]
    return ids if limit is None else ids[:limit]


def run_qgemm(e, X, Q, S, table, table2, bits, g, tid, ovr=None):
    d = e.dev
    if ovr is not None:       # per-call launch-plan override (flute_qgemm_ex)
        from flute_amd import dev
        return dev.qgemm_planned(X.to(d), torch.as_tensor(Q).to(d), S.to(d), table.to(d), table2.to(d),
                                 e.ws, bits, g, tid, e.num_sms, dev.Overrides(**ovr)).cpu()
    return e.fa.qgemm(X.to(d), torch.as_tensor(Q).to(d), S.to(d), table.to(d), table2.to(d),
                      e.ws, bits, g, tid, e.num_sms).cpu()


# ---------------------------------------------------------------------------
# golden fixtures (produced by the reference's own packers / formulas)
# ---------------------------------------------------------------------------


def test_golden_identity_exact(env, golden):
    # tests/kernel.py:30-36,105-107 and tests/higgs.py:103-104
    K = golden.Q.shape[1]
    I = torch.eye(K, dtype=golden.dtype)
    # one template per (SMs_Multiple, tile, lut mode) family with the fixture's TileP
    tids = template_ids_for(env.fa, golden.num_bits, golden.tile_p)
    for tid in tids[:: max(1, len(tids) // 6)]:
        D = run_qgemm(env, I, golden.Q, golden.S, golden.table, golden.table2,
                      golden.num_bits, golden.group_size, tid)
        assert torch.equal(D, golden.D_identity), (golden.name, tid)


def test_golden_random(env, golden):
    if golden.kind != "kernel":
        pytest.skip("HIGGS fixtures pin the identity case")
    tid = template_ids_for(env.fa, golden.num_bits, golden.tile_p)[0]
    D = run_qgemm(env, golden.A, golden.Q, golden.S, golden.table, golden.table2,
                  golden.num_bits, golden.group_size, tid)
    assert norm_rel_err(D, golden.D) < tol_of(golden.dtype), golden.name


# ---------------------------------------------------------------------------
# seeded random vs the oracle (tests/kernel.py::test_integer distributions)
# ---------------------------------------------------------------------------

LAYOUTS = [(4, 32), (4, 64), (2, 32), (2, 64), (3, 32)]
M_VALUES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 53, 64, 100, 256]


def make_case(e, bits, tile_p, g, dtype, K, N, seed, table_kind="randn"):
    torch.manual_seed(seed)
    W = torch.randint(0, 2 ** bits, (K, N), dtype=torch.uint8)
    S = torch.randn(N, K // g).to(dtype)
    if table_kind == "arange":
        table = torch.arange(2 ** bits).to(dtype)
    else:
        table = torch.randn(2 ** bits).to(dtype)
    table2 = e.utils.make_qmap2_from_qmap(table)
    Q = torch.from_numpy(e.O.pack(W.numpy(), bits, tile_p))
    return W, Q, S, table, table2


@pytest.mark.parametrize("bits,tile_p", LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_random_vs_oracle_all_M(env, bits, tile_p, dtype):
    K, N, g = 1024, 1024, 64
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=bits * 10 + tile_p)
    What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
    W_exact = table.double()[W.long()] * torch.repeat_interleave(S.double(), g, dim=1).T        # lut * s before any rounding
    tids = template_ids_for(env.fa, bits, tile_p)
    for i, M in enumerate(M_VALUES):
        X = (torch.randn(M, K) / 100).to(dtype)
        ref = (X.float() @ What).to(dtype)
        tid = tids[(i * 7) % len(tids)]
        D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid)
        assert D.shape == (M, N) and D.dtype == dtype
        err = norm_rel_err(D, ref)
        assert err < tol_of(dtype), (bits, tile_p, dtype, M, tid, err)
        XC.assert_componentwise(D, X, W_exact, K, dtype, what=(bits, tile_p, dtype, M, tid))


@pytest.mark.parametrize("bits,tile_p", LAYOUTS)
@pytest.mark.parametrize("g", [32, 64, 128, 256])
def test_group_sizes_identity_and_random(env, bits, tile_p, g):
    dtype = torch.float16
    K, N = 512, 512 if bits != 3 else 512
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=g + bits, table_kind="arange")
    What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p)
    tid = template_ids_for(env.fa, bits, tile_p)[1 % len(template_ids_for(env.fa, bits, tile_p))]
    D = run_qgemm(env, torch.eye(K, dtype=dtype), Q, S, table, table2, bits, g, tid)
    assert torch.equal(D, What), (bits, tile_p, g)
    for M in (1, 4, 24):
        X = (torch.randn(M, K) / 100).to(dtype)
        D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid)
        assert norm_rel_err(D, (X.float() @ What.float())) < FP16_TOL


@pytest.mark.parametrize("bits,tile_p", LAYOUTS)
def test_ragged_k_and_odd_shapes(env, bits, tile_p):
    # K not a multiple of the 4096-k chunk / 512-k wave span; N = one or three blocks
    dtype = torch.float16
    blk = tile_p * (16 if bits == 3 else 16 // bits)
    for K, N in ((64, blk), (192, blk), (4608, blk), (8256, 3 * blk)):
        g = 64
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K + N)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        for M in (1, 3, 8, 20):
            X = (torch.randn(M, K) / 100).to(dtype)
            D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid)
            err = norm_rel_err(D, X.float() @ What)
            assert err < FP16_TOL, (bits, tile_p, K, N, M, err)


def test_forced_splitk_and_kw_variants(env):
    """Every K-split mode of both kernel families gives the same answer: in-workgroup split (kw), grid split
    (fp32 slabs combined inside the launch by the last arriver - csrc/xwg.h - or by the reduce pass), any number of waves
    per workgroup (the decode kernel is not limited to powers of two), both ring depths."""
    bits, tile_p, g, dtype = 4, 32, 64, torch.float16
    K, N = 4096, 512
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=7)
    What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    for M in (1, 4, 8, 16, 64):
        X = (torch.randn(M, K) / 100).to(dtype)
        ref = X.float() @ What
        for kw in (1, 2, 4, 8):
            for splitk in (1, 2, 4):
                for waves, depth in ((-1, -1), (8, 2), (12, 4)) if M <= 4 else ((-1, -1),):
                    if waves > 0 and waves % kw:
                        continue
                    ovr = dict(kw=kw, splitk=splitk, waves=waves, ring_depth=depth)
                    D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid, ovr)
                    err = norm_rel_err(D, ref)
                    assert err < FP16_TOL, (M, ovr, err)
        if M <= 4:                                   # both decode kernels, forced
            for one in (0, 1):
                D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid, dict(family=0, one_shot=one))
                assert norm_rel_err(D, ref) < FP16_TOL, (M, "one_shot", one)
    # the per-wave MFMA kernel's grid split is combined inside the launch while the slabs are small (round 4: csrc/xwg.h, L
    # form) and by the reduce pass beyond; both forms, every in-workgroup split, one-hot rows exact, repeat-identical, the
    # state words left clean
    from flute_amd import dev
    d = env.dev
    Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
    for (M, N2, modes) in ((64, N, (1,)), (16, N, (1,)), (3000, N, (0,))):
        X = (torch.randn(M, K) / 100).to(dtype)
        ks = torch.randint(0, K, (M,))
        E = torch.zeros(M, K, dtype=dtype)
        E[torch.arange(M), ks] = 1
        ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
        for kw in (1, 2, 8):
            for splitk in (2, 3, 4, 8):
                ovr = dev.Overrides(family=2, kw=kw, splitk=splitk)
                plan = dev.get_plan(M, N2, K, bits, g, tid, env.num_sms, dtype, ovr)
                assert plan["family"] == 2 and plan["splitk"] > 1 and plan["splitk_mode"] in modes, plan
                o = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr)
                o1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr)
                o2 = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr)
                assert norm_rel_err(o.cpu(), X.float() @ What) < FP16_TOL, (M, kw, splitk)
                assert torch.equal(o1.cpu(), ref1) and torch.equal(o, o2), (M, kw, splitk)
                assert int(env.ws[:65536].view(torch.int32).abs().sum().item()) == 0, (M, kw, splitk)


def test_decode_plan_shapes(env):
    """The streaming decode kernel under every launch shape the planner can produce: odd wave counts, deep K
    splits with idle waves (more K parts than 512-k pieces), ragged last unit group, several visits per
    workgroup (num_sms = 4 forces a persistent loop), 2/3/4-bit, both dtypes, all group sizes; one-hot rows
    bit-exact."""
    from flute_amd import dev
    d = env.dev
    cases = [
        # bits, tile_p, g, dtype, K, N
        (4, 32, 64, torch.float16, 2048, 1024), (4, 64, 128, torch.bfloat16, 1536, 1024),
        (4, 32, 256, torch.float16, 4096, 256), (4, 32, 32, torch.bfloat16, 1024, 512),
        (2, 32, 64, torch.float16, 2560, 512), (2, 64, 128, torch.bfloat16, 2048, 1024),
        (3, 32, 64, torch.bfloat16, 2048, 1024), (3, 32, 128, torch.float16, 3072, 512),
        (4, 32, 64, torch.float16, 4416, 256),          # G = 69: unaligned scale rows (element-wise staging)
        (4, 32, 64, torch.float16, 192, 128),           # K < one piece
    ]
    shapes = [dict(), dict(waves=1, kw=1), dict(waves=3, kw=1), dict(waves=5, kw=1), dict(waves=6, kw=2),
              dict(waves=8, kw=8), dict(waves=12, kw=4), dict(waves=14, kw=2), dict(waves=16, kw=16),
              dict(waves=7, kw=1, ring_depth=2), dict(waves=16, kw=1, ring_depth=4), dict(waves=4, kw=4, splitk=2)]
    for (bits, tile_p, g, dtype, K, N) in cases:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 91 + bits)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for M in (1, 2, 3, 4):
            X = (torch.randn(M, K) / 100).to(dtype)
            ks = torch.randint(0, K, (M,))
            E = torch.zeros(M, K, dtype=dtype)
            E[torch.arange(M), ks] = 1
            ref = X.float() @ What
            ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
            for shp in shapes:
                for num_sms in (env.num_sms, 4):
                    ovr = dev.Overrides(family=0, **shp)           # (M = 3, 4 take the MFMA kernel unless asked)
                    assert dev.get_plan(M, N, K, bits, g, tid, num_sms, dtype, ovr)["family"] == 0
                    out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, num_sms, ovr).cpu()
                    err = norm_rel_err(out, ref)
                    assert err < tol_of(dtype), (bits, tile_p, g, dtype, K, N, M, shp, num_sms, err)
                    out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, num_sms, ovr).cpu()
                    assert torch.equal(out1, ref1), (bits, tile_p, g, dtype, K, N, M, shp, num_sms)


def test_persistent_oneshot_kernel(env):
    """The persistent one-shot kernel (qgemm_persist.h; override one_shot = 2, automatic for one row on layers of
    >= 40 M weights): one and two rows, 2/3/4 bits, both dtypes and TileP, every group size it takes, 2- and 4-piece segments, one and
    several visits per wave (num_sms = 4), idle waves in the last workgroup, rows longer than the register-staged
    activations (K = 28672), the fused Hadamard rotation - against the oracle, one-hot rows bit-exact."""
    from flute_amd import dev
    d = env.dev
    cases = [
        # bits, tile_p, g, dtype, K, N
        (4, 32, 64, torch.float16, 4096, 1024), (4, 64, 128, torch.bfloat16, 2048, 1024), (4, 32, 256, torch.float16, 1024, 512),
        (4, 32, 64, torch.bfloat16, 5120, 256),          # 10 pieces: 2-piece segments
        (2, 32, 64, torch.float16, 2048, 1024), (2, 64, 128, torch.bfloat16, 4096, 512),
        (3, 32, 64, torch.bfloat16, 2048, 1024), (3, 32, 128, torch.float16, 3072, 512),
        (4, 32, 64, torch.float16, 28672, 256), (3, 32, 64, torch.float16, 17408, 512),
    ]
    for (bits, tile_p, g, dtype, K, N) in cases:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 87 + bits)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for M in (1, 2):
            X = (torch.randn(M, K) / 100).to(dtype)
            ks = torch.randint(0, K, (M,))
            E = torch.zeros(M, K, dtype=dtype)
            E[torch.arange(M), ks] = 1
            ref = X.float() @ What
            ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
            for shp in (dict(), dict(waves=8), dict(waves=5), dict(waves=4, ring_depth=2), dict(waves=6)):
                for num_sms in (env.num_sms, 4):
                    ovr = dev.Overrides(family=0, one_shot=2, **shp)
                    plan = dev.get_plan(M, N, K, bits, g, tid, num_sms, dtype, ovr)
                    if plan["one_shot"] != 3:                    # the rows' activations do not fit LDS beside the table: ring kernel
                        assert M > 1 and plan["family"] == 0, plan
                        continue
                    assert plan["m_block"] >= M and plan["k_chunks"] * plan["ring_depth"] * 512 == K
                    assert plan["grid"] * plan["waves"] * plan["visits"] >= N // (16 if bits == 3 else 16 // bits)
                    out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, num_sms, ovr)
                    assert norm_rel_err(out.cpu(), ref) < tol_of(dtype), (bits, tile_p, g, dtype, K, N, M, shp, num_sms)
                    out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, num_sms, ovr).cpu()
                    assert torch.equal(out1, ref1), (bits, tile_p, g, dtype, K, N, M, shp, num_sms)
        for h in (512, 64):                              # fused rotation == rotate, then multiply
            if K % h:
                continue
            Xh = (torch.randn(2, K) / 10).to(dtype).to(d)
            fused = dev.qgemm_planned(Xh, Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, dev.Overrides(family=0, one_shot=2), hadamard_size=h)
            two = dev.qgemm_planned(env.fa.hadamard_transform(Xh, h), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms,
                                    dev.Overrides(family=0, one_shot=2))
            assert torch.equal(fused, two), (bits, dtype, K, h)
    # what it does not take: more than two rows, odd group counts, K that is not whole pieces -> the ring kernel
    for (M, K) in ((3, 4096), (1, 4416), (1, 4096 + 256)):
        plan = dev.get_plan(M, 1024, K, 4, 64, template_ids_for(env.fa, 4, 32)[0], env.num_sms, torch.float16, dev.Overrides(family=0, one_shot=2))
        assert plan["one_shot"] == 0, (M, K, plan)
    # automatic for one row on the big layers
    plan = dev.get_plan(1, 28672, 8192, 4, 64, template_ids_for(env.fa, 4, 32)[0], env.num_sms, torch.float16)
    assert plan["one_shot"] == 3 and plan["waves"] * plan["grid"] <= 8 * env.num_sms, plan


def test_lean_decode_kernel(env):
    """The lean decode kernel (qgemm_fast.h, round 5; plan.one_shot == 4; override one_shot = 4, automatic for the
    automatic 4-bit ids on K = 2048 / 4096 layers in the one-shot regime): every instantiated shape (waves per
    workgroup, waves per unit row, pieces per wave) x rows per pass (M = 1 .. 4) x dtype x TileP x group size - against
    the oracle, one-hot rows bit-exact (the identity contract of tests/kernel.py:30-36), an arbitrary pair codebook
    (HIGGS vector_size = 2: table2 is not an outer product) included.  What it does not take falls back to the round-4
    kernels."""
    from flute_amd import dev
    d = env.dev
    cases = [
        # tile_p, g, dtype, K, N, template rank (Stages - 2)
        (32, 64, torch.float16, 4096, 1024, 0), (32, 64, torch.float16, 4096, 1024, 1), (64, 128, torch.bfloat16, 4096, 2048, 0),
        (64, 256, torch.float16, 4096, 1024, 1), (32, 128, torch.bfloat16, 8192, 1024, 0), (64, 64, torch.float16, 8192, 512, 0),
        (32, 256, torch.bfloat16, 2048, 1024, 0), (64, 64, torch.float16, 2048, 2048, 0), (32, 64, torch.bfloat16, 4096, 11008 // 128 * 128, 1),
        (32, 64, torch.float16, 3584, 2048, 0), (64, 128, torch.bfloat16, 3584, 1024, 0), (32, 256, torch.float16, 3584, 512, 0),     # K = 7 pieces (Gemma-2-9B)
    ]
    ran = {1: 0, 2: 0, 4: 0}
    for (tile_p, g, dtype, K, N, rank) in cases:
        bits = 4
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 83 + N % 11 + rank)
        tid = template_ids_for(env.fa, bits, tile_p)[0] + 4 * rank          # Stages 2 + rank, QuantMapMode digit 0
        ovr = dev.Overrides(family=0, one_shot=4)
        Qd, Sd, td = Q.to(d), S.to(d), table.to(d)
        for pair_codebook in (False, True):
            t2 = table2
            if pair_codebook:                                               # any 256 x 2 codebook (flute/integrations/higgs.py:67-71)
                grid = torch.randn(256, 2).to(dtype)
                t2 = grid.view(16, 16, 2).contiguous().view(torch.float32)          # [16, 16, 1]: two T in a 32-bit container
            What = env.O.dequantize(Q.numpy(), S, t2, bits, g, tile_p).float()
            for M in (1, 2, 3, 4):
                mb = 1 if M == 1 else (2 if M == 2 else 4)
                plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)
                if mb * K * 2 > 32768:                                      # the rows do not fit beside the table image: a round-4 kernel
                    assert plan["one_shot"] != 4 or plan["family"] != 0, (M, K, plan)
                    continue
                assert plan["family"] == 0 and plan["one_shot"] == 4 and plan["m_block"] == mb, plan
                assert 512 * plan["ring_depth"] * plan["kw"] == K and plan["grid"] * (plan["waves"] // plan["kw"]) == N // 4, plan
                ran[mb] += 1
                X = (torch.randn(M, K) / 100).to(dtype)
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2.to(d), env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert out.shape == (M, N)
                assert norm_rel_err(out, X.float() @ What) < tol_of(dtype), (tile_p, g, dtype, K, N, rank, M, pair_codebook)
                ks = torch.randint(0, K, (M,))
                ks[0] = (0, K - 1)[M % 2]
                E = torch.zeros(M, K, dtype=dtype)
                E[torch.arange(M), ks] = 1
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2.to(d), env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert torch.equal(out1.float(), What[ks].to(dtype).float()), ("one-hot", tile_p, g, dtype, K, N, M, pair_codebook)
        # the automatic plan of the same id is this kernel for one row while the layer is in the one-shot regime
        plan1 = dev.get_plan(1, N, K, bits, g, tid, env.num_sms, dtype, ovr)
        auto = dev.get_plan(1, N, K, bits, g, tid, env.num_sms, dtype)
        if N * K <= (48 << 20) and env.num_sms <= 2 * plan1["grid"] <= (6 if K != 3584 else 2) * env.num_sms and K != 8192:
            assert auto["one_shot"] == 4, auto
        auto4 = dev.get_plan(4, N, K, bits, g, tid, env.num_sms, dtype)
        if N * K <= (16 << 20) and env.num_sms <= 2 * plan1["grid"] <= 2 * env.num_sms and K != 8192:      # one round of workgroups
            assert auto4["family"] == 0 and auto4["one_shot"] == 4 and auto4["m_block"] == 4, auto4
    assert min(ran.values()) > 0, ran
    # flute.qgemm_hadamard (qgemm.cpp:201-244) never takes this kernel: the fused rotation stays with the round-4 one-shot kernel
    # (measured, qgemm_fast.h) - the Hadamard call still fuses its rotation and its result is that of hadamard_transform
    # followed by flute.qgemm, up to the order of the k sum
    lib = env.fa._lib.get()
    for (tile_p, g, dtype, K, N) in ((32, 64, torch.float16, 3584, 4096), (64, 128, torch.bfloat16, 4096, 3584 // 256 * 256)):
        W, Q, S, table, table2 = make_case(env, 4, tile_p, g, dtype, K, N, seed=K % 71 + N % 17)
        tid = template_ids_for(env.fa, 4, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        assert dev.get_plan(1, N, K, 4, g, tid, env.num_sms, dtype)["one_shot"] == 4
        for h in (512, 2):
            X = (torch.randn(1, K) / 10).to(dtype).to(d)
            assert lib.flute_qgemm_hadamard_fused(0 if dtype == torch.float16 else 1, 4, g, h, 1, N, K, tid, env.num_sms, env.ws.numel()) == 1
            auto = env.fa.qgemm_hadamard(X, Qd, Sd, td, t2d, env.ws, 4, g, h, tid, env.num_sms)
            two = env.fa.qgemm(env.fa.hadamard_transform(X, h), Qd, Sd, td, t2d, env.ws, 4, g, tid, env.num_sms)
            tol = 2e-3 if dtype == torch.float16 else 4e-3
            assert norm_rel_err(auto, two) < tol, (dtype, K, N, h)               # different kernels: the same products, summed in another order
    # not taken: five rows, 2 / 3 bits, 32-wide groups, K that is not 2048 / 3584 / 4096 / 8192
    for (M, K, bits, g) in ((5, 4096, 4, 64), (1, 4096, 2, 64), (1, 4096, 3, 64), (1, 4096, 4, 32), (1, 3072, 4, 64), (1, 14336, 4, 64)):
        plan = dev.get_plan(M, 4096, K, bits, g, template_ids_for(env.fa, bits, 32)[0], env.num_sms, torch.float16, dev.Overrides(family=0, one_shot=4) if M <= 4 else dev.Overrides(one_shot=4))
        assert plan["one_shot"] != 4 or plan["family"] != 0, (M, K, bits, g, plan)


def test_lean_mfma_decode_kernel(env):
    """The lean MFMA decode kernel (qgemm_fastm.h, round 5; family 7): a workgroup = 4 unit rows x all of K, its 8 waves
    split K, M <= 16.  Every instantiation (K = 4096 / 2048 x group size x dtype x TileP) x M in {1, 5, 8, 13, 16} against
    the oracle, one-hot rows bit-exact (tests/kernel.py:30-36), an arbitrary pair codebook included.  Round 6: one, two and three
    column groups per workgroup on one staged activation set (slabs_per_wave), also where the last workgroup holds fewer groups
    than the others (N = 11008: 688 groups, N = 5248: 328 groups, at three per workgroup)."""
    from flute_amd import dev
    d = env.dev
    cases = [
        # tile_p, g, dtype, K, N
        (32, 64, torch.float16, 4096, 1024), (64, 128, torch.bfloat16, 4096, 2048), (32, 256, torch.float16, 4096, 512),
        (64, 64, torch.bfloat16, 4096, 1024), (32, 64, torch.float16, 2048, 1024), (64, 128, torch.bfloat16, 2048, 2048),
        (32, 128, torch.float16, 4096, 11008 // 128 * 128), (32, 64, torch.bfloat16, 2048, 5248),
    ]
    for (tile_p, g, dtype, K, N) in cases:
        bits = 4
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 79 + N % 13 + g)
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td = Q.to(d), S.to(d), table.to(d)
        for pair_codebook in (False, True):
            t2 = table2
            if pair_codebook:
                grid = torch.randn(256, 2).to(dtype)
                t2 = grid.view(16, 16, 2).contiguous().view(torch.float32)
            What = env.O.dequantize(Q.numpy(), S, t2, bits, g, tile_p).float()
            for M, ng in [(M, ng) for M in (1, 5, 8, 13, 16) for ng in ((1, 2, 3) if M in (5, 16) else (-1,))]:
                ovr = dev.Overrides(family=7, slabs_per_wave=ng)
                plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)
                assert plan["family"] == 7 and plan["waves"] == 8 and plan["lds_bytes"] == 32768 + 32 * K, plan
                assert plan["grid"] == -(-(N // 16) // plan["slabs_per_wave"]) and (ng < 0 or plan["slabs_per_wave"] == ng), plan
                X = (torch.randn(M, K) / 100).to(dtype)
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2.to(d), env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert out.shape == (M, N)
                assert norm_rel_err(out, X.float() @ What) < tol_of(dtype), (tile_p, g, dtype, K, N, M, ng, pair_codebook, norm_rel_err(out, X.float() @ What))
                ks = torch.randint(0, K, (M,))
                ks[0] = (0, K - 1)[M % 2]
                E = torch.zeros(M, K, dtype=dtype)
                E[torch.arange(M), ks] = 1
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2.to(d), env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert torch.equal(out1.float(), What[ks].to(dtype).float()), ("one-hot", tile_p, g, dtype, K, N, M, ng, pair_codebook)
    # not taken (the override falls back): 17 rows, 2 / 3 bits, 32-wide groups, other K, one group per wave
    for (M, K, bits, g) in ((17, 4096, 4, 64), (8, 4096, 2, 64), (8, 4096, 3, 64), (8, 4096, 4, 32), (8, 8192, 4, 64), (8, 2048, 4, 256)):
        plan = dev.get_plan(M, 4096, K, bits, g, template_ids_for(env.fa, bits, 32)[0], env.num_sms, torch.float16, dev.Overrides(family=7))
        assert plan["family"] != 7, (M, K, bits, g, plan)


def test_persistent_mfma_decode_kernel(env):
    """The persistent MFMA decode kernel (qgemm_persistm.h, round 6; family 8; 4-bit and 2-bit members): workgroups stream column-group sets x all of K, the eight
    waves of a workgroup take the 128-k macro-steps w, w + 8, ... - every (group size, TileP, dtype), one / two / three column groups per
    set, one / two / four activation requests per macro-step (M <= 4 / 8 / 16), one and several sets per workgroup (override m_tiles), K
    that leaves the waves unequal shares (1152 = 9 macro-steps, 1280 = 10, 3584 = 28), layers whose last set holds fewer groups (N = 5248:
    328 groups), the activations resident in LDS (K x rows within 64 KB: every K <= 8192 case here at M <= 4, K <= 4096 at M <= 8) and through the rings -
    against the oracle, one-hot rows bit-exact (tests/kernel.py:30-36), an arbitrary pair codebook included."""
    from flute_amd import dev
    d = env.dev
    cases = [
        # bits, tile_p, g, dtype, K, N
        (4, 32, 64, torch.float16, 8192, 1024), (4, 64, 128, torch.bfloat16, 8192, 2048), (4, 32, 64, torch.bfloat16, 1152, 5248),
        (4, 64, 64, torch.float16, 3584, 1024), (4, 32, 128, torch.float16, 1280, 5248), (4, 32, 64, torch.float16, 11008, 512),
        # the 2-bit member (a group = two unit rows of eight columns, 16-entry pair table)
        (2, 32, 64, torch.float16, 8192, 1024), (2, 64, 128, torch.bfloat16, 4096, 2048), (2, 32, 64, torch.bfloat16, 1152, 5376), (2, 32, 128, torch.float16, 3584, 768),
    ]
    for (bits, tile_p, g, dtype, K, N) in cases:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 79 + N % 13 + g)
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td = Q.to(d), S.to(d), table.to(d)
        for pair_codebook in (False, True):
            t2 = table2
            if pair_codebook:
                grid = torch.randn(4 ** bits, 2).to(dtype)
                t2 = grid.view(2 ** bits, 2 ** bits, 2).contiguous().view(torch.float32)
            What = env.O.dequantize(Q.numpy(), S, t2, bits, g, tile_p).float()
            for M, ng, vis, res in [(M, ng, vis, res) for M in (1, 3, 4, 7, 8, 13, 16) for ng in ((1, 2, 3) if M in (3, 7, 16) else (-1,)) for vis in ((-1, 3) if M in (3, 16) else (-1,))
                                    for res in ((-1, 0) if M in (3, 7) and vis < 0 else (-1,))]:     # res 0: the activation rings also where the activations could be resident
                ovr = dev.Overrides(family=8, slabs_per_wave=ng, m_tiles=vis, one_shot=res)
                plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)
                nsets = -(-(N // 16) // plan["slabs_per_wave"])
                assert plan["family"] == 8 and plan["waves"] == 8 and (ng < 0 or plan["slabs_per_wave"] == ng), plan
                assert plan["grid"] * plan["visits"] >= nsets and plan["grid"] <= nsets and (vis < 0 or plan["visits"] == vis), plan
                xr = 1 if M <= 4 else 2 if M <= 8 else 4
                assert plan["one_shot"] == (1 if res != 0 and K * xr <= 8192 and xr <= 2 and not (xr == 1 and plan["slabs_per_wave"] == 3) else 0), plan
                X = (torch.randn(M, K) / 100).to(dtype)
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2.to(d), env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert out.shape == (M, N)
                assert norm_rel_err(out, X.float() @ What) < tol_of(dtype), (tile_p, g, dtype, K, N, M, ng, vis, pair_codebook, norm_rel_err(out, X.float() @ What))
                ks = torch.randint(0, K, (M,))
                ks[0] = (0, K - 1)[M % 2]
                E = torch.zeros(M, K, dtype=dtype)
                E[torch.arange(M), ks] = 1
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2.to(d), env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert torch.equal(out1.float(), What[ks].to(dtype).float()), ("one-hot", tile_p, g, dtype, K, N, M, ng, vis, pair_codebook)
    # automatic on the large layers it was measured on (ids that leave the choice to the planner)
    for (M, N, K, fam) in ((4, 4096, 4096, 8), (16, 4096, 4096, 8), (16, 8192, 28672, 8), (16, 28672, 8192, 2), (2, 4096, 4096, 0)):
        plan = dev.get_plan(M, N, K, 2, 64, template_ids_for(env.fa, 2, 32)[0], env.num_sms, torch.float16)
        assert env.num_sms != 256 or plan["family"] == fam, (2, M, N, K, plan)
    for (M, N, K, fam) in ((4, 8192, 8192, 8), (16, 8192, 8192, 8), (8, 4096, 14336, 8), (16, 28672, 8192, 8), (4, 14336, 4096, 8), (8, 14336, 4096, 8), (16, 14336, 4096, 5), (8, 14336, 3584, 8),
                           (8, 4096, 4096, 8), (16, 4096, 4096, 7), (4, 4096, 4096, 0), (2, 8192, 8192, 0)):
        plan = dev.get_plan(M, N, K, 4, 64, template_ids_for(env.fa, 4, 32)[0], env.num_sms, torch.float16)
        assert env.num_sms != 256 or plan["family"] == fam, (M, N, K, plan)
    # not taken (the override is refused): 17 rows, 3 bits, 32- / 256-wide groups, K below 1024 or not a multiple of 128, group size 128 with an odd number of groups
    for (M, K, bits, g) in ((17, 8192, 4, 64), (17, 8192, 2, 64), (8, 8192, 3, 64), (8, 8192, 4, 32), (8, 8192, 4, 256), (8, 512, 4, 64), (8, 4096 + 64, 4, 64), (8, 1152, 4, 128)):
        try:
            plan = dev.get_plan(M, 4096, K, bits, g, template_ids_for(env.fa, bits, 32)[0], env.num_sms, torch.float16, dev.Overrides(family=8))
        except Exception:  # noqa: BLE001
            continue
        assert plan["family"] != 8, (M, K, bits, g, plan)


def test_skinny_mfma_kernel(env):
    """The skinny MFMA kernel (qgemm_skinny.h; override family 5, automatic for 4-bit layers at 3 <= M <= 16 whose
    64-column slabs fill the chip in one round): every k-step depth (K = 32 x depth x waves), 4 and 8 waves, both dtypes
    and TileP, group sizes 32 .. 256, every M up to 16 (rows beyond M read as zero) - against the oracle, one-hot rows
    bit-exact (w^ = round_T(lut * s), the reference's contract)."""
    from flute_amd import dev
    d = env.dev
    cases = [
        # bits, tile_p, g, dtype, K, N
        (4, 32, 64, torch.float16, 4096, 1024), (4, 64, 128, torch.bfloat16, 2048, 1024), (4, 32, 256, torch.float16, 4096, 256),
        (4, 32, 32, torch.bfloat16, 1024, 256), (4, 64, 64, torch.float16, 512, 512), (4, 32, 128, torch.float16, 1024, 11008),
    ]
    for (bits, tile_p, g, dtype, K, N) in cases:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 85 + N % 7)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for M in (1, 3, 7, 16):
            X = (torch.randn(M, K) / 100).to(dtype)
            ks = torch.randint(0, K, (M,))
            E = torch.zeros(M, K, dtype=dtype)
            E[torch.arange(M), ks] = 1
            ref = X.float() @ What
            ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
            ran = 0
            for waves in (8, 4):
                ovr = dev.Overrides(family=5, waves=waves)
                plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)
                if plan["family"] != 5:                      # K / (32 waves) is not 4, 8 or 16 (or too many groups per wave)
                    continue
                ran += 1
                assert plan["ring_depth"] * plan["waves"] * 32 == K and plan["grid"] == N // 64 and plan["splitk"] == 1
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert norm_rel_err(out, ref) < tol_of(dtype), (bits, tile_p, g, dtype, K, N, M, waves)
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert torch.equal(out1, ref1), (bits, tile_p, g, dtype, K, N, M, waves)
            assert ran, (K, g)
    # taken automatically on the Llama-3 8B MLP width (11008: round 6 - the lean MFMA decode kernel with three column groups per workgroup);
    # same results as the per-wave kernel within tolerance
    bits, tile_p, g, dtype, K, N = 4, 32, 64, torch.float16, 4096, 14336
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=5)
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    X = (torch.randn(16, K) / 100).to(dtype)
    assert dev.get_plan(16, N, K, bits, g, tid, env.num_sms, dtype)["family"] == 5
    assert dev.get_plan(16, 11008, K, bits, g, tid, env.num_sms, dtype)["family"] == 7
    a = run_qgemm(env, X, Q, S, table, table2, bits, g, tid)
    b = run_qgemm(env, X, Q, S, table, table2, bits, g, tid, dict(family=2))
    assert norm_rel_err(a, b.float()) < 5e-4


def test_decode_chunked_activations(env):
    """K ranges whose activations do not fit in LDS at once are staged in chunks (M = 4, K = 28672: 224 KB)."""
    from flute_amd import dev
    d = env.dev
    for (bits, tile_p, g, dtype, K, N, M) in ((4, 32, 64, torch.float16, 28672, 256, 4),
                                              (4, 64, 128, torch.bfloat16, 28672, 256, 3),
                                              (3, 32, 64, torch.bfloat16, 28672, 512, 2),
                                              (2, 32, 64, torch.float16, 36864, 256, 4)):
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 83)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, dev.Overrides(family=0, splitk=1))
        assert plan["family"] == 0 and (plan["k_chunks"] > 1 or bits == 3), plan     # 3-bit: 8 KB table, the rows fit
        X = (torch.randn(M, K) / 100).to(dtype)
        for shp in (dict(splitk=1), dict(waves=8, kw=8, splitk=1), dict(waves=6, kw=1, splitk=1), dict()):
            out = dev.qgemm_planned(X.to(d), Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, tid,
                                    env.num_sms, dev.Overrides(family=0, **shp)).cpu()
            err = norm_rel_err(out, X.float() @ What)
            assert err < tol_of(dtype), (bits, g, dtype, K, M, shp, err)


def test_mfma_family_for_small_M(env):
    """Forcing the MFMA kernel at M <= 8 must agree with the decode kernel."""
    bits, tile_p, g = 4, 64, 128
    for dtype in (torch.float16, torch.bfloat16):
        K, N = 1024, 512
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=3)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        for M in (1, 7):
            X = (torch.randn(M, K) / 100).to(dtype)
            D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid, dict(family=2))
            assert norm_rel_err(D, X.float() @ What) < tol_of(dtype)


def test_mfma_scale_block_and_ring_paths(env):
    """The MFMA kernel's scale blocks (8 groups, fetched by LDS-DMA one block ahead) and its operand ring:
    many blocks per wave (no K split), blocks shorter than the ring is deep (g = 32 with 4 lanes per unit),
    a K range that starts mid-block, scale rows that are not 16-B aligned (plain staged loads), a ragged
    last macro-step (K % 128 != 0 with 4 k-steps per weight piece) and a shallow ring (fewer waves)."""
    cases = [
        # bits, tile_p, g, dtype, K, N, M, overrides (family, R, waves, kw, splitk, MT, slabs per wave)
        (4, 32, 64, torch.float16, 8192, 512, 64, (2, 1, 8, 1, 1, 4, -1)),      # 16 blocks per wave
        (4, 32, 64, torch.bfloat16, 8192, 512, 48, (2, 1, 8, 1, 1, 4, -1)),
        (4, 32, 32, torch.float16, 2048, 512, 16, (2, 4, 8, 1, 1, 1, -1)),      # block = 2 macro-steps < ring depth
        (4, 64, 32, torch.bfloat16, 2048, 512, 9, (2, 4, 8, 2, 1, 1, -1)),
        (4, 32, 64, torch.float16, 4096 + 320, 512, 16, (2, 4, 8, 4, 1, 1, -1)),  # G = 69: unaligned scale rows, ragged K
        (2, 32, 64, torch.float16, 4096 + 320, 512, 33, (2, 2, 8, 2, 1, 2, -1)),
        (4, 32, 128, torch.float16, 3072, 512, 16, (2, 2, 4, 4, 1, 1, -1)),      # wave ranges start mid-block
        (3, 32, 64, torch.bfloat16, 4096, 512, 20, (2, 1, 8, 2, 1, 1, -1)),
        (3, 32, 64, torch.float16, 2048 + 64, 1024, 5, (2, 1, 4, 1, 2, 1, -1)),  # grid split-K partials (16-B stores)
        (4, 32, 64, torch.float16, 2048, 1024, 100, (2, 1, 8, 4, 1, 4, 2)),       # two slabs per wave (8 column tiles)
        (4, 64, 64, torch.bfloat16, 2048 + 64, 1024, 40, (2, 1, 8, 2, 1, 2, 2)),
        (4, 32, 128, torch.float16, 4096, 512, 33, (2, 1, 4, 2, 2, 2, 2)),
        (4, 32, 64, torch.float16, 2048, 1024, 16, (2, 1, 8, 8, 1, 1, 2)),        # one row tile x two slabs per wave (round 3: wide layers at M <= 16)
        (4, 64, 64, torch.bfloat16, 4096 + 64, 1024, 5, (2, 1, 8, 4, 1, 1, 2)),
    ]
    for (bits, tile_p, g, dtype, K, N, M, o) in cases:
        ovr = dict(family=o[0], m_block=o[1], waves=o[2], kw=o[3], splitk=o[4], m_tiles=o[5], slabs_per_wave=o[6])
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 97)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        X = (torch.randn(M, K) / 100).to(dtype)
        D = run_qgemm(env, X, Q, S, table, table2, bits, g, tid, ovr)
        err = norm_rel_err(D, X.float() @ What)
        assert err < tol_of(dtype), (bits, tile_p, g, dtype, K, N, M, ovr, err)
        # one-hot rows: bit-exact (each output element is one rounded product)
        ks = torch.randint(0, K, (M,))
        E = torch.zeros(M, K, dtype=dtype)
        E[torch.arange(M), ks] = 1
        D1 = run_qgemm(env, E, Q, S, table, table2, bits, g, tid, ovr)
        ref = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks]
        assert torch.equal(D1.float(), ref.to(dtype).float()), (bits, g, dtype, K, ovr)


def test_block_prefill_kernel(env):
    """The block-tiled prefill kernels (family 3, qgemm_block2.h / qgemm_block3.h / qgemm_block.h): 256- and 128-row blocks, ragged M (rows past M
    read as zero and are not stored), every group size (scale blocks of 8 groups arrive by LDS-DMA), both TileP
    layouts and dtypes, a forced grid-level K split; one-hot rows bit-exact (w^ = round_T(lut * s))."""
    from flute_amd import dev
    d = env.dev
    for (bits, tile_p, g, dtype, K, N) in [(4, 32, 64, torch.float16, 4096, 1024), (4, 64, 64, torch.bfloat16, 2048, 1024),
                                           (4, 32, 128, torch.float16, 3072, 512), (4, 32, 32, torch.bfloat16, 1024, 256),
                                           (4, 64, 256, torch.float16, 4096, 256),
                                           (2, 32, 64, torch.float16, 2048, 1024), (2, 64, 128, torch.bfloat16, 3072, 512),
                                           (2, 32, 32, torch.bfloat16, 1024, 256),
                                           (3, 32, 64, torch.float16, 2048, 1024), (3, 32, 128, torch.bfloat16, 3072, 512),
                                           (3, 32, 32, torch.bfloat16, 1024, 512)]:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K + N)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for M in (1, 130, 256, 700):
            X = (torch.randn(M, K) / 100).to(dtype)
            ks = torch.randint(0, K, (M,))
            E = torch.zeros(M, K, dtype=dtype)
            E[torch.arange(M), ks] = 1
            ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
            # 256- / 128-row blocks of the 1 x 8 wave split (qgemm_block2.h; 3 bits: qgemm_block3.h, whose 256-row blocks keep
            # the second / third bit-plane pieces of two waves in LDS), with and without a grid K split
            for shp in (dict(family=3, m_tiles=8), dict(family=3, m_tiles=4),
                        dict(family=3, m_tiles=8, splitk=2), dict(family=3, m_tiles=4, splitk=2)):
                ovr = dev.Overrides(**shp)
                plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)
                assert plan["family"] == 3
                if "splitk" in shp:      # 3-bit blocks of up to 128 rows combine their K slices inside the launch (round 5), the others by a reduce launch
                    assert plan["splitk_mode"] == (1 if bits == 3 and shp["m_tiles"] == 4 else 0), plan
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                err = norm_rel_err(out, X.float() @ What)
                assert err < tol_of(dtype), (tile_p, g, dtype, K, N, M, shp, err)
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert torch.equal(out1, ref1), (tile_p, g, dtype, K, N, M, shp)
    # 3-bit skinny blocks (16 / 32 / 64 rows, grid K split: qgemm_block3.h RT = 1, 2, 4)
    bits, tile_p, g, dtype, K, N = 3, 32, 64, torch.bfloat16, 2048, 1024
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=77)
    What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
    for M in (5, 16, 17, 40, 64, 90):
        X = (torch.randn(M, K) / 100).to(dtype)
        ks = torch.randint(0, K, (M,))
        E = torch.zeros(M, K, dtype=dtype)
        E[torch.arange(M), ks] = 1
        ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
        for rt in (1, 2, 4):
            for sk in (-1, 1):
                ovr = dev.Overrides(family=3, m_block=rt, splitk=sk)
                assert dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)["m_block"] == 8 + rt
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert norm_rel_err(out, X.float() @ What) < tol_of(dtype), (M, rt, sk)
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr).cpu()
                assert torch.equal(out1, ref1), (M, rt, sk)
    assert int(env.ws[:65536].view(torch.int32).abs().sum().item()) == 0        # the tile state words are zero again (xwg.h)
    p = dev.get_plan(64, 8192, 8192, 3, 64, 4, 256, torch.bfloat16)
    assert p["family"] == 3 and p["m_block"] == 12 and p["splitk"] > 1, p
    # the planner takes it by itself where the output has enough blocks
    p = dev.get_plan(4096, 4096, 4096, 4, 64, 16, 256, torch.float16)
    assert p["family"] == 3 and p["m_block"] == 4 and p["grid"] == 256, p           # 256-row blocks, 1 x 8 split
    p = dev.get_plan(2048, 4096, 4096, 4, 64, 16, 256, torch.bfloat16)
    assert p["family"] == 3 and p["m_block"] == 5 and p["grid"] == 256, p           # 128-row blocks fill the chip
    assert dev.get_plan(256, 4096, 4096, 4, 64, 16, 256, torch.float16)["family"] == 6       # 64 x 64 tiles over all of K (round 6; rounds 2 - 5: the per-wave kernel)
    p = dev.get_plan(4096, 4096, 4096, 2, 64, 0, 256, torch.float16)
    assert p["family"] == 3 and p["m_block"] == 4, p                                 # 2-bit layers: the 1 x 8 split only
    p = dev.get_plan(4096, 4096, 4096, 3, 64, 4, 256, torch.bfloat16)
    assert p["family"] == 3 and p["m_block"] == 4 and p["grid"] == 256, p          # 3 bits: 256-row blocks (qgemm_block3.h, round 3)
    p = dev.get_plan(1024, 4096, 4096, 3, 64, 4, 256, torch.bfloat16)
    assert p["family"] == 3 and p["m_block"] == 5 and p["splitk"] == 2 and p["grid"] == 256, p   # ... 128-row blocks x two K slices (round 4) where whole blocks leave CUs idle
    assert dev.get_plan(700, 1024, 2048, 3, 64, 4, 256, torch.float16, dev.Overrides(family=3, m_tiles=8))["m_block"] == 4


def _state_words_clean(env):
    """First 64 KB of the workspace: the tile state words of the in-launch reductions (csrc/xwg.h) - zero between calls."""
    return int(env.ws[:65536].view(torch.int32).abs().sum().item()) == 0


def test_splitk_block_kernel(env):
    """The split-K block kernel (family 6, qgemm_splitk.h): 128 x 128 tiles x K slices whose partial tiles meet inside the
    launch (csrc/xwg.h - the role of the reference's FixupHelper, tile_scheduler_utils.hpp:58-211).  Every form of the seam
    (no split; E form at 2 and 4 slices; L form at 3, 6, 8, 16), ragged M (rows past M read as zero, never stored), both
    TileP layouts and dtypes, 2 and 4 bits, group sizes 32 .. 256 (the wave's scales for its whole K half are staged once);
    against the oracle, one-hot rows bit-exact (w^ = round_T(lut * s)), repeated launches bit-identical (fixed summation
    order) and the state words zero after every call (tile_scheduler_utils.hpp:196)."""
    from flute_amd import dev
    d = env.dev
    assert _state_words_clean(env)
    for (bits, tile_p, g, dtype, K, N) in [(4, 32, 64, torch.float16, 4096, 1024), (4, 64, 64, torch.bfloat16, 2048, 1024),
                                           (4, 32, 128, torch.float16, 3072, 512), (4, 32, 32, torch.bfloat16, 1024, 256),
                                           (4, 64, 256, torch.float16, 4096, 256), (2, 32, 64, torch.float16, 2048, 1024),
                                           (2, 64, 128, torch.bfloat16, 3072, 512), (2, 32, 32, torch.bfloat16, 1024, 256)]:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K + N + 1)
        What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for M in (1, 130, 256, 700):
            X = (torch.randn(M, K) / 100).to(dtype)
            ks = torch.randint(0, K, (M,))
            E = torch.zeros(M, K, dtype=dtype)
            E[torch.arange(M), ks] = 1
            ref = X.float() @ What
            ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
            ran = set()
            # 128- and 64-row tiles x two K parts per workgroup, 64-row tiles x four K parts (64-column tiles, round 6)
            for sk, rt, kp in [(sk, rt, kp) for sk in (1, 2, 3, 4, 6, 8, 16) for (rt, kp) in ((8, 2), (4, 2), (4, 4))]:
                ovr = dev.Overrides(family=6, splitk=sk, m_tiles=rt, kw=kp)
                try:
                    plan = dev.get_plan(M, N, K, bits, g, tid, env.num_sms, dtype, ovr)
                except RuntimeError:
                    continue                                      # not a legal split of this K (qgemm_splitk.h's host contract)
                assert plan["family"] == 6 and plan["splitk"] == sk and plan["m_tiles"] == rt and plan["kw"] == kp and plan["waves"] == 12
                assert plan["grid"] == -(-M // (16 * rt)) * (N // (256 // kp)) * sk
                ran.add(sk)
                out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr)
                out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr)
                out2 = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, ovr)
                assert norm_rel_err(out.cpu(), ref) < tol_of(dtype), (bits, tile_p, g, dtype, K, N, M, sk, rt, kp)
                assert torch.equal(out1.cpu(), ref1), (bits, tile_p, g, dtype, K, N, M, sk, rt, kp)
                assert torch.equal(out, out2), (bits, tile_p, g, dtype, K, N, M, sk, rt, kp)
                assert _state_words_clean(env), (bits, tile_p, g, dtype, K, N, M, sk, rt, kp)
                if M == 256 and sk == 1 and rt == 4:                 # the XCD-aware block orders (m_block = row tiles per group) are the same numbers
                    for mb in (1, 2, 4):
                        om = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, dev.Overrides(family=6, splitk=1, m_tiles=4, kw=kp, m_block=mb))
                        assert torch.equal(om, out), (bits, tile_p, g, dtype, K, N, kp, mb)
            assert 1 in ran or g == 32 and K > 2048, (K, g, ran)
            assert len(ran) >= 3, (K, g, ran)
    # the planner takes it by itself where it was measured faster (profiles/r04): one workgroup per tile on the MLP widths
    p = dev.get_plan(256, 11008, 4096, 4, 64, 16, 256, torch.float16)
    assert p["family"] == 6 and (p["grid"], p["splitk"]) == (172, 1), p
    p = dev.get_plan(1024, 4096, 4096, 4, 64, 16, 256, torch.bfloat16)
    assert p["family"] == 6 and (p["grid"], p["splitk"]) == (256, 1), p
    p = dev.get_plan(256, 8192, 8192, 4, 64, 16, 256, torch.float16)
    assert p["family"] == 6 and (p["grid"], p["splitk"]) == (256, 2), p
    p = dev.get_plan(256, 4096, 4096, 4, 64, 16, 256, torch.float16)                        # round 6: 64 x 64 tiles over all of K, no seam (rounds 4 / 5: the per-wave kernel)
    assert p["family"] == 6 and (p["grid"], p["splitk"], p["kw"], p["m_tiles"]) == (256, 1, 4, 4), p
    # the automatic plan through the operator, at a BASELINE shape, against the per-wave kernel
    bits, tile_p, g, dtype, K, N = 4, 32, 64, torch.float16, 4096, 11008
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=11)
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    X = (torch.randn(256, K) / 100).to(dtype)
    a = run_qgemm(env, X, Q, S, table, table2, bits, g, tid)
    b = run_qgemm(env, X, Q, S, table, table2, bits, g, tid, dict(family=2))
    assert torch.equal(a, b) or norm_rel_err(a, b.float()) < 2e-4         # same arithmetic contract, different summation order


def test_splitk_seam_under_load(env):
    """The in-launch reduction under uneven load: split-K launches of three weight sets back to back in one hipGraph (the
    workgroups of neighbouring launches overlap at the seams, the slabs and state words are reused at once), replayed; every
    result word for word what the first, isolated launch of that weight set produced (MI355X_MICROARCH.md: test every
    hand-off under uneven load, consumer caches warm, every word)."""
    import bench
    from flute_amd import dev
    # (bits 3, family 3: 2 / 4 K slices of qgemm_block3.h's 128-row blocks, round 5)
    for (bits, M, N, K, sk, fam, dtype, rt, mb) in ((4, 256, 4096, 4096, 4, 6, torch.float16, 8, -1), (4, 200, 2048, 4096, 8, 6, torch.bfloat16, 8, -1),
                                                    (4, 256, 2048, 8192, 2, 6, torch.float16, 8, -1), (4, 256, 4096, 4096, 2, 6, torch.float16, 4, -1),
                                                    (4, 200, 2048, 4096, 4, 6, torch.bfloat16, 4, -1), (4, 16, 4096, 4096, 4, 5, torch.float16, -1, -1),
                                                    (4, 9, 2048, 8192, 8, 5, torch.bfloat16, -1, -1),
                                                    (3, 1024, 4096, 4096, 2, 3, torch.bfloat16, 4, -1), (3, 200, 2048, 4096, 4, 3, torch.float16, 4, -1),
                                                    (3, 256, 8192, 8192, 4, 3, torch.bfloat16, 4, -1)):
        lay = bench.Layer(M, N, K, bits, 64, dtype, env.dev, 3)
        lay.template_id = template_ids_for(env.fa, bits, 32)[0]
        lay.ovr = dev.Overrides(family=fam, splitk=sk, m_tiles=rt, m_block=mb)
        plan = dev.get_plan(M, N, K, bits, 64, lay.template_id, env.num_sms, dtype, lay.ovr)
        assert plan["family"] == fam and plan["splitk"] == sk and plan["splitk_mode"] == 1, plan
        first = [lay.step(c).clone() for c in range(3)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        outs = []
        with torch.cuda.graph(graph):
            for i in range(45):
                outs.append(lay.step(i))
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(o, first[i % 3]) for i, o in enumerate(outs)), (bits, M, N, K, sk, fam)
        assert _state_words_clean(env)
        del lay, outs, graph
        torch.cuda.empty_cache()


def test_skinny_grid_split(env):
    """The skinny MFMA kernel with a grid-level K split (family 5 + splitk, round 4): the K slices of a 64-column slab are
    neighbouring workgroups whose 4-KB partial tiles meet inside the launch (csrc/xwg.h, L form)."""
    from flute_amd import dev
    d = env.dev
    for (tile_p, g, dtype, K, N) in [(32, 64, torch.float16, 4096, 1024), (64, 128, torch.bfloat16, 2048, 1024), (32, 32, torch.float16, 1024, 256),
                                     (32, 64, torch.bfloat16, 14336, 512)]:
        W, Q, S, table, table2 = make_case(env, 4, tile_p, g, dtype, K, N, seed=K % 91 + N % 5)
        What = env.O.dequantize(Q.numpy(), S, table2, 4, g, tile_p).float()
        tid = template_ids_for(env.fa, 4, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for M in (3, 7, 16):
            X = (torch.randn(M, K) / 100).to(dtype)
            ks = torch.randint(0, K, (M,))
            E = torch.zeros(M, K, dtype=dtype)
            E[torch.arange(M), ks] = 1
            ref = X.float() @ What
            ref1 = (table.float()[W.long()] * torch.repeat_interleave(S.float(), g, dim=1).T)[ks].to(dtype)
            ran = 0
            for sk in (2, 4, 7, 8, 14):
                for waves in (-1, 4):
                    ovr = dev.Overrides(family=5, splitk=sk, waves=waves)
                    try:
                        plan = dev.get_plan(M, N, K, 4, g, tid, env.num_sms, dtype, ovr)
                    except RuntimeError:
                        continue
                    if plan["family"] != 5 or plan["splitk"] != sk:
                        continue
                    assert plan["ring_depth"] * plan["waves"] * 32 * sk == K and plan["grid"] == N // 64 * sk and plan["splitk_mode"] == 1
                    ran += 1
                    out = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, 4, g, tid, env.num_sms, ovr)
                    out1 = dev.qgemm_planned(E.to(d), Qd, Sd, td, t2d, env.ws, 4, g, tid, env.num_sms, ovr)
                    out2 = dev.qgemm_planned(X.to(d), Qd, Sd, td, t2d, env.ws, 4, g, tid, env.num_sms, ovr)
                    assert norm_rel_err(out.cpu(), ref) < tol_of(dtype), (tile_p, g, dtype, K, N, M, sk, waves)
                    if dtype == torch.float16:
                        assert torch.equal(out1.cpu(), ref1), (tile_p, g, dtype, K, N, M, sk, waves)
                    else:                                            # bf16: the scale is applied to the fp32 sum of a group run
                        assert norm_rel_err(out1.cpu(), ref1.float()) < tol_of(dtype)
                    assert torch.equal(out, out2) and _state_words_clean(env), (tile_p, g, dtype, K, N, M, sk, waves)
            assert ran, (K, g, M)


# ---------------------------------------------------------------------------
# full BASELINE shapes: size-independent properties, checker runs on the GPU
# ---------------------------------------------------------------------------

FULL_SHAPES = [
    # (bits, tile_p, g, dtype, K, N)
    (4, 32, 64, torch.float16, 4096, 4096),
    (4, 64, 64, torch.float16, 4096, 11008),
    (3, 32, 64, torch.bfloat16, 8192, 8192),
    (4, 32, 64, torch.float16, 8192, 3584),      # TP=8 column shard of 8192x28672
    (2, 64, 128, torch.bfloat16, 4096, 4096),
    # Llama-3-70B linear shapes of the reference's tests/shapes.py:9-15 (BASELINE configs[2], [3])
    (3, 32, 64, torch.bfloat16, 8192, 28672),
    (3, 32, 64, torch.bfloat16, 28672, 8192),    # K = 28672: activations staged in K chunks at M = 4
    (3, 32, 64, torch.bfloat16, 8192, 10240),
    (3, 32, 64, torch.bfloat16, 8192, 1024),     # narrow: grid-level K split
    (4, 32, 64, torch.float16, 8192, 28672),
    (4, 64, 64, torch.float16, 28672, 8192),
    # Gemma-2-9B (configs[4]; tests/shapes.py:53-61)
    (4, 32, 64, torch.float16, 3584, 14336),
    (4, 32, 64, torch.float16, 14336, 3584),
]


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N", FULL_SHAPES)
def test_full_size_properties(env, bits, tile_p, g, dtype, K, N):
    d = env.dev
    torch.manual_seed(K + N + bits)
    W = torch.randint(0, 2 ** bits, (K, N), dtype=torch.uint8, device=d)
    S = torch.randn(N, K // g, device=d).to(dtype)
    table = torch.randn(2 ** bits, device=d).to(dtype)
    table2 = env.utils.make_qmap2_from_qmap(table)
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    Q = env.utils.pack(W, bits, [tid], env.num_sms)
    # host packer == oracle packer on a slice of rows
    assert Q.shape == (bits * N // 16, K)
    # ground truth weights on the GPU (tests/kernel.py:68-70), checker only
    What = table[W.long()] * torch.repeat_interleave(S, g, dim=1).T      # [K, N] in T

    def f(X, t=tid):
        return env.fa.qgemm(X, Q, S, table, table2, env.ws, bits, g, t, env.num_sms)

    # 1. one-hot rows select weight rows exactly (the identity test without a K x K input)
    ks = torch.randint(0, K, (64,), device=d)
    ks[0], ks[1] = 0, K - 1
    X = torch.zeros(64, K, device=d, dtype=dtype)
    X[torch.arange(64), ks] = 1
    for M in (1, 4, 8, 64):
        assert torch.equal(f(X[:M]), What[ks[:M]]), ("one-hot", M)
    # 2. native unpack recovers the codes
    assert torch.equal(env.utils.unpack_codes(Q, bits, tid), W)
    # 3. random input vs torch.mm in fp32 on the GPU
    for M in (1, 16, 256):
        X = (torch.randn(M, K, device=d) / 100).to(dtype)
        ref = X.float() @ What.float()
        err = ((f(X).float() - ref).norm() / ref.norm()).item()
        assert err < tol_of(dtype), (M, err)
    # 4. linearity in X with exactly representable coefficients (2*x1 is exact in T)
    x1 = (torch.randn(1, K, device=d) / 100).to(dtype)
    assert torch.allclose(f(2 * x1).float(), 2 * f(x1).float(), rtol=2e-3, atol=1e-4)
    # 5. row m of a batch does not depend on the other rows beyond accumulation order
    Xb = (torch.randn(8, K, device=d) / 100).to(dtype)
    yb = f(Xb).float()
    y0 = f(Xb[:1]).float()
    assert ((yb[:1] - y0).norm() / y0.norm()).item() < tol_of(dtype)


# ---------------------------------------------------------------------------
# HIGGS vector LUT (tests/higgs.py) and the Hadamard pre-rotation
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", [4, 3, 2])
@pytest.mark.parametrize("vector_size", [2, 1])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_higgs_vector_dequantize_exact(env, bits, vector_size, dtype):
    from flute_amd.integrations import higgs
    d = env.dev
    torch.manual_seed(bits * 4 + vector_size)
    N, K, g = 1024, 1024, 64
    num_codes = 2 ** (bits * vector_size)
    weight_higgs = torch.randint(0, num_codes, (N, K // vector_size), dtype=torch.uint8, device=d)
    scales_higgs = torch.randn((N, K // g), device=d).to(dtype)
    grid = torch.randn((num_codes, vector_size), device=d).to(dtype)
    Q, S, tables, tables2, meta = higgs.prepare_data_transposed(
        weight_higgs, scales_higgs, grid, bits, g, vector_size, dtype, d,
        example_batch_size=1, check_correctness=(vector_size == 1))
    I = torch.eye(K, dtype=dtype, device=d)
    out = env.fa.qgemm(I, Q, S, tables, tables2, env.ws, bits, g, meta.template_id, meta.num_sms)
    ref = env.O.vector_dequantize_higgs(weight_higgs.cpu(), scales_higgs.cpu(), grid.cpu())
    assert torch.equal(out.cpu(), ref.T), (bits, vector_size, dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("h", [2, 4, 8, 64, 256, 512, 1024, 4096, 8192, 16384, 32768])
def test_hadamard_vs_definition(env, dtype, h):
    # parity unpinned in the reference (no test there); oracle = H_h/sqrt(h) in fp64
    torch.manual_seed(h)
    rows = 3 if h >= 4096 else 37
    x = torch.randn(rows, h).to(dtype)
    y = env.fa.hadamard_transform(x.to(env.dev), h).cpu()
    ref = env.O.hadamard_transform(x, h)
    tol = 2e-3 if dtype == torch.float16 else 1.2e-2      # ~1 ulp of T rel. to the row norm
    assert norm_rel_err(y, ref) < tol, (h, norm_rel_err(y, ref))
    # several blocks per row
    if h <= 512:
        x2 = torch.randn(5, 4 * h).to(dtype)
        y2 = env.fa.hadamard_transform(x2.to(env.dev), h).cpu()
        assert norm_rel_err(y2, env.O.hadamard_transform(x2, h)) < tol


def test_qgemm_hadamard(env):
    bits, tile_p, g, dtype, K, N, h = 4, 32, 64, torch.float16, 1024, 512, 512
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=11)
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    d = env.dev
    for M in (1, 5, 40):
        X = (torch.randn(M, K) / 10).to(dtype)
        ref = env.O.qgemm_hadamard(X, Q.numpy(), S, table, table2, bits, g, h, tile_p)
        out = env.fa.qgemm_hadamard(X.to(d), Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws,
                                    bits, g, h, tid, env.num_sms).cpu()
        assert norm_rel_err(out, ref) < 3e-3, (M, norm_rel_err(out, ref))


def test_qgemm_hadamard_fused_equals_two_launches(env):
    """Decode-kernel plans rotate the activations while staging them (one launch); the result must be
    BIT-identical to hadamard_transform followed by qgemm (same fp32 butterflies, one rounding), for
    every block size the fused path takes, both dtypes, M up to the decode limit, K not a multiple
    of 512, chunked staging (large K) and the 3-bit / 2-bit kernels."""
    from flute_amd import dev
    d = env.dev
    lib = env.fa._lib.get()
    cases = [(4, 32, 64, torch.float16, 1024, 512), (4, 64, 64, torch.bfloat16, 3584, 512),
             (2, 32, 64, torch.float16, 1536, 512), (3, 32, 64, torch.bfloat16, 2048, 512),
             (4, 32, 128, torch.float16, 16384, 256)]
    for (bits, tile_p, g, dtype, K, N) in cases:
        W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=K % 89)
        tid = template_ids_for(env.fa, bits, tile_p)[0]
        Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
        for h in (512, 128, 16, 2):
            if K % h:
                continue
            for M in (1, 2, 3, 4):
                # the operator fuses while the rotation is cheaper inside the kernel than as a launch of its own (M x K <= 8192,
                # round 4); forcing the decode family fuses regardless - both forms against rotate-then-multiply
                auto_fused = lib.flute_qgemm_hadamard_fused(0 if dtype == torch.float16 else 1, bits, g, h, M, N, K,
                                                            tid, env.num_sms, env.ws.numel())
                assert auto_fused == (1 if M * K <= 8192 else 0), (bits, K, h, M)
                X = (torch.randn(M, K) / 10).to(dtype).to(d)
                fused = dev.qgemm_planned(X, Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms, dev.Overrides(family=0), hadamard_size=h)
                # the same kernel on pre-rotated activations (M = 3, 4: the plain product may take another kernel)
                two = dev.qgemm_planned(env.fa.hadamard_transform(X, h), Qd, Sd, td, t2d, env.ws, bits, g, tid,
                                        env.num_sms, dev.Overrides(family=0))
                assert torch.equal(fused, two), (bits, dtype, K, h, M)
                auto = env.fa.qgemm_hadamard(X, Qd, Sd, td, t2d, env.ws, bits, g, h, tid, env.num_sms)
                plain = env.fa.qgemm(env.fa.hadamard_transform(X, h), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms)
                assert torch.equal(auto, plain) or norm_rel_err(auto.cpu(), plain.float().cpu()) < 5e-4, (bits, dtype, K, h, M)
    # plans that cannot fuse (MFMA kernel, blocks larger than 512) take the scratch path
    bits, tile_p, g, dtype, K, N = 4, 32, 64, torch.float16, 2048, 512
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=2)
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    for (M, h) in ((1, 1024), (9, 512), (64, 2048)):
        assert lib.flute_qgemm_hadamard_fused(0, bits, g, h, M, N, K, tid, env.num_sms, env.ws.numel()) == 0
        X = (torch.randn(M, K) / 10).to(dtype).to(d)
        out = env.fa.qgemm_hadamard(X, Q.to(d), S.to(d), table.to(d), table2.to(d), env.ws, bits, g, h,
                                    tid, env.num_sms)
        two = env.fa.qgemm(env.fa.hadamard_transform(X, h), Q.to(d), S.to(d), table.to(d), table2.to(d),
                           env.ws, bits, g, tid, env.num_sms)
        assert torch.equal(out, two), (M, h)


def test_cached_plan_entries_keep_their_kernel(env):
    """A plan is cached with its kernel's entry point (32 entries per host thread, replaced in turn): more than three times as
    many distinct calls, so that every entry is evicted and reused, each checked against the oracle - and in a second pass, in
    another order, every call returns the bits of its first.  Small layers (N = 512, K = 512 / 1024, group 64), 2 / 3 / 4 bits
    under an id that leaves the kernel to the planner, both dtypes, M = 1 .. 64; at M = 1 the plain call is followed by the
    fused rotation (Hadamard 512) and, where 1024 divides K, the two-launch rotation (Hadamard 1024) of the same layer.  On
    layers this small the automatic ids reach the decode and the per-wave kernels only (families 0 and 2, whatever the CU
    count), so the 4-bit K = 1024 layers are also called at M = 5, 16 under the id that asks for the skinny MFMA kernel
    (QuantMapMode digit 3, family 5)."""
    d = env.dev
    lib = env.fa._lib.get()
    N, g, tile_p = 512, 64, 32
    calls, families, fused_seen = [], set(), set()
    for bits in (4, 3, 2):
        auto_id = template_ids_for(env.fa, bits, tile_p)[0]
        for K in (512, 1024):
            for dtype in (torch.float16, torch.bfloat16):
                dt = 0 if dtype == torch.float16 else 1
                W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=bits * 100 + K // 512 + dt)
                layer = dict(dev=[t.to(d) for t in (Q, S, table, table2)], bits=bits, dtype=dtype,
                             What=env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float())
                shapes = [(M, auto_id, 0) for M in (1, 2, 3, 5, 16, 17, 33, 64)]
                shapes[1:1] = [(1, auto_id, h) for h in (512, 1024) if K % h == 0]
                if bits == 4 and K == 1024:
                    shapes += [(M, auto_id + 3, 0) for M in (5, 16)]
                for M, tid, h in shapes:
                    calls.append((layer, M, tid, h, (torch.randn(M, K) / 10).to(dtype)))
                    if h:
                        fused_seen.add(lib.flute_qgemm_hadamard_fused(dt, bits, g, h, M, N, K, tid, env.num_sms, env.ws.numel()))
                    else:
                        p = env.fa._lib.Plan()
                        assert lib.flute_qgemm_plan(dt, bits, g, M, N, K, tid, env.num_sms, env.ws.numel(), p) == 0
                        families.add(p.family)
    assert len(calls) > 3 * 32
    assert {0, 2} <= families and families & {5, 6, 7, 8}, families
    assert fused_seen == {0, 1}, fused_seen

    def run(call):
        layer, M, tid, h, X = call
        Qd, Sd, td, t2d = layer["dev"]
        if h:
            return env.fa.qgemm_hadamard(X.to(d), Qd, Sd, td, t2d, env.ws, layer["bits"], g, h, tid, env.num_sms).cpu()
        return env.fa.qgemm(X.to(d), Qd, Sd, td, t2d, env.ws, layer["bits"], g, tid, env.num_sms).cpu()

    first = []
    for call in calls:
        layer, M, tid, h, X = call
        out = run(call)
        Xr = env.O.hadamard_transform(X, h) if h else X
        ref = (Xr.float() @ layer["What"]).to(layer["dtype"])
        err = norm_rel_err(out, ref)
        assert err < tol_of(layer["dtype"]), (layer["bits"], layer["dtype"], M, tid, h, err)
        first.append(out)
    order = torch.randperm(len(calls), generator=torch.Generator().manual_seed(7)).tolist()
    assert order != list(range(len(calls)))
    for i in order:
        layer, M, tid, h, X = calls[i]
        assert torch.equal(run(calls[i]), first[i]), (layer["bits"], layer["dtype"], M, tid, h)


# ---------------------------------------------------------------------------
# boundary behaviour
# ---------------------------------------------------------------------------


def test_batch_dims_errors_and_graph(env):
    bits, tile_p, g, dtype, K, N = 4, 32, 64, torch.float16, 512, 256
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=5)
    d = env.dev
    Qd, Sd, td, t2d = Q.to(d), S.to(d), table.to(d), table2.to(d)
    tid = template_ids_for(env.fa, bits, tile_p)[0]
    What = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).float()
    # leading batch dims are flattened and restored (qgemm.cpp:109-110,195-197)
    X = (torch.randn(2, 3, K) / 100).to(dtype)
    out = env.fa.qgemm(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms)
    assert out.shape == (2, 3, N)
    assert norm_rel_err(out.cpu().reshape(6, N), X.reshape(6, K).float() @ What) < FP16_TOL
    # keyword calling convention of qgemm_v2 (tune.py:508-531)
    out2 = env.fa.qgemm(input=X.to(d), weight=Qd, scales=Sd, table=td, table2=t2d,
                        workspace=env.ws, num_bits=bits, group_size=g, template_id=tid,
                        num_sms=env.num_sms)
    assert torch.equal(out, out2)
    # error convention: RuntimeError with the reference's message prefixes
    with pytest.raises(RuntimeError, match="Unsupported template_id value"):
        env.fa.qgemm(X.to(d), Qd, Sd, td, t2d, env.ws, bits, g, 9999, env.num_sms)
    with pytest.raises((RuntimeError, ValueError)):
        env.fa.qgemm(X.to(d), Qd, Sd, td, t2d, env.ws, 5, g, tid, env.num_sms)
    # no CPU fallback: CPU tensors have no kernel
    with pytest.raises((NotImplementedError, RuntimeError)):
        env.fa.qgemm(X, Q, S, table, table2, torch.zeros(16, dtype=torch.uint8), bits, g, tid, 256)
    # hipGraph capture and replay (qgemm.cpp:103-105: current stream, no host sync)
    xg = X.to(d).reshape(6, K)[:1].contiguous()
    static_out = env.fa.qgemm(xg, Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = env.fa.qgemm(xg, Qd, Sd, td, t2d, env.ws, bits, g, tid, env.num_sms)
    xg.copy_((torch.randn(1, K) / 100).to(dtype))
    graph.replay()
    torch.cuda.synchronize()
    assert norm_rel_err(static_out.cpu(), xg.cpu().float() @ What) < FP16_TOL


def test_prepare_model_flute_matches_fake_quantized_model(env):
    """flute/integrations/base.py:44-200: every nn.Linear becomes a FluteLinear (NF codes, tuned + packed);
    the quantized model must reproduce the fake-quantized fp16 model (kernel-faithful rounding, base.py:84-100)."""
    import copy
    from flute_amd.integrations.base import FluteLinear, prepare_model_flute
    d = env.dev
    torch.manual_seed(4)

    class Block(torch.nn.Module):
        def __init__(self, dim):
            super().__init__()
            self.up = torch.nn.Linear(dim, 2 * dim, bias=True)
            self.act = torch.nn.GELU()
            self.down = torch.nn.Linear(2 * dim, dim, bias=False)
            self.norm = torch.nn.LayerNorm(dim)

        def forward(self, x):
            return self.norm(self.down(self.act(self.up(x))))

    for dtype, bits, dim, tol in ((torch.float16, 4, 256, 2e-3), (torch.bfloat16, 3, 512, 1.5e-2)):
        model = torch.nn.Sequential(Block(dim), Block(dim)).to(device=d, dtype=dtype)
        fake = copy.deepcopy(model)
        prepare_model_flute("model", fake, bits, 64, example_batch_size=1, fake=True)
        prepare_model_flute("model", model, bits, 64, example_batch_size=1)
        assert all(isinstance(b.up, FluteLinear) and isinstance(b.down, FluteLinear) for b in model)
        assert model[0].up.weight.dtype == torch.int16 and model[0].up.bias is not None
        for M in (1, 7, 33):
            x = torch.randn(M, dim, device=d, dtype=dtype)
            with torch.no_grad():                         # inference only: the op has no autograd formula (as the reference)
                y, y_ref = model(x), fake(x)
            assert norm_rel_err(y.cpu(), y_ref.cpu()) < tol, (dtype, M, norm_rel_err(y.cpu(), y_ref.cpu()))
    cpu_model = torch.nn.Sequential(torch.nn.Linear(64, 64)).half()
    with pytest.raises(ValueError):
        prepare_model_flute("m", cpu_model, 4, 64, 1)            # no CPU path


def test_flute_linear_and_repack(env):
    from flute_amd.integrations.base import FluteLinear
    from flute_amd import tune
    d = env.dev
    bits, g, dtype, K, N = 4, 64, torch.float16, 1024, 512
    torch.manual_seed(2)
    codes = torch.randint(0, 16, (K, N), dtype=torch.uint8)
    S = torch.randn(N, K // g).to(dtype).to(d)
    table = torch.tensor(env.O.NF4_VALUES).to(dtype).to(d)
    bias = torch.randn(N).to(dtype).to(d)
    layer = FluteLinear.from_codes(codes, S, table, bits, g, template_id=0, bias=bias)
    x = (torch.randn(3, K) / 10).to(dtype).to(d)
    tile_p = env.fa.TEMPLATE_CONFIGS[(bits, 0)]["TileP"]
    What = env.O.dequantize(layer.weight.cpu().numpy(), S.cpu(), layer.tables2.cpu(), bits, g, tile_p)
    ref = x.cpu().float() @ What.float() + bias.cpu().float()
    assert norm_rel_err(layer(x).cpu(), ref) < 2e-3
    sd = layer.state_dict()
    assert set(k for k in sd if not k.startswith("_")) >= {"weight", "scales", "tables", "tables2", "bias"}
    # a checkpoint "packed on another GPU" (num_sms 108, reference id 132, TileP 32)
    ref_meta = tune.TuneMetaData(M=1, N=N, K=K, num_bits=bits, group_size=g, num_sms=108,
                                 dtype=dtype, device=d, template_id=132)
    Q_ref = torch.from_numpy(env.O.pack(codes.numpy(), bits, 32)).to(d)
    Q_new, meta = tune.maybe_tune_and_repack(Q_ref, S, ref_meta, example_batch_size=1)
    assert meta.num_sms == env.num_sms
    assert torch.equal(env.utils.unpack_codes(Q_new, bits, meta.template_id).cpu(), codes)
    assert tune.TuneMetaData.from_dict(meta.to_dict()) == meta


def test_opcheck(env):
    bits, tile_p, g, dtype, K, N = 4, 32, 64, torch.float16, 256, 128
    W, Q, S, table, table2 = make_case(env, bits, tile_p, g, dtype, K, N, seed=1)
    d = env.dev
    args = (torch.eye(K, dtype=dtype, device=d), Q.to(d), S.to(d), table.to(d), table2.to(d),
            env.ws, bits, g, template_ids_for(env.fa, bits, tile_p)[0], env.num_sms)
    torch.library.opcheck(env.fa.qgemm, args)      # tune.py:350-360


def test_random_launch_plan_fuzz_sweep(env):
    """tools/gpu_fuzz.py: random shape x group size x dtype x batch x TEMPLATE ID (every id is another launch
    plan) against an fp32 evaluation of the reference formula; one-hot rows bit-exact.  A failed experiment of
    round 1 passed every structured sweep and failed 15 % of these draws."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gpu_fuzz.py"), "600", "5"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_bench_dump_outputs_is_the_last_timed_step(env, tmp_path):
    """bench.py --dump-outputs DIR writes what the headline qgemm returned in its last timed step (float32).  The inputs
    are seeded: a second run (the first run's template id given explicitly) dumps the same array, and an eager launch of
    that step on inputs rebuilt here returns it too.  The result line reports the steps asked for and ms_per_step."""
    import json
    import subprocess
    import sys
    import bench
    from flute_amd.nf_utils import NF4_VALUES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps, warmup = 3, 2
    lines, dumps = [], []
    for i in range(2):
        extra = ["--template-id", str(lines[0]["config"]["template_id"])] if i else []
        out = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", str(warmup), "--no-extras", "--no-cpu", "--dump-outputs", str(out)] + extra,
                           cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        dumps.append(np.load(out / "qgemm_out.npy"))
    for line in lines:
        assert line["steps"] == steps and line["ms_per_step"] > 0, line
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (1, 4096)
    assert np.array_equal(dumps[0], dumps[1])
    M, N, K, bits, g = 1, 4096, 4096, 4, 64
    layer = bench.Layer(M, N, K, bits, g, torch.float16, env.dev, bench.copies_for(N, K, bits), NF4_VALUES, seed=0)
    layer.template_id = lines[0]["config"]["template_id"]
    y = layer.step(warmup + steps - 1).float().cpu().numpy()
    assert np.array_equal(y, dumps[0])
