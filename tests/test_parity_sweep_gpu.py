"""GPU parity tests for the configurations round 1 only timed ("next round" item 1):

  * BASELINE.json configs[4] end to end: `higgs.prepare_data` (pair codebook) + `qgemm_hadamard(512)` on the
    Gemma-2-9B shapes of the reference's tests/shapes.py:53-61, against `oracle.qgemm_hadamard`;
  * M = 1024 / 4096 (the prefill plans) on 4096x4096 and 4096x11008, tests/kernel.py:160;
  * the reference's whole SUPPORTED_SHAPES list (tests/shapes.py:1-96) x M in {1, 3, 16, 32, 53, 64, 256}
    (tests/kernel.py:137-169 + the batch sizes of BASELINE.json configs[1]).  By default every shape runs with
    EIGHT (num_bits, group_size, dtype, table, TileP) combinations - a window sliding over the 60 legal ones
    (3 x 3 x 2 x 2 at TileP 32, 2 x 3 x 2 x 2 at TileP 64: the reference has no 3-bit packer for TileP 64,
    utils.py:137-139), so that every combination occurs about seven times over the list; one pytest case per
    (shape, combination); FLUTE_SLOW=1 runs the full cross product;
  * product packer == oracle packer on row slices of a full-size matrix;
  * Hadamard: distance of the HIP kernel to the reference kernel's STAGED arithmetic
    (oracle.hadamard_transform_staged) next to its distance to the definition.

Checkers for full-size shapes run on the GPU in fp32 (torch), as the reference's own test does
(tests/kernel.py:68-71); the CPU oracle is used where it finishes in seconds.
"""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import exact_cases as XC
from tests.qgemm_cases import GEMMA2_9B, SUPPORTED_SHAPES
from tests.support import env, first_template, norm_rel_err  # noqa: F401

pytestmark = pytest.mark.gpu

FP16_TOL = 1e-3          # north_star
BF16_TOL = 4e-3          # what tests/test_oracle.py grants the oracle; the reference accepts 1.1e-2 (tests/kernel.py:13)

COMBOS = [c + (32,) for c in itertools.product([4, 3, 2], [64, 128, 256], [torch.float16, torch.bfloat16], [True, False])] + \
         [c + (64,) for c in itertools.product([4, 2], [64, 128, 256], [torch.float16, torch.bfloat16], [True, False])]
assert len(COMBOS) == 60
# a fixed shuffle, so that a window of consecutive entries mixes bit widths, group sizes, dtypes and TileP
COMBOS = [COMBOS[(i * 23) % 60] for i in range(60)]
assert len(set(COMBOS)) == 60
SLOW = os.environ.get("FLUTE_SLOW") == "1"
PER_SHAPE = 60 if SLOW else 8
SWEEP_MS = (1, 3, 16, 32, 53, 64, 256)


def tol_of(dtype):
    return FP16_TOL if dtype == torch.float16 else BF16_TOL


def packable(N, bits, tile_p):
    return N % (tile_p * (16 if bits == 3 else 16 // bits)) == 0


def served_template(e, M, N, K, bits, g, dtype, tile_p):
    """The template id the PRODUCT serves for this call - the shipped table's entry for the (shape, M bucket), as
    FluteLinear / tune_and_pack / bench.py take it (flute_amd/data/gfx950_tuned.json, ~9.5 k keys: ids 28, 12, 5, 29, 24, 20, 18, ...)
    - when it exists and shares the packed matrix's TileP; else the first id of that TileP (the automatic plan)."""
    from flute_amd import tune
    # (the table keys 2- / 4-bit layers twice - any TileP, and TileP 32 - and 3-bit layers, which exist for TileP 32 only, once)
    tid = tune.lookup_tuned(M, N, K, bits, g, e.num_sms, dtype, 32 if (tile_p == 32 and bits != 3) else None)
    if tid is not None and e.fa.TEMPLATE_CONFIGS[(bits, tid)]["TileP"] == tile_p and \
            e.utils.is_template_supported(M, N, K, bits, tid, e.num_sms, g, dtype):
        return tid
    return first_template(bits, tile_p)


def check_shape_case(e, N, K, bits, g, dtype, uniform, Ms, seed, tile_p=32, tuned=False):
    """tests/kernel.py::test_integer for one (shape, config): identity -> one-hot rows bit-exact, random rows
    within tolerance, evaluated against the reference formula in fp32 on the GPU.  tuned: every batch size runs the
    template id of the shipped table (tune.py:294-392 checks the id it has just tuned), not the first id."""
    d = e.dev
    if not packable(N, bits, tile_p) or K % g:
        pytest.skip(f"N={N} K={K} not packable for b={bits} g={g}")
    torch.manual_seed(seed)
    W = torch.randint(0, 2 ** bits, (K, N), dtype=torch.uint8, device=d)      # includes the top code
    S = torch.randn(N, K // g, device=d).to(dtype)
    table = (torch.arange(2 ** bits, device=d) if uniform else torch.randn(2 ** bits, device=d)).to(dtype)
    table2 = e.utils.make_qmap2_from_qmap(table)
    tid0 = first_template(bits, tile_p)
    tid_of = (lambda M: served_template(e, M, N, K, bits, g, dtype, tile_p)) if tuned else (lambda M: tid0)
    Q = e.utils.pack(W, bits, [tid0], e.num_sms)                                # (the layout depends on TileP only)
    Sx = torch.repeat_interleave(S, g, dim=1).T                                 # [K, N]
    # identity input, sampled: 64 one-hot rows (first, last, random k) reproduce round_T(table*S) exactly
    ks = torch.randint(0, K, (64,), device=d)
    ks[0], ks[1] = 0, K - 1
    E = torch.zeros(64, K, device=d, dtype=dtype)
    E[torch.arange(64), ks] = 1
    What_rows = table[W[ks].long()] * Sx[ks]
    for M in sorted(set(min(m, 64) for m in Ms)):
        out = e.fa.qgemm(E[:M], Q, S, table, table2, e.ws, bits, g, tid_of(M), e.num_sms)
        assert torch.equal(out, What_rows[:M]), ("one-hot", N, K, bits, g, dtype, M, tid_of(M))
    del E
    What = (table[W.long()] * Sx).float()                                        # [K, N] checker, fp32 copy
    W_exact = table.double()[W.long()] * Sx.double()                             # lut * s before any rounding (componentwise bound)
    del W, Sx
    for M in Ms:
        X = (torch.randn(M, K, device=d) / 100).to(dtype)
        out = e.fa.qgemm(X, Q, S, table, table2, e.ws, bits, g, tid_of(M), e.num_sms)
        ref = X.float() @ What
        err = ((out.float() - ref).norm() / ref.norm()).item()
        assert err < tol_of(dtype), (N, K, bits, g, dtype, uniform, M, tid_of(M), err)
        XC.assert_componentwise(out, X, W_exact, K, dtype, what=(N, K, bits, g, dtype, uniform, M, tid_of(M)))
    del What, W_exact
    torch.cuda.empty_cache()


@pytest.mark.parametrize("slot", range(PER_SHAPE))
@pytest.mark.parametrize("idx", range(len(SUPPORTED_SHAPES)))
def test_supported_shapes_sweep(env, idx, slot):
    N, K = SUPPORTED_SHAPES[idx]
    bits, g, dtype, uniform, tile_p = COMBOS[(idx * PER_SHAPE + slot) % len(COMBOS)]
    # odd slots run the ids the product serves (the shipped table's entry per batch size), even slots the first id
    check_shape_case(env, N, K, bits, g, dtype, uniform, SWEEP_MS, seed=idx * 64 + slot, tile_p=tile_p, tuned=bool(slot & 1))


@pytest.mark.parametrize("N,K", [(4096, 4096), (11008, 4096)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_prefill_batches(env, N, K, dtype):
    """tests/kernel.py:160 (M = 1024) and the M = 4096 prefill line of bench.py: tuned template, rel-Frobenius
    and exact one-hot rows spread over every 16-row tile of the batch."""
    d = env.dev
    bits, g = 4, 64
    torch.manual_seed(N + K)
    W = torch.randint(0, 2 ** bits, (K, N), dtype=torch.uint8, device=d)
    S = torch.randn(N, K // g, device=d).to(dtype)
    table = torch.randn(2 ** bits, device=d).to(dtype)
    table2 = env.utils.make_qmap2_from_qmap(table)
    What = table[W.long()] * torch.repeat_interleave(S, g, dim=1).T
    from flute_amd import tune
    for M in (1024, 4096):
        X = (torch.randn(M, K, device=d) / 100).to(dtype)
        Q, meta = tune.tune_and_pack(X, W, bits, g, check_correctness=False)
        out = env.fa.qgemm(X, Q, S, table, table2, env.ws, bits, g, meta.template_id, meta.num_sms)
        ref = X.float() @ What.float()
        err = ((out.float() - ref).norm() / ref.norm()).item()
        assert err < tol_of(dtype), (N, K, dtype, M, meta.template_id, err)
        ks = torch.randint(0, K, (M,), device=d)
        E = torch.zeros(M, K, device=d, dtype=dtype)
        E[torch.arange(M), ks] = 1
        out = env.fa.qgemm(E, Q, S, table, table2, env.ws, bits, g, meta.template_id, meta.num_sms)
        assert torch.equal(out, What[ks]), ("one-hot", N, K, dtype, M)


@pytest.mark.parametrize("N,K", GEMMA2_9B)
def test_higgs_pair_codebook_hadamard_gemma2(env, N, K):
    """BASELINE.json configs[4]: HIGGS vector_size = 2 codebook (an arbitrary 256 x 2 table, not an outer
    product) + hadamard_size = 512 pre-rotation, W4G64, Gemma-2-9B shapes, through `higgs.prepare_data`
    (flute/integrations/higgs.py:8-97) and `qgemm_hadamard` (qgemm.cpp:214-244).  K = 3584 = 7 x 512."""
    from flute_amd.integrations import higgs
    d = env.dev
    bits, g, vs, h, dtype = 4, 64, 2, 512, torch.float16
    if K % h:
        pytest.skip("hadamard_size must divide K")
    torch.manual_seed(N * 3 + K)
    codes = torch.randint(0, 2 ** (bits * vs), (N, K // vs), dtype=torch.uint8, device=d)
    scales = torch.randn((N, K // g), device=d).to(dtype)
    grid = torch.randn((2 ** (bits * vs), vs), device=d).to(dtype)
    Q, S, tables, tables2, meta = higgs.prepare_data_transposed(
        codes, scales, grid, bits, g, vs, dtype, d, example_batch_size=1, check_correctness=False)
    What = env.O.vector_dequantize_higgs(codes, scales, grid).T.float()          # [K, N], tests/higgs.py:7-17
    for M in (1, 4, 16):
        X = (torch.randn(M, K, device=d) / 10).to(dtype)
        out = env.fa.qgemm_hadamard(X, Q, S, tables, tables2, env.ws, bits, g, h, meta.template_id,
                                    meta.num_sms)
        Xr = env.O.hadamard_transform(X.cpu(), h).to(d)                             # definition, rounded to T
        ref = Xr.float() @ What
        err = ((out.float() - ref).norm() / ref.norm()).item()
        assert err < 3e-3, (N, K, M, err)
    # the lookup + scale part is exact: one-hot rows through the plain op select rows of the codebook weight
    ks = torch.randint(0, K, (16,), device=d)
    E = torch.zeros(16, K, device=d, dtype=dtype)
    E[torch.arange(16), ks] = 1
    out = env.fa.qgemm(E, Q, S, tables, tables2, env.ws, bits, g, meta.template_id, meta.num_sms)
    assert torch.equal(out.float(), What[ks].to(dtype).float()), ("pair codebook one-hot", N, K)
    # the whole path through the CPU oracle (closed-form unpack of the packed matrix, table2 lookup, rotation)
    # where it finishes in seconds
    if N * K <= 16 * 1024 * 1024:
        tile_p = env.fa.TEMPLATE_CONFIGS[(bits, meta.template_id)]["TileP"]
        X = (torch.randn(4, K) / 10).to(dtype)
        ref = env.O.qgemm_hadamard(X, Q.cpu().numpy(), S.cpu(), tables.cpu(), tables2.cpu(), bits, g, h, tile_p)
        out = env.fa.qgemm_hadamard(X.to(d), Q, S, tables, tables2, env.ws, bits, g, h, meta.template_id,
                                    meta.num_sms).cpu()
        assert norm_rel_err(out, ref) < 3e-3, (N, K, norm_rel_err(out, ref))


@pytest.mark.parametrize("bits,tile_p", [(4, 32), (4, 64), (2, 32), (2, 64), (3, 32)])
def test_product_packer_equals_oracle_on_row_slices(env, bits, tile_p):
    """utils.pack (closed form, runs on the GPU) against oracle.pack (pinned to the reference's packers by
    tests/golden) on column-block slices of a full-size matrix: a slice of whole column blocks packs to the
    corresponding rows of Q."""
    d = env.dev
    K, N = 4096, 4096
    torch.manual_seed(bits * 100 + tile_p)
    W = torch.randint(0, 2 ** bits, (K, N), dtype=torch.uint8, device=d)
    tid = first_template(bits, tile_p)
    Q = env.utils.pack(W, bits, [tid], env.num_sms).cpu().numpy()
    blk = tile_p * (16 if bits == 3 else 16 // bits)
    Wc = W.cpu().numpy()
    for b0 in (0, N // blk // 2, N // blk - 1):
        cols = slice(b0 * blk, (b0 + 1) * blk)
        Qo = env.O.pack(Wc[:, cols], bits, tile_p)
        if bits == 3:
            P1 = N // 16
            rows = np.concatenate([np.arange(b0 * 32, b0 * 32 + 32), P1 + np.arange(b0 * 64, b0 * 64 + 64)])
        else:
            rows = np.arange(b0 * tile_p, (b0 + 1) * tile_p)
        assert np.array_equal(Q[rows], Qo), (bits, tile_p, b0)
    # and the whole matrix for one moderate case
    assert np.array_equal(Q, env.O.pack(Wc, bits, tile_p))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("h", [16, 64, 512, 4096])
def test_hadamard_distance_to_reference_staged_arithmetic(env, dtype, h):
    """The reference has no test for hadamard_transform: this reports and bounds the distance of the
    HIP kernel (fp32 butterflies, one rounding) to an emulation of the reference kernel's staged arithmetic
    (one 16x16 factor per tensor-core pass, every pass rounded to T: hadamard_transform_cuda.cu:56-73).
    The HIP result must be at least as close to the exact transform as the staged emulation is."""
    torch.manual_seed(h)
    x = torch.randn(64, h).to(dtype)
    y = env.fa.hadamard_transform(x.to(env.dev), h).cpu()
    exact = (x.double() @ env.O.hadamard_matrix(h))
    staged = env.O.hadamard_transform_staged(x, h)
    d_def = ((y.double() - exact).norm() / exact.norm()).item()
    d_staged_def = ((staged.double() - exact).norm() / exact.norm()).item()
    d_to_staged = ((y.double() - staged.double()).norm() / exact.norm()).item()
    ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    print(f"hadamard {dtype} h={h}: |hip-exact|={d_def:.2e} |staged-exact|={d_staged_def:.2e} |hip-staged|={d_to_staged:.2e}")
    assert d_def <= d_staged_def * 1.05 + 1e-7
    stages = (h.bit_length() - 1 + 3) // 4
    assert d_to_staged < 1.5 * (stages + 1) * ulp, (h, d_to_staged)
