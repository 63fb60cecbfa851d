"""flute_amd.dequantize / flute_dequantize on the GPU: the dense weight [N, K] must equal round_T(table2-lookup * scale)
bit for bit - against the reference's fixtures (qgemm on an identity, D_identity), the CPU oracle, utils.reconstruct and
the exact weights of tests/exact_cases.Layer - and a direct ABI call must write exactly its [N, k_count] block."""

import pytest
import torch

from tests import exact_cases as XC
from tests.grouped_cases import random_case
from tests.support import bits16, env, first_template  # noqa: F401

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16


def test_golden_fixtures(env, golden):
    """Every reference fixture (the HIGGS pair codebooks included): dequantize == qgemm(I) of the reference."""
    d = env.dev
    tid = first_template(golden.num_bits, golden.tile_p)
    out = env.fa.dequantize(torch.as_tensor(golden.Q).to(d), golden.S.to(d), golden.table2.to(d), golden.num_bits,
                            golden.group_size, tid).cpu()
    ref = golden.D_identity.T
    assert out.shape == ref.shape and out.dtype == golden.dtype
    assert torch.equal(out, ref), golden.name            # by value: the identity GEMM's sum turns -0.0 into +0.0
    nz = ref != 0
    assert torch.equal(bits16(out)[nz], bits16(ref)[nz]), golden.name


def sweep_cases():
    out = []
    i = 0
    for bits in (4, 3, 2):
        for tile_p in ((32, 64) if bits != 3 else (32,)):
            block = tile_p * (16 if bits == 3 else 16 // bits)
            for g in (32, 64, 128, 256):
                for dtype in (F16, BF16):
                    shapes = [(max(64, g), block), (1024 + max(64, g), 3 * block), (8192, block)]
                    for K, N in shapes:
                        out.append((bits, tile_p, g, dtype, K, N, i % 2 == 1))
                        i += 1
    return out


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,pair", sweep_cases())
def test_against_oracle(env, bits, tile_p, g, dtype, K, N, pair):
    d = env.dev
    Q, S, table2 = random_case(env, bits, tile_p, g, dtype, K, N, seed=K * 7 + N + g + bits, pair=pair)
    out = env.fa.dequantize(Q.to(d), S.to(d), table2.to(d), bits, g, first_template(bits, tile_p)).cpu()
    ref = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).T
    assert torch.equal(bits16(out), bits16(ref))


@pytest.mark.parametrize("bits,K,N,tile_p,dtype,pair", [
    (4, 8192, 28672, 32, F16, False), (4, 28672, 8192, 64, BF16, True), (2, 4096, 11008 // 512 * 512, 64, F16, False),
    (3, 8192, 8192, 32, BF16, False)])
def test_large_layers_exact(env, bits, K, N, tile_p, dtype, pair):
    """Full-size layers: against the exact weights of tests/exact_cases (lut * scale is exact in T there)."""
    d = env.dev
    lay = XC.Layer(bits, K, N, 64, dtype, seed=bits * 1000 + K + N, tile_p=tile_p, pair=pair)
    tid = first_template(bits, tile_p)
    Q = env.utils.pack(lay.W.to(d), bits, [tid], env.num_sms)
    out = env.fa.dequantize(Q, lay.S.to(d), lay.table2.to(d), bits, 64, tid)
    for n0 in range(0, N, 4096):
        n1 = min(N, n0 + 4096)
        ref = lay.w_exact(n0, n1, device=d).T.to(dtype)
        assert torch.equal(bits16(out[n0:n1]), bits16(ref)), (n0, n1)
    del out, Q
    torch.cuda.empty_cache()


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,pair", [
    (4, 32, 64, F16, 2048, 1024, False), (4, 64, 128, BF16, 1024, 2048, True), (3, 32, 32, F16, 1024, 1024, False),
    (2, 32, 256, BF16, 2048, 512, False), (2, 64, 64, F16, 512, 4096, True)])
def test_against_reconstruct(env, bits, tile_p, g, dtype, K, N, pair):
    d = env.dev
    Q, S, table2 = random_case(env, bits, tile_p, g, dtype, K, N, seed=3 + K + N, pair=pair)
    n = 2 ** bits
    table = torch.zeros(n, dtype=dtype)
    tid = first_template(bits, tile_p)
    Qd, Sd, t2 = Q.to(d), S.to(d), table2.to(d)
    out = env.fa.dequantize(Qd, Sd, t2, bits, g, tid)
    rec = env.utils.reconstruct(Qd, Sd, table.to(d), t2, env.ws, bits, g, tid, env.num_sms)
    assert out.shape == rec.shape == (N, K)
    assert torch.equal(out, rec)                             # by value (signed zeros)
    nz = rec != 0
    assert torch.equal(bits16(out)[nz], bits16(rec.contiguous())[nz])


def raw_call(env, dtype, bits, g, N, K, k_begin, k_count, Q, S, table2, Wptr, tid):
    lib = env.lib
    with torch.cuda.device(env.dev):
        return lib.flute_dequantize(0 if dtype == F16 else 1, bits, g, N, K, Q.shape[0], k_begin, k_count, Q.data_ptr(),
                                    S.data_ptr(), table2.data_ptr(), Wptr, tid, torch.cuda.current_stream(env.dev).cuda_stream)


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,chunks", [
    (4, 32, 64, F16, 4096, 1024, (0, 64, 1024, 3008, 4096)), (3, 32, 128, BF16, 2048, 512, (0, 1024, 2048)),
    (2, 64, 32, BF16, 1536, 1024, (0, 192, 256, 1536))])
def test_k_chunks_concatenate(env, bits, tile_p, g, dtype, K, N, chunks):
    d = env.dev
    Q, S, table2 = random_case(env, bits, tile_p, g, dtype, K, N, seed=11 + K, pair=False)
    tid = first_template(bits, tile_p)
    Qd, Sd, t2 = Q.to(d), S.to(d), table2.to(d)
    whole = env.fa.dequantize(Qd, Sd, t2, bits, g, tid)
    parts = []
    for k0, k1 in zip(chunks[:-1], chunks[1:]):
        part = torch.empty(N, k1 - k0, dtype=dtype, device=d)
        assert raw_call(env, dtype, bits, g, N, K, k0, k1 - k0, Qd, Sd, t2, part.data_ptr(), tid) == 0
        parts.append(part)
    assert torch.equal(bits16(torch.cat(parts, 1)), bits16(whole))


@pytest.mark.parametrize("bits,tile_p,g,dtype,K,N,k0,kc", [
    (4, 32, 64, F16, 1024, 512, 256, 512), (4, 64, 256, BF16, 2048, 2048, 0, 2048), (3, 32, 32, F16, 512, 1024, 448, 64),
    (2, 32, 128, BF16, 1024, 256, 128, 768)])
def test_direct_abi_writes_exactly_its_block(env, bits, tile_p, g, dtype, K, N, k0, kc):
    """Into a NaN-filled buffer with 64 KB guard bands on each side: every element of [N, kc] is written (no NaN is
    left: the tables and scales are finite), the guard bands are untouched, and the block equals the oracle's."""
    d = env.dev
    Q, S, table2 = random_case(env, bits, tile_p, g, dtype, K, N, seed=5 + K + k0, pair=True)
    tid = first_template(bits, tile_p)
    Qd, Sd, t2 = Q.to(d), S.to(d), table2.to(d)
    guard = 32768
    buf = torch.full((guard + N * kc + guard,), XC.NAN_BITS[dtype], dtype=torch.int16, device=d)
    assert raw_call(env, dtype, bits, g, N, K, k0, kc, Qd, Sd, t2, buf[guard:].data_ptr(), tid) == 0
    torch.cuda.synchronize()
    assert torch.all(buf[:guard] == XC.NAN_BITS[dtype]) and torch.all(buf[guard + N * kc:] == XC.NAN_BITS[dtype])
    block = buf[guard:guard + N * kc].view(dtype).view(N, kc).cpu()
    assert not torch.isnan(block).any()
    ref = env.O.dequantize(Q.numpy(), S, table2, bits, g, tile_p).T[:, k0:k0 + kc]
    assert torch.equal(bits16(block), bits16(ref))
    # k_count == 0 writes nothing
    assert raw_call(env, dtype, bits, g, N, K, 0, 0, Qd, Sd, t2, buf.data_ptr(), tid) == 0
    torch.cuda.synchronize()
    assert torch.all(buf[:guard] == XC.NAN_BITS[dtype])


def test_opcheck(env):
    d = env.dev
    Q, S, table2 = random_case(env, 4, 32, 64, F16, 512, 256, seed=1, pair=False)
    torch.library.opcheck(env.fa.dequantize, (Q.to(d), S.to(d), table2.to(d), 4, 64, first_template(4, 32)))
