"""flute_qgemm_grouped, flute_amd.qgemm_grouped and integrations.moe.sort_by_expert without a GPU: the export, the C
ABI's refusals (each returned before anything is enqueued, with null pointers), the wrapper's validation on meta
tensors and the grouping against a naive loop."""
import os

import pytest
import torch

import flute_amd
from flute_amd import _lib
from flute_amd.integrations.moe import sort_by_expert
from flute_amd.ops import _validate_grouped
from tests.support import first_template

OK, ERR_NUM_BITS, ERR_GROUP_SIZE, ERR_TEMPLATE_ID, ERR_SHAPE, ERR_DTYPE, ERR_NULL = 0, -1, -2, -3, -4, -7, -9
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flute_amd.h")


def call(dtype=0, bits=4, g=64, E=4, T=8, N=1024, K=512, P=None, tid=0, ptrs=(None,) * 6, num_sms=256):
    P = bits * N // 16 if P is None else P
    return _lib.get().flute_qgemm_grouped(dtype, bits, g, E, T, N, K, P, tid, *ptrs, num_sms, None)


def test_symbol_declared_abi_unchanged():
    assert "flute_qgemm_grouped" in _lib.SYMBOLS
    with open(HEADER) as f:
        text = f.read()
    assert "int flute_qgemm_grouped(" in text
    assert "#define FLUTE_AMD_ABI_VERSION 9" in text
    assert _lib.get().flute_abi_version() == 9
    assert flute_amd.qgemm_grouped is flute_amd.ops.qgemm_grouped


def test_layer_refusals_with_null_pointers():
    assert call(dtype=2) == ERR_DTYPE
    assert call(bits=5) == ERR_NUM_BITS
    assert call(bits=1) == ERR_NUM_BITS
    for g in (0, 16, 48, 512):
        assert call(g=g) == ERR_GROUP_SIZE, g
    assert call(tid=10 ** 6) == ERR_TEMPLATE_ID
    assert call(bits=3, N=512, tid=first_template(3, 64)) == ERR_TEMPLATE_ID      # 3 bits: TileP 32 only


def test_shape_refusals_with_null_pointers():
    assert call(N=1000) == ERR_SHAPE             # N % (J * TileP)
    assert call(N=64, tid=first_template(4, 32)) == ERR_SHAPE
    assert call(N=128, tid=first_template(4, 64)) == ERR_SHAPE      # TileP 64: the column block is 256
    assert call(bits=3, N=256, tid=first_template(3, 32)) == ERR_SHAPE
    assert call(K=480) == ERR_SHAPE              # K % 64
    assert call(K=384, g=256) == ERR_SHAPE       # K % g
    assert call(K=0) == ERR_SHAPE
    assert call(P=255) == ERR_SHAPE
    assert call(E=-1) == ERR_SHAPE
    assert call(T=-1) == ERR_SHAPE


def test_nothing_to_do_is_ok_and_nulls_are_refused():
    assert call(T=0) == OK                       # no launch: the null pointers are never looked at
    assert call(E=0) == OK
    assert call() == ERR_NULL
    fake = (0x1000,) * 6
    for i in range(6):
        ptrs = list(fake)
        ptrs[i] = None
        assert call(ptrs=ptrs) == ERR_NULL, i


def meta(*shape, dtype=torch.float16):
    return torch.empty(shape, dtype=dtype, device="meta")


def args(E=4, T=8, K=512, N=1024, bits=4, g=64, dtype=torch.float16):
    return (meta(T, K, dtype=dtype), meta(E + 1, dtype=torch.int32), meta(E, bits * N // 16, K, dtype=torch.int16),
            meta(E, N, K // g, dtype=dtype), meta(E, 2 ** bits, 2 ** bits, 1, dtype=torch.float32))


def test_validate_grouped():
    x, off, w, s, t2 = args()
    _validate_grouped(x, off, w, s, t2, 4, 64)                 # the valid call passes
    V, T = ValueError, TypeError
    bad = [
        (V, (x[0], off, w, s, t2)),                            # ranks
        (V, (x, off[:, None], w, s, t2)),
        (V, (x, off, w[0], s, t2)),
        (V, (x, off, w, s[0], t2)),
        (V, (x, off, w, s, t2[0])),
        (T, (x.float(), off, w, s.float(), t2)),               # dtypes
        (T, (x, off, w, s.to(torch.bfloat16), t2)),
        (T, (x, off, w.to(torch.int32), s, t2)),
        (T, (x, off, w, s, t2.half())),
        (T, (x, off.long(), w, s, t2)),                        # offsets: int32 only
        (V, (x, off[:4], w, s, t2)),                           # offsets: E + 1 elements
        (V, (x, meta(6, dtype=torch.int32), w, s, t2)),
        (V, (x, off, w[:, :255], s, t2)),                      # P != b N / 16
        (V, (x, off, w[:3], s, t2)),                           # E differs
        (V, (x, off, w, s, t2[:3])),
        (V, (x, off, w, s, t2[:, :8])),
        (V, (x[:, :448], off, w, s, t2)),                      # K != weight's
    ]
    for exc, a in bad:
        with pytest.raises(exc):
            _validate_grouped(*a, 4, 64)
    with pytest.raises(V):
        _validate_grouped(x, off, w, s, t2, 5, 64)             # bits
    with pytest.raises(V):
        _validate_grouped(x, off, w, s, t2, 4, 48)             # group size
    # K a multiple of g but not of max(64, g)
    with pytest.raises(V):
        _validate_grouped(*args(K=96, g=32), 4, 32)
    with pytest.raises(V):
        _validate_grouped(*args(K=384, g=128)[:3], meta(4, 1024, 1), t2, 4, 256)      # g does not divide K
    # the public function validates before any device call, then refuses tensors that are not on a GPU
    with pytest.raises(T):
        flute_amd.qgemm_grouped(x, off.long(), w, s, t2, 4, 64, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        flute_amd.qgemm_grouped(x, off, w, s, t2, 4, 64, 0)


def naive_grouping(ids, E):
    flat = [int(v) for row in ids.tolist() for v in row]
    perm, offsets = [], [0]
    for e in range(E):
        perm += [i for i, v in enumerate(flat) if v == e]       # ascending i: equal ids keep their order
        offsets.append(len(perm))
    return perm, offsets


@pytest.mark.parametrize("T,k,E,seed", [(1, 2, 8, 0), (37, 2, 4, 1), (64, 2, 8, 2), (5, 4, 16, 3), (200, 1, 3, 4)])
def test_sort_by_expert_equals_naive_loop(T, k, E, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, E, (T, k), generator=gen)
    if E > 2:
        ids[ids == 1] = 2                                       # expert 1 receives nothing; many ties on 2
    perm, offsets = sort_by_expert(ids, E)
    ref_perm, ref_off = naive_grouping(ids, E)
    assert offsets.dtype == torch.int32 and offsets.shape == (E + 1,)
    assert offsets.tolist() == ref_off
    assert perm.tolist() == ref_perm
    if E > 2:
        assert ref_off[1] == ref_off[2]


def test_sort_by_expert_all_to_the_last_expert():
    ids = torch.full((6, 2), 3, dtype=torch.int64)
    perm, offsets = sort_by_expert(ids, 4)
    assert perm.tolist() == list(range(12))
    assert offsets.tolist() == [0, 0, 0, 0, 12]


def test_sort_by_expert_ids_outside_the_experts_sort_last():
    """Ids outside [0, E) belong to no expert: they sort behind every expert's rows, in their original order."""
    ids = torch.tensor([[2, 7], [-1, 0], [2, 4], [0, 2]])
    perm, offsets = sort_by_expert(ids, 4)
    assert offsets.tolist() == [0, 2, 2, 5, 5]
    assert perm.tolist() == [3, 6, 0, 4, 7, 1, 2, 5]


def test_sort_by_expert_uses_no_op_of_data_dependent_shape():
    """On meta tensors an op whose output shape depends on the data (bincount, nonzero, unique) cannot run."""
    perm, offsets = sort_by_expert(torch.empty((5, 2), dtype=torch.int64, device="meta"), 8)
    assert perm.shape == (10,) and offsets.shape == (9,) and offsets.dtype == torch.int32
