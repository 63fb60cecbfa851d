"""The lean decode kernel's prologue (qgemm_fast.h): four ways a reordered prologue can go wrong, one case each.

Every case launches the lean kernel (the resolved plan must say `one_shot 4`: no other kernel can pass in its place) and the
round-4 one-shot kernel (`one_shot = 1`) on the same operands and compares the outputs with `torch.equal`.  The activation rows
are one-hot, so both kernels' documented arithmetic allows one answer only - round_T(table entry * group scale), one product and
one rounding - and the outputs are also held against that closed form.

  * an image read before it is complete: the 256 pair entries are all distinct and non-zero, the hot positions draw every entry,
    and every launch gets the codebook rotated by another amount - the image a workgroup finds in LDS from the launch before is
    a wrong one;
  * a scale used before it is read: every (column, group) has its own scale, one launch per group, g = 64 and g = 256;
  * a piece count that is no power of two: K = 3584, seven pieces per wave;
  * rows past M: three rows on the four-row instantiation.

N = 128 throughout: the packed format holds whole blocks of 4 * TileP columns, so 128 is the narrowest layer the library takes
(the shapes were set as N = 64, which flute_qgemm_plan refuses as unsupported)."""
import pytest
import torch

from tests.support import env, first_template  # noqa: F401

N = 128
DTYPE = torch.float16

# (name, M, K, g, rows per pass of the lean plan, pieces per wave)
CASES = {
    "image": (1, 2048, 64, 1, 4),
    "scales_g64": (1, 4096, 64, 1, 8),
    "scales_g256": (1, 4096, 256, 1, 8),
    "seven_pieces": (1, 3584, 64, 1, 7),
    "rows_past_m": (3, 2048, 64, 4, 4),
}


def _pairs():
    """256 distinct non-zero pair entries, exact in fp16: entry i = ((i + 1) / 16, -(i + 1) / 32)."""
    i = torch.arange(256, dtype=torch.float64)
    return torch.stack([(i + 1) / 16, -(i + 1) / 32], dim=-1)


def _scales(K, g):
    """One fp16 value per (column, group), all distinct: the bit patterns 0x2000 + index lie in [2^-7, 2)."""
    G = K // g
    assert N * G <= 0x2000
    return (torch.arange(N * G, dtype=torch.int32) + 0x2000).to(torch.int16).view(torch.float16).reshape(N, G).clone()


def _hot_positions(name, K, g):
    if name == "image":
        # every piece, several lanes, both elements of a pair
        return [512 * (t % 4) + 8 * ((17 * t + 5) % 64) + 2 * (t % 4) + (t // 4) % 2 for t in range(8)]
    if name.startswith("scales"):
        return [grp * g + (grp * 29 + 3) % g for grp in range(K // g)]          # one per group
    if name == "seven_pieces":
        return [512 * (t % 7) + (37 * t + 11) % 512 for t in range(14)]         # two per piece
    return [512 * (t % 4) + (53 * t + 7) % 512 for t in range(12)]              # rows_past_m: three per launch


def _codes(name, K, hot):
    gen = torch.Generator().manual_seed(len(name) + K)
    W = torch.randint(0, 16, (K, N), generator=gen, dtype=torch.uint8)
    if name == "image":
        # launch t draws entries 128 * (t % 2) + column: launches 0 .. 3 take every entry's first element, 4 .. 7 its second
        for t, k in enumerate(hot):
            idx = 128 * (t % 2) + torch.arange(N)
            W[k & ~1] = (idx >> 4).to(torch.uint8)
            W[k | 1] = (idx & 15).to(torch.uint8)
    return W


def _run_case(env, name):
    M, K, g, mb, depth = CASES[name]
    dev, utils = env.dev_mod, env.utils
    tid = first_template(4, 32)
    lean = dev.Overrides(family=0, one_shot=4)
    plan = dev.get_plan(M, N, K, 4, g, tid, env.num_sms, DTYPE, lean)
    assert (plan["family"], plan["one_shot"], plan["waves"], plan["kw"], plan["ring_depth"], plan["m_block"]) == (0, 4, 4, 1, depth, mb), plan
    ref_plan = dev.get_plan(M, N, K, 4, g, tid, env.num_sms, DTYPE, dev.Overrides(family=0, one_shot=1))
    assert ref_plan["family"] == 0 and ref_plan["one_shot"] in (1, 2), ref_plan        # either form of the round-4 one-shot kernel

    hot = _hot_positions(name, K, g)
    W = _codes(name, K, hot)
    S = _scales(K, g)
    pairs = _pairs()
    Q = utils.pack(W, 4, [tid], env.num_sms).to(env.dev)
    Sd = S.to(env.dev)
    launches = []
    want = []
    for t in range(len(hot) // M):
        ks = [hot[t * M + m] for m in range(M)]
        pt = torch.roll(pairs, shifts=37 * t, dims=0)                             # another codebook for every launch
        table2 = pt.to(DTYPE).view(16, 16, 2).contiguous().view(torch.float32)
        X = torch.zeros(M, K, dtype=DTYPE)
        exp = torch.empty(M, N, dtype=torch.float64)
        for m, k in enumerate(ks):
            X[m, k] = 1.0
            idx = (W[k & ~1].long() << 4) | W[k | 1].long()
            exp[m] = pt[idx, k & 1] * S[:, k // g].double()
        launches.append((X.to(env.dev), pt[:16, 0].to(DTYPE).to(env.dev), table2.to(env.dev)))
        want.append(exp.to(DTYPE))
    outs = {}
    for key, ovr in (("lean", lean), ("one_shot", dev.Overrides(family=0, one_shot=1))):
        outs[key] = [dev.qgemm_planned(X, Q, Sd, table, table2, env.ws, 4, g, tid, env.num_sms, ovr)
                     for (X, table, table2) in launches]
    torch.cuda.synchronize()
    got = torch.stack(outs["lean"]).cpu()
    ref = torch.stack(outs["one_shot"]).cpu()
    assert got.shape == (len(launches), M, N)
    assert torch.equal(got, ref), (name, int((got != ref).sum()))
    assert torch.equal(got, torch.stack(want)), (name, int((got != torch.stack(want)).sum()))
    return got


@pytest.mark.gpu
def test_table_image_is_complete_before_the_first_lookup(env):  # noqa: F811
    got = _run_case(env, "image")
    # every pair entry was drawn: launches 0 .. 3 and 4 .. 7 each return 256 distinct magnitudes per scale-free ratio
    assert got.shape[0] == 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scales_g64", "scales_g256"])
def test_every_group_scale_is_read_before_its_use(env, name):  # noqa: F811
    got = _run_case(env, name)
    assert got.shape[0] == CASES[name][1] // CASES[name][2]                       # one launch per group


@pytest.mark.gpu
def test_seven_pieces_per_wave(env):  # noqa: F811
    _run_case(env, "seven_pieces")


@pytest.mark.gpu
def test_rows_past_m_on_the_four_row_instantiation(env):  # noqa: F811
    got = _run_case(env, "rows_past_m")
    assert got.shape[1] == 3


def test_cases_plan_the_lean_kernel_on_a_full_chip():
    """Without a GPU: on 256 CUs every case resolves to the lean kernel's plan (so the GPU cases cannot pass on another kernel)."""
    from flute_amd import dev
    tid = first_template(4, 32)
    for name, (M, K, g, mb, depth) in CASES.items():
        plan = dev.get_plan(M, N, K, 4, g, tid, 256, DTYPE, dev.Overrides(family=0, one_shot=4))
        assert (plan["family"], plan["one_shot"], plan["waves"], plan["kw"], plan["ring_depth"], plan["m_block"]) == (0, 4, 4, 1, depth, mb), (name, plan)
        hot = _hot_positions(name, K, g)
        assert len(hot) % M == 0 and all(0 <= k < K for k in hot) and len(set(hot)) == len(hot), name
        S = _scales(K, g)
        assert S.unique().numel() == S.numel() and bool(torch.isfinite(S).all()), name
    # the image case draws all 256 entries, each element once
    hot = _hot_positions("image", 2048, 64)
    W = _codes("image", 2048, hot)
    drawn = set()
    for k in hot:
        idx = (W[k & ~1].long() << 4) | W[k | 1].long()
        drawn |= {(int(i), k & 1) for i in idx}
    assert len(drawn) == 512
