"""The give-up path of the in-launch split-K reduction (csrc/xwg.h, E form) on the hardware, in every suite run.

A healthy launch of the shipped library never exhausts the poll bound (FLUTE_XWG_SPIN_LIMIT = 4096), so the branch a preempted
workgroup takes - publish the own share too, mark it abandoned, the last arriver sweeps and combines it from the slabs - runs
here in the two variant libraries the normal build makes (csrc/Makefile, SPIN_UNITS): poll limit 0, where EVERY owner that is
not last gives up, and poll limit 1, where claims and give-ups meet in one tile.  Both copies of the E form run: the epilogue
of qgemm_splitk.h (family 6) and xwg_seam (the 3-bit 128-row blocks of qgemm_block3.h, family 3), at 2 and at 4 shares; the
L-form plans run too and must not notice the limit.

The variants are loaded NEXT to the package's library (same ABI, ctypes) and launch into a private workspace: state words
zero, everything behind them one NaN pattern no finite partial sum can produce.  Per case and variant:
  1. exact data: round_T(X @ W_exact) bit for bit against the fp64 product, guards, coverage, state words, repeat (run_exact);
  2. random data: word for word the SHIPPED library's output for the same plan - one summation order whoever combines (owner
     first, then the other slices ascending), which exact data cannot see; at 4 shares also on operands whose slices cancel
     (cancelling_operands), where another order changes most words and not one in 2^16;
  3. that the give-up path ran, from the canary left in the slab region (`region` bytes behind the state words).  Every slab
     store is a whole 1-KB fragment with no row predicate, so with nsh shares a healthy launch leaves every slice's own share
     untouched, region / nsh, while an all-give-up launch leaves only the last arriver's own share, region / nsh^2: that is
     asserted at limit 0, the interval between the two (in whole shares) at limit 1, nothing left in the L form.  Which form a
     case takes is decided from the kernel's rule - E iff the 2 or 4 slices divide a wave's row tiles - never from the count;
  4. state words zero after every launch, the canary behind `region` untouched.
"""
import copy
import ctypes
import os

import pytest
import torch

from tests import exact_cases as E
from tests.qgemm_cases import DevLayer, check_plan, get_layer, guarded_qgemm, run_exact, seed_of, state_words_clean
from tests.support import bits_by_size, env, first_template  # noqa: F401

pytestmark = pytest.mark.gpu

VARIANTS = ("spin0", "spin1")
FLAG_BYTES = 65536                   # xwg.h kXwgFlagBytes: the state words; the slabs start behind them
CANARY = 0x7FC5A5A5                  # a NaN in fp32: no sum of finite partials stores it


# ---------------------------------------------------------------------------
# the variant libraries and the private workspace (used by this module only)
# ---------------------------------------------------------------------------

def load_variant(lib_mod, tag):
    path = os.path.join(os.path.dirname(os.path.abspath(lib_mod.__file__)), "csrc", "libflute_amd_%s.so" % tag)
    assert os.path.exists(path), "%s is missing: the normal build makes it (csrc/Makefile)" % path
    lib = ctypes.CDLL(path)
    for name, (res, args) in lib_mod.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


@pytest.fixture(scope="module")
def envs(env):
    """{"shipped" | variant: a shallow copy of Env with that library and the private workspace}; caches and layers are shared."""
    ws = torch.zeros(env.ws.numel(), dtype=torch.uint8, device=env.dev)       # the size the plans were made for
    out = {}
    for tag in ("shipped",) + VARIANTS:
        e = copy.copy(env)
        e.ws = ws
        if tag != "shipped":
            e.lib = load_variant(env.lib_mod, tag)
            assert e.lib._handle != env.lib._handle and e.lib.flute_abi_version() == env.lib.flute_abi_version()
        out[tag] = e
    return out


def fresh(e):
    """State words zero (they must be already), the canary everywhere behind them."""
    assert state_words_clean(e)
    e.ws[FLAG_BYTES:].view(torch.int32).fill_(CANARY)


def canary_left(e, region):
    return 4 * int((e.ws[FLAG_BYTES:FLAG_BYTES + region].view(torch.int32) == CANARY).sum().item())


def tail_intact(e, region):
    return bool(torch.all(e.ws[FLAG_BYTES + region:].view(torch.int32) == CANARY))


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

def shares_of(fam, plan):
    """The kernel's rule: the E form with nsh = splitk shares iff the 2 or 4 slices divide the row tiles a wave holds at the
    seam - qgemm_splitk.h: HR = row tiles / K parts; xwg_seam in qgemm_block3.h: NR = 8 (128-row blocks); 0: the L form."""
    per_wave = plan["m_tiles"] // plan["kw"] if fam == 6 else 8
    sk = plan["splitk"]
    return sk if sk in (2, 4) and per_wave % sk == 0 else 0


def _planned(kw, M, ovr):
    """The plan of a case when the module is collected (host only, for the 256 CUs of an MI355X; a forced split does not depend on
    the CU count - the test plans again on the device and must find the same split), None where the planner refuses."""
    from flute_amd import dev
    try:
        return dev.get_plan(M, kw["N"], kw["K"], kw["bits"], kw["g"], first_template(kw["bits"], kw["tile_p"]), 256, kw["dtype"],
                            dev.Overrides(**ovr))
    except RuntimeError:
        return None


def _cases():
    """[(id, family, layer kwargs, M, overrides, expected plan fields)], the smallest launch first, grouped by layer:
    one tile x 2 slices; every entry of the forced matrix in families 6 and 3 that meets inside the launch (the small layers,
    K <= 4096, N <= 1536, M <= 257, and at the end the two full-size layers, whose automatic family-6 plans at M = 16 cut K
    too) - E form at 2 and 4 shares of qgemm_splitk.h, 2 shares of xwg_seam, the L form at 3 .. 16 slices and where the slices
    do not divide the row tiles; the 4-share case of xwg_seam, which the matrix lacks."""
    out = [(6, E._lay(4, 1024, 128, 32, E.BF16), 17, dict(family=6, splitk=2, m_tiles=8, kw=2), dict(family=6, splitk=2, m_tiles=8, kw=2))]
    out += [c for c in E.forced_matrix() if c[0] in (6, 3)]
    lay = next(c[1] for c in E.forced_matrix() if c[0] == 3 and c[1]["bits"] == 3)
    ovr = dict(family=3, m_tiles=4, splitk=4)
    while (_planned(lay, 257, ovr) or {}).get("splitk") != 4 and lay["K"] < 65536:       # the smallest K the planner cuts four ways
        lay = dict(lay, K=2 * lay["K"])
    out += [(3, lay, M, ovr, dict(family=3, m_block=5, splitk=4)) for M in (13, 257)]
    keyed = []
    for fam, kw, M, ovr, exp in out:
        plan = _planned(kw, M, ovr)
        if plan is None or plan["family"] != fam or plan["splitk"] <= 1 or plan["splitk_mode"] != 1:
            continue
        cid = "f%d-b%d-K%d-N%d-M%d-sk%d-rt%d-kp%d" % (fam, kw["bits"], kw["K"], kw["N"], M, plan["splitk"], plan["m_tiles"], plan["kw"])
        keyed.append(((kw["K"] * kw["N"], E.layer_key(kw), plan["grid"], plan["splitk"], M), (cid, fam, kw, M, ovr, exp)))
    keyed.sort(key=lambda c: c[0])
    return [c for _, c in keyed]


CASES = _cases()


def test_cases_reach_both_copies_of_the_e_form():
    forms = {(fam, shares_of(fam, _planned(kw, M, ovr))) for _, fam, kw, M, ovr, _ in CASES}
    assert forms == {(6, 0), (6, 2), (6, 4), (3, 2), (3, 4)}, forms
    assert len({c[0] for c in CASES}) == len(CASES)
    first = _planned(*[CASES[0][i] for i in (2, 3, 4)])
    assert (first["grid"], first["splitk"]) == (2, 2), first                   # the smallest launch runs first: one tile, 2 slices


def variant_plan(e, dl, M, ovr):
    lay = dl.lay
    plan = e.lib_mod.Plan()
    e.check(e.lib.flute_qgemm_plan_ex(0 if lay.dtype == torch.float16 else 1, lay.bits, lay.g, M, lay.N, lay.K, dl.tid, e.num_sms,
                                      e.ws.numel(), e.dev_mod.Overrides(**ovr), plan))
    return plan.as_dict()


def random_operands(e, dl, M, seed):
    """The layer's codes under a randn table and randn scales, and randn / 100 activations."""
    lay = dl.lay
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(2 ** lay.bits, generator=gen).to(lay.dtype)
    S = torch.randn(lay.N, lay.K // lay.g, generator=gen).to(lay.dtype)
    X = (torch.randn(M, lay.K, generator=gen) / 100).to(lay.dtype)
    rdl = DevLayer.__new__(DevLayer)
    rdl.__dict__.update(dl.__dict__)
    rdl.set_operands(e.dev, dl.Q, S, table, e.utils.make_qmap2_from_qmap(table))
    return rdl, X


def cancelling_operands(e, dl, M, plan, seed):
    """Operands on which the ORDER of a four-way sum reaches the output (on randn data an order change moves the fp32 sum by
    an ulp, which one output word in ~2^16 shows after the rounding to T).  Every K slice holds the weights of the first
    (codes and scales repeated); the activations of slice 1 are minus those of slice 0, both 2^18 times the others'.  The
    partials of slices 0 and 1 are then +-P exactly: added to each other first they vanish, with a small partial between
    them they swallow its low bits.  Asserted below on fp32 sums of the dequantized weights: owner first and the others
    ascending - the order xwg.h promises - and another order give different words in most of share 2."""
    lay = dl.lay
    T, sk, kps = lay.dtype, plan["splitk"], plan["k_per_split"]
    assert sk == 4 and kps * sk == lay.K and kps % lay.g == 0
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(2 ** lay.bits, generator=gen).to(T)
    S = torch.randn(lay.N, kps // lay.g, generator=gen).to(T).repeat(1, sk)
    x = torch.randn(M, lay.K, generator=gen) / 100
    x[:, :kps] *= 2.0 ** 18
    X = x.to(T)
    X[:, kps:2 * kps] = -X[:, :kps]
    cdl = DevLayer.__new__(DevLayer)
    cdl.__dict__.update(dl.__dict__)
    Q = e.utils.pack(lay.W[:kps].repeat(sk, 1).to(e.dev), lay.bits, [dl.tid], e.num_sms)
    cdl.set_operands(e.dev, Q, S, table, e.utils.make_qmap2_from_qmap(table))
    Wd = e.fa.dequantize(cdl.Q, cdl.S, cdl.table2, lay.bits, lay.g, dl.tid).float()          # [N, K]
    p = [X[:, s * kps:(s + 1) * kps].to(e.dev).float() @ Wd[:, s * kps:(s + 1) * kps].T for s in range(sk)]
    promised, other = ((p[2] + p[0]) + p[1]) + p[3], ((p[2] + p[3]) + p[1]) + p[0]
    assert float((promised.to(T) != other.to(T)).float().mean()) > 0.5, "the data does not show the order of the sum"
    return cdl, X


@pytest.mark.parametrize("tag", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_giveup_case(envs, case, tag):
    cid, fam, kw, M, ovr, exp = case
    ship, var = envs["shipped"], envs[tag]
    dl = get_layer(ship, kw)
    plan = check_plan(ship, dl, M, ovr, dict(exp, splitk_mode=1))
    assert plan is not None and plan["splitk"] > 1, (cid, plan)
    assert cid.endswith("-sk%d-rt%d-kp%d" % (plan["splitk"], plan["m_tiles"], plan["kw"])), (cid, plan)
    assert variant_plan(var, dl, M, ovr) == plan, cid
    nsh = shares_of(fam, plan)
    ntiles = plan["grid"] // plan["splitk"]
    region = plan["workspace_needed"] - FLAG_BYTES
    assert region > 0 and region % (plan["splitk"] * ntiles * 1024) == 0 and FLAG_BYTES + region < var.ws.numel()

    # 1. exact data
    fresh(var)
    run_exact(var, dl, M, ovr, seed_of(fam, M, tuple(sorted(ovr.items()))))
    assert tail_intact(var, region), cid

    # 2. random data: the shipped library's words, computed once per case
    if ship.cache.get("case") != cid:
        ship.cache.clear()
        rdl, X = random_operands(ship, dl, M, seed_of("giveup", cid))
        fresh(ship)
        D = guarded_qgemm(ship, rdl, X, ovr)
        left = canary_left(ship, region)
        assert tail_intact(ship, region), cid
        print("shipped library, %s: %d of %d slab bytes untouched (%s)" % (
            cid, left, region, "E form, %d shares: a healthy launch leaves %d" % (nsh, region // nsh) if nsh else "L form: none"))
        ship.cache.update(case=cid, rdl=rdl, X=X, D=D)
        if nsh == 4:                                             # ... and on data that shows the order of a four-way sum
            cdl, Xc = cancelling_operands(ship, dl, M, plan, seed_of("cancel", cid))
            fresh(ship)
            ship.cache.update(cdl=cdl, Xc=Xc, Dc=guarded_qgemm(ship, cdl, Xc, ovr))
    if nsh == 4:
        fresh(var)
        Dc = guarded_qgemm(var, ship.cache["cdl"], ship.cache["Xc"], ovr)
        differ = int((bits_by_size(Dc) != bits_by_size(ship.cache["Dc"])).sum().item())
        assert differ == 0, "%s, %s, cancelling slices: %d output words differ from the shipped library's" % (cid, tag, differ)
        assert tail_intact(var, region), cid
    rdl, X, D_ship = ship.cache["rdl"], ship.cache["X"], ship.cache["D"]
    fresh(var)
    D = guarded_qgemm(var, rdl, X, ovr)
    left = canary_left(var, region)
    assert tail_intact(var, region), cid
    differ = int((bits_by_size(D) != bits_by_size(D_ship)).sum().item())
    assert differ == 0, "%s, %s: %d output words differ from the shipped library's" % (cid, tag, differ)

    # 3. the give-up path ran
    if nsh == 0:
        assert left == 0, (cid, tag, left)
    elif tag == "spin0":
        assert region % (nsh * nsh) == 0 and left == region // (nsh * nsh), (cid, tag, left, region)
    else:
        share = region // (nsh * nsh * ntiles)               # one slice's partial of one share of one tile
        assert region // (nsh * nsh) <= left <= region // nsh and left % share == 0, (cid, tag, left, region)


# ---------------------------------------------------------------------------
# under load: launches of three weight sets back to back in one captured graph
# ---------------------------------------------------------------------------

# (bits, M, N, K, slices, family, dtype, row tiles): one E-form shape per copy of the protocol, out of test_splitk_seam_under_load's
# list the smallest with more than one tile per slice - family 6 at 2 and at 4 shares, xwg_seam at 2
LOAD_SHAPES = [(4, 256, 2048, 8192, 2, 6, torch.float16, 8), (4, 256, 4096, 4096, 4, 6, torch.float16, 8),
               (3, 1024, 4096, 4096, 2, 3, torch.bfloat16, 4)]


@pytest.mark.parametrize("tag", VARIANTS)
@pytest.mark.parametrize("shape", LOAD_SHAPES, ids=["f%d-b%d-sk%d" % (s[5], s[0], s[4]) for s in LOAD_SHAPES])
def test_giveup_under_load(envs, shape, tag):
    """45 overlapping launches (three weight sets in turn) in one hipGraph, replayed three times: every output word for word the
    shipped library's isolated result for its weight set, state words clean, nothing written behind the slabs.  At limit 1 a
    tile's claims and give-ups mix, and the sweep sees both kinds of bits."""
    import bench
    bits, M, N, K, sk, fam, dtype, rt = shape
    ship, var = envs["shipped"], envs[tag]
    ship.layers.clear()
    torch.cuda.empty_cache()
    lay = bench.Layer(M, N, K, bits, 64, dtype, ship.dev, 3)
    tid = first_template(bits, 32)
    ovr = ship.dev_mod.Overrides(family=fam, splitk=sk, m_tiles=rt)
    plan = ship.dev_mod.get_plan(M, N, K, bits, 64, tid, ship.num_sms, dtype, ovr)
    assert plan["family"] == fam and plan["splitk"] == sk and plan["splitk_mode"] == 1 and shares_of(fam, plan) == sk, plan
    assert plan["grid"] // sk > 1
    region = plan["workspace_needed"] - FLAG_BYTES

    def launch(e, c, out):
        rc = e.lib.flute_qgemm_ex(0 if dtype == torch.float16 else 1, bits, 64, 0, M, N, K, lay.Q[c].shape[0],
                                  lay.X.data_ptr(), lay.Q[c].data_ptr(), out.data_ptr(), lay.S[c].data_ptr(), lay.table.data_ptr(),
                                  lay.table2.data_ptr(), None, e.ws.data_ptr(), e.ws.numel(), tid, e.num_sms, ovr, e.stream_ptr(e.dev))
        e.check(rc)

    first = []
    with torch.cuda.device(ship.dev):
        for c in range(3):                                       # the shipped library, each weight set alone
            fresh(ship)
            first.append(torch.empty(M, N, dtype=dtype, device=ship.dev))
            launch(ship, c, first[c])
            torch.cuda.synchronize()
        fresh(var)
        outs = [torch.full((M, N), float("nan"), dtype=dtype, device=var.dev) for _ in range(45)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i, o in enumerate(outs):
                launch(var, i % 3, o)
        for _ in range(3):
            for o in outs:
                o.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(bits_by_size(o), bits_by_size(first[i % 3])) for i, o in enumerate(outs)), (shape, tag)
            assert state_words_clean(var) and tail_intact(var, region), (shape, tag)
    del lay, outs, graph, first
    torch.cuda.empty_cache()
