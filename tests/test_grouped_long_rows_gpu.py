"""The grouped kernels past 2 and 4 GiB of rows, at K = 7168 (tests/long_rows_cases.py has the shape, the constants and the
helpers; tests/test_long_rows_host.py pins the same premises on the host): the plain and weighted forward in the block form
at the last T its eligibility rule admits and in the row form past it, the input gradient in both forms, the fused SwiGLU
launch over a source of 4 GiB, and the grouped scale and table gradients.

What a wrap would corrupt are the rows past 2 or 4 GiB only, so every result is compared on every element: the GEMM forms
against round_T of the exact product (one allowed value per element; the reference is an fp32 torch.mm per expert, checked
bit for bit against fp64 on the first and last 64 rows, on ROW_2G +- 1 and ROW_4G +- 1 and on the first and last row of every
expert), the GLU launch against the fp64 formula within grouped_cases.assert_glu's account and bit for bit against the same
launch on a compact copy of the rows it reads.  Every launch goes through the C ABI into a buffer guarded on both sides with
the type's NaN bits and must leave the guards and its inputs as they were and every element it owes written.

The second dimension is the smallest a layer of the layout has: N = F = 256 in the forward, and in the input gradient one
column block of the layout (128 columns at 4 bits, 256 at 2 bits; a packed layer has no fewer).  4 bits, g = 64, TileP 32,
fp16 unless a case says otherwise."""
import pytest
import torch

from tests import exact_cases as XC
from tests import glu_block_cases as GB
from tests import grouped_cases as GC
from tests import long_rows_cases as LC
from tests import scale_grad_ref as SR
from tests.support import make_env

pytestmark = pytest.mark.gpu

F16, BF16 = LC.F16, LC.BF16
K, GIB = LC.K, LC.GIB
ERR_SHAPE = -4
AUTO, ROWS, BLOCKS = 0, 1, 2                 # flute_grouped_form_t
IG_AUTO, IG_SLABS, IG_BLOCKS = 0, 1, 2       # flute_grouped_input_grad_form_t
N_FWD = 256


@pytest.fixture(scope="module")
def env():
    e = make_env()
    torch.cuda.reset_peak_memory_stats(e.dev)
    yield e
    print("peak device memory: %.2f GiB" % (torch.cuda.max_memory_allocated(e.dev) / GIB))
    e.cache.clear()
    torch.cuda.empty_cache()


def need(gib):
    """Skip when the device cannot hold the case (peak of this module: DESIGN.md, "Long rows").  Blocks the allocator holds
    free count as free: the cache is kept between the tests, so the 4 GiB buffers of one test are the next one's."""
    free, _ = torch.cuda.mem_get_info()
    free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free < gib * GIB:
        pytest.skip("needs %.0f GiB of free device memory, %.1f GiB free" % (gib, free / GIB))


def dtype_id(dtype):
    return 0 if dtype == F16 else 1


def off_tensor(env, off):
    return torch.tensor(off, dtype=torch.int32, device=env.dev)


def activations(env, dtype):
    """X [R_LONG, K] of the type and its bit copy, once per module; the last row of every prefix the cases use is a witness."""
    key = ("X", dtype)
    if key not in env.cache:
        X = LC.device_x(LC.R_LONG, XC.seed_of("long rows x", str(dtype)), dtype, (LC.T_EDGE - 1, LC.T_EDGE, LC.R_LONG - 1))
        assert torch.equal(X.abs().amax(), torch.tensor(4.0, dtype=dtype, device=env.dev))
        env.cache[key] = (X, LC.snapshot(X))
    return env.cache[key]


def stack(env, bits, N, dtype, E):
    key = ("stack", bits, N, dtype, E)
    if key not in env.cache:
        env.cache[key] = LC.ExactStack(env, bits, N, dtype, E, "grouped")
    return env.cache[key]


def witnessed(env, st, X, T, off):
    """The last row of the prefix is the accumulator witness of the expert that serves it."""
    e = max(i for i in range(st.E) if off[i + 1] > off[i])
    key = ("witness", id(st), e)
    if key not in env.cache:
        assert off[e + 1] == T and bool((X[T - 1] == 4).all())
        st.witness(X[T - 1], e)
        env.cache[key] = True


# ---- 1 and 2: plain and weighted -------------------------------------------------------------------------------------------

def forward_launch(env, st, X, T, off, rw, form, out):
    """flute_qgemm_grouped_ex / _weighted_ex on X[:T] into `out`; returns the code."""
    offd = off_tensor(env, off)
    head = (dtype_id(st.dtype), st.bits, st.g, st.E, T, st.N, K, st.Q.shape[1], st.tid, X.data_ptr(), offd.data_ptr(),
            st.Q.data_ptr(), st.S.data_ptr(), st.t2.data_ptr())
    tail = (out.out.data_ptr(), env.num_sms, env.stream_ptr(env.dev), form)
    with torch.cuda.device(env.dev):
        if rw is None:
            rc = env.lib.flute_qgemm_grouped_ex(*head, *tail)
        else:
            rc = env.lib.flute_qgemm_grouped_weighted_ex(*head, rw.data_ptr(), *tail)
    torch.cuda.synchronize()
    return rc


def forward_check(env, st, X, snap, T, off, rw, form, R, what):
    """One launch against R: guards, coverage (every served row written; the rows from off[E] on unwritten in the plain
    launch and +0 in the weighted one), inputs, every element."""
    out = LC.Guarded((T, st.N), st.dtype, env.dev)
    small = (st.Q, st.S, st.t2, rw)
    before = LC.snapshot(*small)
    env.check(forward_launch(env, st, X, T, off, rw, form, out))
    out.assert_guards()
    served = off[-1]
    out.assert_written(0, served)
    if rw is None:
        out.assert_unwritten(served, T)
    else:
        out.assert_zero_bits(served, T)
    LC.assert_unchanged(before, *small)
    LC.assert_unchanged(snap, X)
    LC.assert_equal_rows(out.out, R, what, 0, served)
    print("%s: exact" % (what,))


def forward_case(env, bits, dtype, table, T, weighted):
    counts = LC.TABLES[table](T)
    off = LC.served_offsets(counts)
    st = stack(env, bits, N_FWD, dtype, len(counts))
    X, snap = activations(env, dtype)
    witnessed(env, st, X, T, off)
    rw = LC.device_row_weights(T, XC.seed_of("long rows rw", table, T)) if weighted else None
    R = st.reference(X[:T], off, rw)
    st.cross_check(X, R, off, LC.check_rows(off, T), rw)
    mode = "weighted" if weighted else "plain"
    auto = env.dev_mod.grouped_form(mode, st.E, T, st.N, K, bits, st.g, st.tid, env.num_sms, dtype)
    return st, X, snap, off, counts, rw, R, mode, auto


@pytest.mark.parametrize("bits,dtype,table", [(4, F16, "fat"), (4, F16, "spread"), (4, BF16, "spread"), (2, F16, "fat")])
def test_block_form_at_the_last_t_it_admits(env, bits, dtype, table):
    """T = T_EDGE, forced and automatic (which must say "blocks").  fat: one expert's relative offsets reach the descriptor
    limit and its last block's idle rows request offsets up to 127 rows past its end; spread: the expert bases pass 2^31 while
    every relative offset is small.  Weighted also with offsets[E] = T - 300: the zero fill then runs at the end of 4 GiB of
    rows.  (2 bits: the plain launch only.)"""
    need(40)
    T = LC.T_EDGE
    for weighted in ((False,) if bits == 2 else (False, True)):
        st, X, snap, off, counts, rw, R, mode, auto = forward_case(env, bits, dtype, table, T, weighted)
        assert auto == "blocks"
        for form in (BLOCKS, AUTO):
            forward_check(env, st, X, snap, T, off, rw, form, R, (mode, table, bits, str(dtype), T, "form", form))
        if weighted:
            short = LC.served_offsets(counts, T - 300)
            assert short[-1] == T - 300
            for form in (BLOCKS, AUTO):
                forward_check(env, st, X, snap, T, short, rw, form, R, (mode, table, T, "offsets[E] = T - 300", "form", form))
        del R


@pytest.mark.parametrize("dtype,table,T", [(F16, "fat", LC.T_EDGE + 1), (F16, "spread", LC.T_EDGE + 1), (F16, "fat", LC.R_LONG),
                                           (F16, "spread", LC.R_LONG), (BF16, "spread", LC.R_LONG)])
def test_row_form_past_the_edge(env, dtype, table, T):
    """T = T_EDGE + 1 and R_LONG: forcing blocks is refused and writes nothing; the automatic form and "rows" run the row
    form - 64-bit row bases - and equal the reference.  At R_LONG the spread table's last expert starts past 2^32."""
    need(40)
    bits = 4
    for weighted in (False, True):
        st, X, snap, off, counts, rw, R, mode, auto = forward_case(env, bits, dtype, table, T, weighted)
        assert auto == "rows"
        out = LC.Guarded((T, st.N), dtype, env.dev)
        assert forward_launch(env, st, X, T, off, rw, BLOCKS, out) == ERR_SHAPE
        out.assert_untouched()
        del out
        op = env.fa.qgemm_grouped_weighted if weighted else env.fa.qgemm_grouped
        args = (X[:T], off_tensor(env, off), st.Q, st.S, st.t2) + ((rw,) if weighted else ())
        with pytest.raises(RuntimeError):
            op(*args, bits, st.g, st.tid, env.num_sms, form="blocks")
        for form in (AUTO, ROWS):
            forward_check(env, st, X, snap, T, off, rw, form, R, (mode, table, str(dtype), T, "form", form))
        if weighted:
            short = LC.served_offsets(counts, T - 300)
            forward_check(env, st, X, snap, T, short, rw, ROWS, R, (mode, table, T, "offsets[E] = T - 300"))
        del R


# ---- 3: the input gradient -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,dtype,table", [(4, F16, "fat"), (4, F16, "spread"), (4, BF16, "spread"), (2, F16, "spread")])
def test_input_gradient_past_4_gib(env, bits, dtype, table):
    """dY [R_LONG, N], dX [R_LONG, 7168]: 4 GiB of output rows behind 64-bit row bases, slabs and blocks (2 bits: blocks), plain
    and with row_weight (then with offsets[E] = R - 300: the tail is +0).  The reference is dY @ W_e in fp32 - exact: dY
    integers in [-4, 4], N 4 max|w| < 2^21, asserted by the stack - and the two forms give equal bits."""
    need(40)
    Rn = LC.R_LONG
    N = XC.cols_per_block(bits, 32)
    counts = LC.TABLES[table](Rn)
    st = stack(env, bits, N, dtype, len(counts))
    dY = LC.device_ints(Rn, N, XC.seed_of("long rows dy", bits, str(dtype), table), dtype)
    rw_all = LC.device_row_weights(Rn, XC.seed_of("long rows ig rw", table))
    assert env.dev_mod.grouped_input_grad_form(st.E, Rn, N, K, bits, st.g, st.tid, env.num_sms, dtype) == "blocks"
    out = LC.Guarded((Rn, K), dtype, env.dev)
    for rw in (None, rw_all):
        off = LC.served_offsets(counts, None if rw is None else Rn - 300)
        R = st.reference(dY, off, rw, backward=True)
        st.cross_check(dY, R, off, LC.check_rows(off, Rn), rw, backward=True)
        offd = off_tensor(env, off)
        inputs = (dY, st.Q, st.S, st.t2, rw)
        before = LC.snapshot(*inputs)
        first = None
        for form in ((IG_BLOCKS,) if bits == 2 else (IG_SLABS, IG_BLOCKS)):
            out.refill()
            with torch.cuda.device(env.dev):
                rc = env.lib.flute_qgemm_grouped_input_grad_ex(
                    dtype_id(dtype), bits, st.g, st.E, Rn, N, K, st.Q.shape[1], st.tid, dY.data_ptr(), offd.data_ptr(),
                    st.Q.data_ptr(), st.S.data_ptr(), st.t2.data_ptr(), None if rw is None else rw.data_ptr(), None, None, None,
                    None, out.out.data_ptr(), env.num_sms, env.stream_ptr(env.dev), form)
            env.check(rc)
            torch.cuda.synchronize()
            out.assert_guards()
            out.assert_written()
            out.assert_zero_bits(off[-1])
            LC.assert_unchanged(before, *inputs)
            what = ("input gradient", table, bits, str(dtype), "row_weight" if rw is not None else "plain", "form", form)
            LC.assert_equal_rows(out.out, R, what)
            if first is None and bits != 2:
                first = out.out.clone()
            elif first is not None:
                LC.assert_equal_bits(out.out, first, "slabs and blocks")
            print("%s: exact" % (what,))
        del R, first
    del out, dY


# ---- 4: the fused SwiGLU launch ------------------------------------------------------------------------------------------

GLU_R = 4096
GLU_COUNTS = GB.BLOCK_COUNTS[:-1] + [GLU_R - sum(GB.BLOCK_COUNTS[:-1])]       # the last expert scaled up: 29 blocks
GLU_NSRC = 64 + 64 + 3 + 2 + 3000                                               # source rows that hold data
GLU_PAD = 160                                                                   # NaN rows around Xsrc: more than a block has
GLU_F = 256


def source_rows(Tsrc, n, seed):
    """n distinct source rows, sorted: the first 64, the last 64 (the witness, Tsrc - 1, is the last), ROW_2G - 1 .. ROW_2G + 1,
    ROW_4G - 1 .. ROW_4G where they exist, and random rows up to n."""
    must = set(range(64)) | set(range(Tsrc - 64, Tsrc)) | {LC.ROW_2G - 1, LC.ROW_2G, LC.ROW_2G + 1}
    must |= {r for r in (LC.ROW_4G - 1, LC.ROW_4G) if r < Tsrc}
    assert len(must) <= n
    for r in torch.randperm(Tsrc, generator=torch.Generator().manual_seed(seed)).tolist():
        if len(must) == n:
            break
        must.add(r)
    out = sorted(must)
    assert len(out) == n and out[-1] == Tsrc - 1
    return out


def glu_case(env, dtype):
    """Two exact stacks, the compact source rows [GLU_NSRC, K] scaled by 2^-p, the compact `rows` [GLU_R] and the fp64 reference
    with every premise of assert_glu's bound asserted (glu_block_cases.premised_case), once per type."""
    key = ("glu", dtype)
    if key not in env.cache:
        seed0 = XC.seed_of("long rows glu", str(dtype)) // 2
        layers, Xi, rows, ref, tries = GB.premised_case(4, 32, 64, dtype, K, GLU_F, False, GLU_COUNTS, GLU_NSRC, seed0)
        case = GB.GluBlockCase(env, layers)
        env.cache[key] = dict(case=case, ref=ref, rows=rows, Xc=ref["X"].to(env.dev), compact={})
    return env.cache[key]


def glu_launch(env, case, Xsrc, Tsrc, rows, off, R, out, blocks):
    """flute_qgemm_grouped_glu_blocks, or the row form through flute_qgemm_grouped_glu_ex; returns the code."""
    lay = case.lay
    head = (dtype_id(lay.dtype), lay.bits, lay.g, off.shape[0] - 1, R, Tsrc, lay.F, K, case.Qg.shape[1], case.tid,
            Xsrc.data_ptr(), None if rows is None else rows.data_ptr(), off.data_ptr(), *[t.data_ptr() for t in case.ops()],
            out.out.data_ptr(), env.num_sms, env.stream_ptr(env.dev))
    with torch.cuda.device(env.dev):
        rc = env.lib.flute_qgemm_grouped_glu_blocks(*head) if blocks else env.lib.flute_qgemm_grouped_glu_ex(*head, ROWS)
    torch.cuda.synchronize()
    return rc


def glu_compact(env, c, blocks):
    """The launch on the compact copy (Tsrc = GLU_NSRC): checked against the reference, its bits kept."""
    if blocks not in c["compact"]:
        case, dtype = c["case"], c["case"].lay.dtype
        out = LC.Guarded((GLU_R, GLU_F), dtype, env.dev)
        off = off_tensor(env, LC.served_offsets(GLU_COUNTS))
        env.check(glu_launch(env, case, c["Xc"], GLU_NSRC, c["rows"].int().to(env.dev), off, GLU_R, out, blocks))
        out.assert_guards()
        GC.assert_glu(out.out, c["ref"]["E"], dtype, ("compact", "blocks" if blocks else "rows"))
        c["compact"][blocks] = out.out.clone()
    return c["compact"][blocks]


def source_buffer(env, dtype):
    """[GLU_PAD + R_LONG + GLU_PAD, K] for Xsrc and the rows around it, once per module and type."""
    key = ("xsrc", dtype)
    if key not in env.cache:
        env.cache[key] = LC.nan_filled(GLU_PAD + LC.R_LONG + GLU_PAD, K, dtype, env.dev)
    buf = env.cache[key]
    buf.view(torch.int16).fill_(XC.NAN_BITS[dtype])
    return buf


def glu_variant(env, dtype, Tsrc, blocks, refused=False):
    """Xsrc [Tsrc, K] is NaN but for GLU_NSRC rows (source_rows), and so are the rows around it: a misaddressed read returns
    NaN.  The result is inside assert_glu's bound of the reference on the compact copy, and bit for bit the launch on that copy
    with remapped `rows`: a token does not depend on where its row lies."""
    c = glu_case(env, dtype)
    case = c["case"]
    src = torch.tensor(source_rows(Tsrc, GLU_NSRC, Tsrc), device=env.dev)
    buf = source_buffer(env, dtype)
    Xsrc = buf[GLU_PAD:GLU_PAD + Tsrc]
    Xsrc[src] = c["Xc"]
    rows = src[c["rows"].to(env.dev)].int()
    assert int(rows[-1]) == Tsrc - 1 and int(rows.max()) == Tsrc - 1 and int(rows.min()) >= 0
    off = off_tensor(env, LC.served_offsets(GLU_COUNTS))
    out = LC.Guarded((GLU_R, GLU_F), dtype, env.dev)
    inputs = (buf, rows) + case.ops()
    before = LC.snapshot(*inputs)
    rc = glu_launch(env, case, Xsrc, Tsrc, rows, off, GLU_R, out, blocks)
    if refused:
        assert rc == ERR_SHAPE
        out.assert_untouched()
        with pytest.raises(ValueError):
            case.run(Xsrc, off, rows, blocks=True)
        return
    env.check(rc)
    out.assert_guards()
    out.assert_written()
    LC.assert_unchanged(before, *inputs)
    what = ("glu", "blocks" if blocks else "rows", str(dtype), "Tsrc", Tsrc)
    GC.assert_glu(out.out, c["ref"]["E"], dtype, what)
    LC.assert_equal_bits(out.out, glu_compact(env, c, blocks), what)


def test_glu_blocks_at_the_last_tsrc(env):
    """Tsrc = TSRC_EDGE: the descriptor spans 2^32 - 2048 bytes and the last rows' offsets end just below it."""
    need(40)
    glu_variant(env, F16, LC.TSRC_EDGE, blocks=True)


def test_glu_blocks_at_the_last_tsrc_bf16(env):
    need(40)
    glu_variant(env, BF16, LC.TSRC_EDGE, blocks=True)


def test_glu_blocks_refused_one_row_later(env):
    need(40)
    glu_variant(env, F16, LC.TSRC_EDGE + 1, blocks=True, refused=True)


@pytest.mark.parametrize("Tsrc", [LC.TSRC_EDGE + 1, LC.R_LONG])
def test_glu_row_form_past_the_edge(env, Tsrc):
    """The row form reads Xsrc through 64-bit row bases: one row past the block form's limit, and R_LONG rows."""
    need(40)
    glu_variant(env, F16, Tsrc, blocks=False)


def test_glu_blocks_without_rows(env):
    """rows = None, R = Tsrc = TSRC_EDGE: row r reads Xsrc[r].  One table is a run of served rows (offsets[0] > 0: the rows
    below it and from offsets[E] on are served by no expert, hold NaN and stay unwritten); the run lies across the row that
    straddles 2^31, then at the end of the 2^32 - 2048 bytes."""
    need(40)
    dtype, Tsrc = F16, LC.TSRC_EDGE
    c = glu_case(env, dtype)
    case = c["case"]
    gathered = c["Xc"][c["rows"].to(env.dev)]
    want = glu_compact(env, c, True)
    for base in (LC.ROW_2G - GLU_R // 2, Tsrc - GLU_R):
        buf = source_buffer(env, dtype)
        Xsrc = buf[GLU_PAD:GLU_PAD + Tsrc]
        Xsrc[base:base + GLU_R] = gathered
        off = off_tensor(env, [base + o for o in LC.served_offsets(GLU_COUNTS)])
        out = LC.Guarded((Tsrc, GLU_F), dtype, env.dev)
        inputs = (buf,) + case.ops()
        before = LC.snapshot(*inputs)
        env.check(glu_launch(env, case, Xsrc, Tsrc, None, off, Tsrc, out, True))
        out.assert_guards()
        out.assert_unwritten(0, base)
        out.assert_unwritten(base + GLU_R, Tsrc)
        LC.assert_unchanged(before, *inputs)
        H = out.out[base:base + GLU_R]
        assert not torch.isnan(H).any()
        GC.assert_glu(H, c["ref"]["E"], dtype, ("glu blocks, rows = None", "base", base))
        LC.assert_equal_bits(H, want, ("rows = None", base))
        del out, before


# ---- 5: the grouped scale and table gradients ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def param_grad_case(env):
    """R_LONG rows on the spread table, N = 128.  X is zero but for the bands (first and last 64 rows, around ROW_2G and ROW_4G,
    3000 random rows), dY is dense; both are multiples of 1/4 in [-1/4, 1/4] and the scales +-2^e (grouped_cases.exact_inputs /
    exact_scales), so every sum is exact in fp32 in any order (grouped_cases.exact_premise asserts it per expert) and the
    expected values are the fp64 sums over the non-zero rows."""
    need(40)
    d, bits, N, g, dtype, Rn = env.dev, 4, 128, 64, F16, LC.R_LONG
    counts = LC.spread_counts(Rn)
    off = LC.served_offsets(counts)
    E = len(counts)
    seed = XC.seed_of("long rows param grad") // 2
    lays = GC.exact_layers(bits, 32, g, dtype, K, N, False, E, seed)
    Q, _, t2, tid = GC.stack_exact(env, lays)
    S = torch.stack([GC.exact_scales(N, K // g, dtype, seed + 100 + e) for e in range(E)]).to(d)
    src = LC.bands(Rn, 3000, seed)
    X = torch.zeros(Rn, K, dtype=dtype, device=d)
    X[torch.tensor(src, device=d)] = LC.device_ints(len(src), K, seed + 1, dtype, amp=1, div=4)
    dY = LC.device_ints(Rn, N, seed + 2, dtype, amp=1, div=4)
    dT2 = torch.zeros(E, 4 ** bits, 2, dtype=torch.float64, device=d)
    dS = torch.zeros(E, N, K // g, dtype=torch.float64, device=d)
    for e, lay in enumerate(lays):
        sel = [r for r in src if off[e] <= r < off[e + 1]]
        if sel:
            idx = torch.tensor(sel, device=d)
            codes = lay.W.to(d)
            dT2[e], dS[e] = GC.exact_premise(X[idx], dY[idx], S[e], codes, SR.lut_of_codes(codes, lay.pairs, bits), bits, g, dtype)
    assert not dS[1].any() and all(bool(dS[e].any()) for e in (0, 2, 4, 5, 6, 7))      # (expert 1 has no rows)
    c = dict(bits=bits, N=N, g=g, dtype=dtype, R=Rn, E=E, off=off_tensor(env, off), Q=Q, S=S, t2=t2, tid=tid, X=X, dY=dY,
             dT2=dT2, dS=dS)
    c["before"] = LC.snapshot(X, dY, Q, S, t2)
    yield c
    c.clear()


def param_grad_head(c):
    return (dtype_id(c["dtype"]), c["bits"], c["g"], c["E"], c["R"], c["N"], K, c["Q"].shape[1], c["tid"], c["dY"].data_ptr(),
            c["X"].data_ptr(), c["off"].data_ptr(), c["Q"].data_ptr())


def test_grouped_scale_grad_past_2_31_elements(env, param_grad_case):
    c = param_grad_case
    out = LC.Guarded((c["E"], c["N"], K // c["g"]), c["dtype"], env.dev)
    with torch.cuda.device(env.dev):
        rc = env.lib.flute_qgemm_grouped_scale_grad(*param_grad_head(c), c["t2"].data_ptr(), None, out.out.data_ptr(),
                                                    env.num_sms, env.stream_ptr(env.dev))
    env.check(rc)
    torch.cuda.synchronize()
    out.assert_guards()
    assert not torch.isnan(out.out).any()
    LC.assert_unchanged(c["before"], c["X"], c["dY"], c["Q"], c["S"], c["t2"])
    assert XC.exact_equal(out.out, c["dS"], c["dtype"])


def test_grouped_table_grad_past_2_31_elements(env, param_grad_case):
    c = param_grad_case
    n = 2 ** c["bits"]
    nbytes = env.lib.flute_qgemm_grouped_table_grad_scratch_bytes(c["bits"], c["g"], c["E"], c["N"], K)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=env.dev)
    dT2 = LC.Guarded((c["E"], n, n, 2), torch.float32, env.dev)
    dS = LC.Guarded((c["E"], c["N"], K // c["g"]), c["dtype"], env.dev)
    with torch.cuda.device(env.dev):
        rc = env.lib.flute_qgemm_grouped_table_grad(*param_grad_head(c), c["S"].data_ptr(), c["t2"].data_ptr(), None,
                                                    dT2.out.data_ptr(), dS.out.data_ptr(), scratch.data_ptr(), nbytes,
                                                    env.num_sms, env.stream_ptr(env.dev))
    env.check(rc)
    torch.cuda.synchronize()
    dT2.assert_guards()
    dS.assert_guards()
    assert not torch.isnan(dT2.out).any() and not torch.isnan(dS.out).any()
    LC.assert_unchanged(c["before"], c["X"], c["dY"], c["Q"], c["S"], c["t2"])
    assert torch.equal(dT2.out.double().reshape(c["E"], -1, 2), c["dT2"])
    assert XC.exact_equal(dS.out, c["dS"], c["dtype"])
