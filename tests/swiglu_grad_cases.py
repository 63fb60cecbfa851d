"""What the host and the GPU tests of flute_amd.swiglu_grad share: the header's error account read from the header - the constant
`c` stands in one place, include/flute_amd.h - the formula in fp64, the two bounds, and the random draw whose reference alone
keeps the bounds from being vacuous.  Importable without a GPU."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = torch.float16, torch.bfloat16
UNIT_ROUNDOFF = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
EPS_S = 2.0 ** -21                                  # silu32.h's constant, which the header's du bound names


def header_text():
    return open(os.path.join(ROOT, "include", "flute_amd.h")).read()


def header_account():
    """The comment at flute_swiglu_grad, up to its declaration."""
    hdr = header_text()
    end = hdr.index("int flute_swiglu_grad(")
    return hdr[hdr.rindex("/*", 0, end):end]


def header_c():
    """The constant of the dg bound as the header states it: `... + c * 2^-23 * (1 + |g|) * |dh * u|,  c = <integer>`."""
    m = re.search(r"c \* 2\^-23 \* \(1 \+ \|g\|\) \* \|dh \* u\|,\s+c = (\d+)\.", header_account())
    assert m, "include/flute_amd.h no longer states the dg bound and its constant"
    return int(m.group(1))


def formula64(g, u, dh):
    """(dg, du) of the header's formula in fp64 on the 16-bit inputs."""
    g, u, dh = g.double(), u.double(), dh.double()
    d = 1 + torch.exp(-g)
    sig = 1 / d
    return dh * u * (sig * (1 + g * (1 - sig))), dh * (g / d)


def bounds(g, u, dh, dtype, c):
    """(ref dg, ref du, bound dg, bound du, vacuous dg, vacuous du): the header's bounds in fp64; an element whose reference is
    subnormal in T (or zero) is outside the account, which is relative to a result normal in T."""
    rdg, rdu = formula64(g, u, dh)
    uT, tiny = UNIT_ROUNDOFF[dtype], torch.finfo(dtype).tiny
    bdg = uT * rdg.abs() + c * 2.0 ** -23 * (1 + g.double().abs()) * (dh.double() * u.double()).abs()
    bdu = (uT + EPS_S) * rdu.abs()
    return rdg, rdu, bdg, bdu, rdg.abs() < tiny, rdu.abs() < tiny


def draw(R, F, dtype, seed):
    """g uniform in [-8, 8], u and dh standard normal, rounded to T: of 10^5 elements fewer than 1 % have a reference that is
    subnormal in fp16 (|dh silu(g)| < 6.1e-5 needs a tiny dh or a g next to 0), none in bf16."""
    gen = torch.Generator().manual_seed(seed)
    g = ((torch.rand(R, F, generator=gen) * 16) - 8).to(dtype)
    u = torch.randn(R, F, generator=gen).to(dtype)
    dh = torch.randn(R, F, generator=gen).to(dtype)
    return g, u, dh


def torch_chain(g, u, dh):
    """The default backward's lines (flute_amd/ops.py, `_grouped_glu_backward`, native=False) on g, u, dh in T."""
    dtype = g.dtype
    g, u, dh = g.float(), u.float(), dh.float()
    sig = torch.sigmoid(g)
    return (dh * u * sig * (1 + g * (1 - sig))).to(dtype), (dh * (g * sig)).to(dtype)
