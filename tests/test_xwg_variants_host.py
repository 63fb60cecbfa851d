"""The give-up variants of the library (csrc/Makefile: SPIN_UNITS, libflute_amd_spin0.so / _spin1.so), kept honest without a
GPU: the build made them, they are the shipped ABI, and the units they recompile are exactly the instantiation units whose
kernel header takes xwg.h's E form - the only place a poll bound is compiled in.  tests/test_xwg_giveup_gpu.py runs them."""
import ctypes
import glob
import os
import re

import pytest

from flute_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
VARIANTS = ("spin0", "spin1")
# a call of the bounded poll, or of the seam function that contains one (with or without explicit template arguments)
BOUNDED_POLL = re.compile(r"\bxwg_wait_all\s*\(|\bxwg_seam\s*(<[^;{}()]*>)?\s*\(")


def variant_path(tag):
    return os.path.join(CSRC, "libflute_amd_%s.so" % tag)


def makefile_list(name):
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    found = re.findall(r"^%s\s*=(.*)$" % name, text, re.M)
    assert len(found) == 1, (name, found)             # the list is kept in ONE variable
    return found[0].split()


def code_of(path):
    """The file without its // comments."""
    return re.sub(r"//[^\n]*", "", open(path).read())


def units_with_a_bounded_poll():
    units = set()
    for path in glob.glob(os.path.join(CSRC, "inst_*.hip")):
        headers = re.findall(r'^#include "([^"]+)"', open(path).read(), re.M)
        if any(BOUNDED_POLL.search(code_of(os.path.join(CSRC, h))) for h in headers):
            units.add(os.path.basename(path)[:-4])
    return units


@pytest.mark.parametrize("tag", VARIANTS)
def test_variant_is_the_shipped_abi(tag):
    path = variant_path(tag)
    assert os.path.exists(path), "%s is missing: `make -C flute_amd/csrc` builds it with the library" % path
    lib = ctypes.CDLL(path)
    missing = [name for name in _lib.SYMBOLS if not hasattr(lib, name)]
    assert not missing, (tag, missing)
    lib.flute_abi_version.restype = ctypes.c_int
    assert lib.flute_abi_version() == _lib.get().flute_abi_version()


def test_variant_units_are_the_units_with_a_bounded_poll():
    listed = makefile_list("SPIN_UNITS")
    assert len(listed) == len(set(listed))
    assert set(listed) == units_with_a_bounded_poll(), "a kernel that takes the E form of xwg.h joins SPIN_UNITS"
    assert set(listed) <= {s[:-4] for s in makefile_list("SRCS")}
    assert makefile_list("SPIN_LIMITS") == ["0", "1"]


def test_the_poll_rule_sees_what_it_must():
    """The rule finds the two spellings in the tree and the function's definition, and not the kernels that only arrive."""
    assert BOUNDED_POLL.search(code_of(os.path.join(CSRC, "qgemm_splitk.h"))).group(0).startswith("xwg_wait_all")
    assert BOUNDED_POLL.search(code_of(os.path.join(CSRC, "qgemm_block3.h"))).group(0).startswith("xwg_seam<")
    assert BOUNDED_POLL.search(code_of(os.path.join(CSRC, "xwg.h")))
    for h in ("qgemm_skinny.h", "qgemm_tile.h"):
        text = code_of(os.path.join(CSRC, h))
        assert "xwg_arrive(" in text and not BOUNDED_POLL.search(text), h
