"""The parameter-gradient ops return, bit for bit, what the commit named in tests/golden/param_grad/parent_digests.json
returned: every case of tests/golden/make_param_grad_digests.py (all ten layouts, both block shapes, the dense forms
unsplit and split, the grouped forms with an empty expert and with and without a row weight) is recomputed and its
SHA-256 over the raw bytes of every output compared with the recorded one.

The digests pin the compiler as well as the source: after a compiler change, regenerate the file at the UNCHANGED commit
it names (the maker's docstring says how) before reading a mismatch as a changed kernel.  That repeated calls give equal
bits is asserted by the ops' own test_reproducible / test_equal_bits_* tests."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAKER = os.path.join(HERE, "golden", "make_param_grad_digests.py")


def test_bits_equal_the_recorded_commit():
    spec = importlib.util.spec_from_file_location("make_param_grad_digests", MAKER)
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with open(maker.OUT) as f:
        recorded = json.load(f)
    import flute_amd
    got = maker.digests(flute_amd, torch.device("cuda:0"))
    want = recorded["digests"]
    assert len(want) == 300 and sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    print("recorded at commit %s with %s; %d of %d cases differ" % (recorded["commit"], recorded["hipcc"], len(differ), len(want)))
    assert not differ, differ
