"""The lean decode kernel (qgemm_fast.h) returns the stored bits on every instantiated shape.

tests/golden/fast_loop/fast_loop.npz holds the kernel's outputs on tests/fast_loop_cases.py's seeded inputs, as computed by the
library before its decode loop was rewritten to keep several lookup groups in flight (round 5's loop: one group in flight).
The rewrite keeps the arithmetic and its order, so every output must be bit-identical: both dtypes, TileP 32 / 64, one / two /
four rows per pass, 4 / 7 / 8 pieces per wave, the K split across two waves and group sizes 64 / 128 / 256."""
import os

import numpy as np
import pytest
import torch

from tests import fast_loop_cases as C

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast_loop", "fast_loop.npz")


def test_fixture_covers_every_case_and_every_case_plans_the_lean_kernel():
    import flute_amd
    from flute_amd import dev
    z = np.load(FIXTURE)
    assert sorted(z.files) == sorted(c[0] for c in C.cases())
    for (name, dtype, tile_p, w, kw, d, mb, M, K, g, seed) in C.cases():
        assert z[name].shape == (M, C.N) and z[name].dtype == np.int16, name
        plan = dev.get_plan(M, C.N, K, 4, g, C.template_id(flute_amd, tile_p), 256, dtype, C.overrides(dev, w))
        assert (plan["family"], plan["one_shot"], plan["waves"], plan["kw"], plan["ring_depth"], plan["m_block"]) == (0, 4, w, kw, d, mb), (name, plan)


@pytest.mark.gpu
def test_lean_kernel_bits_match_fixture():
    import flute_amd
    from flute_amd import dev, utils
    from oracle import flute_oracle as O

    device = torch.device("cuda:0")
    num_sms = utils.get_device_num_sms(device)
    ws = utils.get_workspace_streamk(device)
    z = np.load(FIXTURE)
    bad = []
    for case in C.cases():
        out = C.run(flute_amd, dev, utils, O, case, num_sms, ws, device)
        want = z[case[0]]
        got = out.view(torch.int16).numpy()
        assert got.shape == want.shape, case[0]
        if not np.array_equal(got, want):
            bad.append((case[0], int((got != want).sum())))
    assert not bad, bad
