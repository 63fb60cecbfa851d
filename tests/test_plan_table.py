"""Every plan the planner hands out over a fixed set of ~75k calls matches the committed fixture
(tests/golden/plans/plan_table.npz, written by tests/golden/make_plan_table.py): return codes always, all 18 plan fields
where the call succeeds, and the fused-rotation flag of flute_qgemm_hadamard_fused.  No GPU."""
import importlib.util
import os

import numpy as np

from flute_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_table", os.path.join(HERE, "golden", "make_plan_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

# (family, one_shot) pairs test_abi.test_plan_invariants_over_random_shapes lists: each must be pinned by many rows
KERNELS = ((0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (2, 0), (3, 0), (5, 0), (6, 0), (7, 0), (8, 0), (8, 1))


def _mismatches(inputs, columns, want, got, fields):
    bad = np.nonzero((want != got).any(axis=1))[0]
    lines = []
    for i in bad[:20]:
        args = ", ".join(f"{c}={v}" for c, v in zip(columns, inputs[i].tolist()) if not (c in T.OVR_FIELDS and v == -1))
        diff = ", ".join(f"{f}: {a} -> {b}" for f, a, b in zip(fields, want[i].tolist(), got[i].tolist()) if a != b)
        lines.append(f"  row {i} ({args}): {diff}")
    return len(bad), "\n".join(lines)


def test_plan_table_matches_fixture():
    z = np.load(T.TABLE_PATH)
    lib = _lib.get()
    pin = T.plan_inputs(lib)
    assert T.digest(pin) == str(z["plan_inputs_sha256"]), \
        "the enumeration of plan inputs changed: regenerate the fixture with tests/golden/make_plan_table.py"
    want = T.load_plans(z)
    assert want.shape == (len(pin), 1 + len(T.PLAN_FIELDS))
    got = T.run_plans(pin, lib)
    n, detail = _mismatches(pin, T.PLAN_COLUMNS, want, got, ["rc"] + T.PLAN_FIELDS)
    assert n == 0, f"{n} of {len(pin)} plans differ from the fixture (first 20):\n{detail}"

    # coverage: every kernel is pinned by many rows, every override family (0 .. 8) is asked for
    ok = want[:, 0] == 0
    fam, one = want[ok, 1], want[ok, 1 + T.PLAN_FIELDS.index("one_shot")]
    for f, o in KERNELS:
        assert int(((fam == f) & (one == o)).sum()) >= 50, (f, o)
    ovr_family = pin[pin[:, T.PLAN_COLUMNS.index("has_ovr")] == 1, T.PLAN_COLUMNS.index("family")]
    assert set(range(9)) <= set(ovr_family.tolist())


def test_hadamard_fused_table_matches_fixture():
    z = np.load(T.TABLE_PATH)
    lib = _lib.get()
    fin = T.fused_inputs()
    assert T.digest(fin) == str(z["fused_inputs_sha256"]), \
        "the enumeration of fused-rotation inputs changed: regenerate the fixture with tests/golden/make_plan_table.py"
    want = z["fused"].astype(np.int32)[:, None]
    got = T.run_fused(fin, lib)[:, None]
    n, detail = _mismatches(fin, T.FUSED_COLUMNS, want, got, ["fused"])
    assert n == 0, f"{n} of {len(fin)} fused flags differ from the fixture (first 20):\n{detail}"
    assert 0 < int(want.sum()) < len(fin)
