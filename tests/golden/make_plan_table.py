"""Regenerate tests/golden/plans/plan_table.npz: what the planner answers over a fixed set of calls.

    python tests/golden/make_plan_table.py

The fixture pins every plan, return code and fused-rotation flag of the library that was built when it was made;
tests/test_plan_table.py replays the same calls and compares.  A pull request that changes the planner on purpose
regenerates the fixture in the same commit, so that its diff shows which plans moved; a refactor leaves it alone.

Stored (outputs only): per flute_qgemm_plan_ex call its rc and the 18 flute_plan fields (zeros where rc != 0), one array
per column (`plan_rc`, `plan_family`, ... in _lib.Plan order), each in the narrowest signed integer type that holds it
exactly - column by column the file compresses to a third of the row-major int32 table; `load_plans` widens them back to
int32 rows.  `fused`: one flute_qgemm_hadamard_fused result per call.  And the SHA-256 of each enumerated input table, so
that a change to the enumeration fails as such and not as a wall of plan mismatches.  The fixture lives in a folder of its
own: tests/conftest.py treats every tests/golden/*.npz as a kernel fixture.

The inputs (`plan_inputs`, `fused_inputs`) are the union of
  1. a seeded sweep of 50 000 calls: bits 2 / 3 / 4 with every legal template id (the automatic ids more often), group 32 .. 256,
     M 1 .. 4096 with the bucket edges, N x K from the model layers, 8 .. 304 CUs, workspaces 0 .. 256 MB, both dtypes;
     about a third of the calls with random overrides of every field (unfit ones too: their error codes are pinned),
     a few with bad arguments;
  2. targeted rows for kernels a uniform sweep rarely reaches (the lean decode kernel, the MFMA decode kernels);
  3. every key of flute_amd/data/gfx950_tuned.json with its stored id (the plans the product and bench.py use);
  4. flute_qgemm_hadamard_fused for M <= 4 over a small grid (the only way the ABI reaches the fused-rotation planning).
"""
import hashlib
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from flute_amd import _lib  # noqa: E402

TABLE_PATH = os.path.join(HERE, "plans", "plan_table.npz")
TUNED_PATH = os.path.join(ROOT, "flute_amd", "data", "gfx950_tuned.json")

OVR_FIELDS = [n for n, _ in _lib.Overrides._fields_]
PLAN_FIELDS = [n for n, _ in _lib.Plan._fields_]
# plan_inputs columns: the plan call's arguments, then whether overrides are passed, then the override fields
PLAN_COLUMNS = ["dtype", "bits", "group", "M", "N", "K", "template_id", "num_sms", "workspace", "has_ovr"] + OVR_FIELDS
FUSED_COLUMNS = ["dtype", "bits", "group", "hadamard", "M", "N", "K", "template_id", "num_sms", "workspace"]

MB = 1 << 20
M_EDGES = [1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 48, 64, 65, 96, 127, 128, 129, 160, 192, 255, 256, 257, 320, 384, 511, 512,
           768, 1000, 1024, 2048, 4096]
N_MULTS = [1, 2, 3, 4, 7, 8, 11, 14, 16, 21, 28, 32, 43, 56, 64, 112, 224]
KS = [256, 512, 1024, 2048, 3584, 4096, 4160, 5120, 6144, 8192, 11008, 12288, 14336, 16384, 28672]
LAYERS = [(4096, 4096), (4096, 11008), (11008, 4096), (4096, 14336), (14336, 4096), (3584, 14336), (14336, 3584),
          (8192, 8192), (8192, 28672), (28672, 8192), (10240, 8192), (6144, 4096), (2048, 4096), (4096, 2048),
          (8192, 2048), (3584, 8192), (12288, 4096), (4096, 16384)]
NUM_SMS = [256, 256, 256, 8, 80, 120, 304]
WORKSPACES = [64 * MB, 64 * MB, 0, 1 * MB, 256 * MB]
OVR_CHOICES = {
    "family": [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -2],
    "m_block": [0, 1, 2, 3, 4, 8, 9, 12],
    "waves": [0, 1, 2, 4, 6, 8, 12, 16],
    "kw": [0, 1, 2, 3, 4, 8],
    "splitk": [0, 1, 2, 3, 4, 8, 16, 32],
    "m_tiles": [0, 1, 2, 3, 4, 8],
    "slabs_per_wave": [0, 1, 2, 3, 4],
    "ring_depth": [0, 2, 3, 4, 8],
    "one_shot": [0, 1, 2, 3, 4, 5],
}
AUTO_IDS = {4: [0, 4, 16, 20], 2: [0, 4, 8], 3: [4, 8, 5]}       # QuantMapMode digit 0 (4 bits), SMs_Multiple 1, Stages 2 / 3


def _tile_p(lib, bits, tid):
    info = _lib.TemplateInfo()
    return info.tile_p if lib.flute_get_template_info(bits, tid, info) == 0 else 32


def _legal_ids(lib, bits):
    return [t for t in range(lib.flute_num_templates(bits)) if bits != 3 or _tile_p(lib, 3, t) == 32]


def _row(dtype, bits, g, M, N, K, tid, num_sms, ws, ovr=None):
    return [dtype, bits, g, M, N, K, tid, num_sms, ws] + ([0] + [-1] * len(OVR_FIELDS) if ovr is None else [1] + ovr)


def _sweep(lib, rng, calls):
    ids = {b: _legal_ids(lib, b) for b in (2, 3, 4)}
    rows = []
    while len(rows) < calls:
        bits = rng.choice([4, 4, 2, 3])
        tid = rng.choice(AUTO_IDS[bits]) if rng.random() < 0.4 else rng.choice(ids[bits])
        g = rng.choice([32, 64, 64, 128, 128, 256])
        J = 16 if bits == 3 else 16 // bits
        if rng.random() < 0.5:
            N, K = rng.choice(LAYERS)
        else:
            N, K = J * _tile_p(lib, bits, tid) * rng.choice(N_MULTS), rng.choice(KS)
        M = rng.choice(M_EDGES) if rng.random() < 0.5 else max(1, min(4096, int(2 ** rng.uniform(0, 12))))
        dtype = rng.choice([0, 1])
        num_sms = rng.choice(NUM_SMS)
        ws = rng.choice(WORKSPACES)
        ovr = None
        if rng.random() < 1 / 3:
            ovr = [rng.choice(OVR_CHOICES[f]) if rng.random() < 0.35 else -1 for f in OVR_FIELDS]
            if rng.random() < 0.6:
                ovr[0] = rng.choice(OVR_CHOICES["family"])
        if rng.random() < 0.02:                       # bad arguments: the order of the error codes is pinned too
            what = rng.randrange(6)
            if what == 0: dtype = rng.choice([2, -1])
            elif what == 1: bits = rng.choice([1, 5, 8])
            elif what == 2: g = rng.choice([16, 48, 512])
            elif what == 3: tid = rng.choice([-1, 36, 144, 999])
            elif what == 4: N += 16
            else: M = rng.choice([0, -1])
        rows.append(_row(dtype, bits, g, M, N, K, tid, num_sms, ws, ovr))
    return rows


def _targeted():
    """Kernels a uniform sweep rarely reaches: the lean decode kernel (one_shot 4), the lean and persistent MFMA decode
    kernels (families 7, 8), the persistent one-shot kernel, the forced 3-bit block configurations."""
    rows = []
    for dtype in (0, 1):
        for tid in AUTO_IDS[4]:
            for K in (2048, 3584, 4096, 8192):
                for N in (1024, 2048, 4096, 5120, 8192, 11008 // 64 * 64, 14336, 16384, 28672):
                    for M in range(1, 17):
                        for num_sms in (256, 304, 120):
                            rows.append(_row(dtype, 4, 128 if K == 8192 else 64, M, N, K, tid, num_sms, 64 * MB))
        for bits in (2, 3, 4):
            for N, K in LAYERS:
                for M in (1, 2, 3, 4, 8, 16, 33, 48, 64, 96):
                    rows.append(_row(dtype, bits, 64, M, N, K, AUTO_IDS[bits][0], 256, 64 * MB))
        for N, K in LAYERS:                           # forced 3-bit blocks: skinny (m_block 1 / 2 / 4), 128 and 256 rows
            for M in (16, 48, 64, 200):
                for m_block, m_tiles in ((1, -1), (2, -1), (4, -1), (-1, 4), (-1, 8)):
                    ovr = [-1] * len(OVR_FIELDS)
                    ovr[0], ovr[OVR_FIELDS.index("m_block")], ovr[OVR_FIELDS.index("m_tiles")] = 3, m_block, m_tiles
                    rows.append(_row(dtype, 3, 64, M, N, K, AUTO_IDS[3][0], 256, 64 * MB, ovr))
    return rows


def _tuned():
    d = json.load(open(TUNED_PATH))
    ws = 64 * MB                                      # flute_amd.utils.make_workspace_streamk
    rows = []
    for key, tid in sorted(d["entries"].items()):
        m, N, K, bits, g, num_sms, dt, _ = key.split("|")
        rows.append(_row(0 if dt == "float16" else 1, int(bits), int(g), int(m), int(N), int(K), int(tid), int(num_sms), ws))
    return rows


def plan_inputs(lib=None):
    lib = lib or _lib.get()
    rng = random.Random(20261015)
    return np.array(_sweep(lib, rng, 50000) + _targeted() + _tuned(), dtype=np.int64)


def fused_inputs():
    rows = []
    for dtype in (0, 1):
        for bits in (2, 3, 4):
            for tid in AUTO_IDS[bits][:2] + [35 if bits != 4 else 143]:
                for g in (64, 128):
                    for h in (16, 64, 512, 1024):
                        for M in (1, 2, 3, 4):
                            for N, K in ((4096, 4096), (4096, 3584), (14336, 4096), (4096, 14336), (2048, 2048), (28672, 8192)):
                                rows.append([dtype, bits, g, h, M, N, K, tid, 256, 64 * MB])
    return np.array(rows, dtype=np.int64)


def digest(inputs):
    return hashlib.sha256(np.ascontiguousarray(inputs, dtype="<i8").tobytes()).hexdigest()


def run_plans(inputs, lib=None):
    lib = lib or _lib.get()
    out = np.zeros((len(inputs), 1 + len(PLAN_FIELDS)), dtype=np.int32)
    for i, r in enumerate(inputs.tolist()):
        p = _lib.Plan()
        ovr = _lib.Overrides(*r[10:]) if r[9] else None
        rc = lib.flute_qgemm_plan_ex(*r[:9], ovr, p)
        out[i, 0] = rc
        if rc == 0:
            out[i, 1:] = [getattr(p, f) for f in PLAN_FIELDS]
    return out


def run_fused(inputs, lib=None):
    lib = lib or _lib.get()
    return np.array([lib.flute_qgemm_hadamard_fused(*r) for r in inputs.tolist()], dtype=np.int32)


def _narrowest(col):
    for dt in (np.int8, np.int16, np.int32):
        if np.iinfo(dt).min <= col.min() and col.max() <= np.iinfo(dt).max:
            return col.astype(dt)
    raise ValueError("a plan field outside int32")


def load_plans(z):
    """The stored plan table as int32 rows: rc, then the 18 flute_plan fields."""
    return np.stack([z["plan_" + f].astype(np.int32) for f in ["rc"] + PLAN_FIELDS], axis=1)


def main():
    pin, fin = plan_inputs(), fused_inputs()
    plans, fused = run_plans(pin), run_fused(fin)
    os.makedirs(os.path.dirname(TABLE_PATH), exist_ok=True)
    cols = {"plan_" + f: _narrowest(plans[:, i]) for i, f in enumerate(["rc"] + PLAN_FIELDS)}
    np.savez_compressed(TABLE_PATH, **cols, fused=fused.astype(np.int8),
                        plan_inputs_sha256=np.array(digest(pin)), fused_inputs_sha256=np.array(digest(fin)))
    print(f"{TABLE_PATH}: {len(plans)} plans ({int((plans[:, 0] == 0).sum())} ok), {len(fused)} fused flags "
          f"({int(fused.sum())} fused), {os.path.getsize(TABLE_PATH)} bytes")


if __name__ == "__main__":
    main()
