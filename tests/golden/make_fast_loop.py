"""Store the lean decode kernel's outputs on tests/fast_loop_cases.py's seeded launches (needs a GPU):

    python tests/golden/make_fast_loop.py [out.npz]

Writes tests/golden/fast_loop/fast_loop.npz: one int16 array (the output's bits) per case.  It also reports, per case, whether
the round-4 one-shot kernel (override one_shot = 0) returns the same bits."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import flute_amd  # noqa: E402
from flute_amd import dev, utils  # noqa: E402
from oracle import flute_oracle as O  # noqa: E402
from tests import fast_loop_cases as C  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fast_loop", "fast_loop.npz")
device = torch.device("cuda:0")
num_sms = utils.get_device_num_sms(device)
ws = utils.get_workspace_streamk(device)
arrays = {}
same_as_oneshot = 0
for case in C.cases():
    out = C.run(flute_amd, dev, utils, O, case, num_sms, ws, device)
    again = C.run(flute_amd, dev, utils, O, case, num_sms, ws, device)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), case[0]
    one = C.run(flute_amd, dev, utils, O, case, num_sms, ws, device, ovr=dev.Overrides(family=0, one_shot=0))
    eq = bool(torch.equal(out.view(torch.int16), one.view(torch.int16)))
    same_as_oneshot += eq
    print(json.dumps({"case": case[0], "equal_to_one_shot_0": eq}), flush=True)
    arrays[case[0]] = out.view(torch.int16).numpy()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
np.savez_compressed(out_path, **arrays)
print(json.dumps({"cases": len(arrays), "equal_to_one_shot_0": same_as_oneshot, "out": out_path}), flush=True)
