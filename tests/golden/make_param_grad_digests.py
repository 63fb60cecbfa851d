"""Record the bits of the parameter-gradient ops (qgemm_scale_grad, qgemm_table_grad and their grouped forms) as one
SHA-256 per case, on an MI355X:

    python tests/golden/make_param_grad_digests.py --commit <hash of the checkout>

Run it on a built checkout of the commit whose bits are to be kept - the parent of a change to these kernels, never the
tree under test - with this file copied in.  It writes tests/golden/param_grad/parent_digests.json: the commit, the hipcc
version and {case id: digest over the raw bytes of every output of the call}.  tests/test_param_grad_parent_bits_gpu.py
recomputes every case with `digests()` below and compares.

The inputs are general values (numpy RandomState randn with fixed seeds, rounded to T): a changed summation order changes
bits.  The cases are the smallest at which each path of the kernels runs: all ten layouts; group size 32 at N = 256,
K = 320 (two n blocks, a second k block that is partial) and group size 256 at N = 128, K = 256 (one group per block,
eight chunks per group), N raised to the layout's packing unit (16 / b) * TileP - 512 at 3 bits - where that is larger,
since no smaller layer of the layout exists; dense at M = 1, M = 33 (two steps, the last ragged, no split) and M = 257
with num_sms = 256 (M split in two: both partial reduces run); grouped over offsets [0, 0, 33, 34, 70] in R = 80 rows (an
empty first expert, experts of 33, 1 and 36 rows, ten rows no expert serves), with and without a row weight; each as
scale only, table only and table with scale."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "param_grad", "parent_digests.json")

LAYOUTS = [(4, 32), (4, 64), (2, 32), (2, 64), (3, 32)]
SHAPES = [(32, 256, 320), (256, 128, 256)]           # (group size, N at least, K)
DENSE_M = [(1, None), (33, None), (257, 256)]        # (M, num_sms)
E, R, OFFSETS = 4, 80, [0, 0, 33, 34, 70]
FORMS = ("scale", "table", "table+scale")


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def digests(fa, dev):
    """{case id: sha256} of every case, computed with the package `fa` on `dev`."""
    from flute_amd import utils
    num_sms = utils.get_device_num_sms(dev)
    out = {}
    for dtype, dname in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for bits, tile_p in LAYOUTS:
            tid = min(t for (b, t), c in fa.TEMPLATE_CONFIGS.items() if b == bits and c["TileP"] == tile_p)
            for g, N, K in SHAPES:
                N = max(N, 512 if bits == 3 else (16 // bits) * tile_p)
                rs = np.random.RandomState(1000 * bits + 10 * tile_p + g + (dtype == torch.bfloat16))
                n = 2 ** bits
                T = lambda a: torch.from_numpy(a).to(dtype).to(dev)
                W = torch.from_numpy(rs.randint(0, n, (E, K, N)).astype(np.uint8)).to(dev)
                Q = torch.stack([utils.pack(W[e], bits, [tid], num_sms) for e in range(E)])
                S = T(rs.randn(E, N, K // g) / 8)
                t2 = torch.stack([utils.make_qmap2_from_qmap(torch.from_numpy(np.sort(rs.randn(n))).to(dtype))
                                  for _ in range(E)]).to(dev)
                dY, X = T(rs.randn(257, N)), T(rs.randn(257, K))
                rw = torch.from_numpy((rs.rand(R) * 1.5 + 0.25).astype(np.float32)).to(dev)
                off = torch.tensor(OFFSETS, dtype=torch.int32, device=dev)
                name = "%s-b%d-tp%d-g%d" % (dname, bits, tile_p, g)

                def run(form, scale_fn, table_fn):
                    if form == "scale":
                        return (scale_fn(),)
                    if form == "table":
                        return (table_fn({}),)
                    return table_fn(dict(with_scale_grad=True))

                for M, sms in DENSE_M:
                    y, x = dY[:M], X[:M]
                    for form in FORMS:
                        res = run(form, lambda: fa.qgemm_scale_grad(y, x, Q[1], t2[1], bits, g, tid, sms),
                                  lambda kw: fa.qgemm_table_grad(y, x, Q[1], S[1], bits, g, tid, sms, table2=t2[1], **kw))
                        out["%s-dense-M%d-%s" % (name, M, form)] = sha(*res)
                for weighted in (False, True):
                    kw_w = dict(row_weight=rw) if weighted else {}
                    y, x = dY[:R], X[:R]
                    for form in FORMS:
                        res = run(form, lambda: fa.qgemm_grouped_scale_grad(y, x, off, Q, t2, bits, g, tid, **kw_w),
                                  lambda kw: fa.qgemm_grouped_table_grad(y, x, off, Q, S, bits, g, tid, table2=t2, **kw_w,
                                                                         **kw))
                        out["%s-grouped-%s-%s" % (name, "weighted" if weighted else "plain", form)] = sha(*res)
    torch.cuda.synchronize()
    return out


def hipcc_version():
    try:
        text = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, check=True).stdout
        return next(line.strip() for line in text.splitlines() if "HIP version" in line)
    except (OSError, subprocess.CalledProcessError, StopIteration):
        return "HIP version: %s (torch.version.hip)" % torch.version.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the hash of the checkout this runs on")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import flute_amd
    d = digests(flute_amd, torch.device("cuda:0"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "hipcc": hipcc_version(), "digests": d}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d digests to %s" % (len(d), args.out))


if __name__ == "__main__":
    main()
