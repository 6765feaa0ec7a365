"""Measure the connected-component labelling (t2map.components) on one MI355X, in one process:

    python tools/components_bench.py [--out profiles/r24_components_bench.json] [--quick]

256^3 voxels (--quick: 64 x 256 x 256), three inputs: the benchmark's brain mask (one large component), that mask plus 1 %
salt noise outside it (many specks), and random foreground at p = 0.31, near the 6-neighbour percolation threshold (the
hardest case for merging).  For each, at connectivity 1, the public calls of t2map.components on device tensors: `label`
(the workspace and output allocation, seven launches and the host's wait for the count), `stats` (three tables), `lut`
(largest, renumbered; waits for the number kept) and `select` (the sizes alone, the table, t2fit_relabel_dev).  HIP events
are recorded around each Python call, the median of 5 after a warm-up: a figure is the time on the stream between the two
events, host gaps included; the kernels are not timed apart.  Beside them: scipy.ndimage.label on the host for the same
input, the HBM time of reading the uint8 input and writing the int32 labels once at 8 TB/s, and a fill_holes call on the
brain mask of the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REPEATS = 5
HBM_BYTES_PER_S = 8.0e12


def median_ms(fn):
    import torch

    fn()  # warm-up
    times = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no_scipy", action="store_true", help="skip the host labelling")
    args = ap.parse_args()

    import torch

    import fetal_t2mapping_amd as t2
    from fetal_t2mapping_amd import synth

    cc = t2.components
    dev = torch.device("cuda", 0)
    shape = (64, 256, 256) if args.quick else (256, 256, 256)
    n_vox = int(np.prod(shape))
    _, mask, _ = synth.brain_volume_torch(shape, 2, seed=synth.SEED_BASE, device=dev)
    brain = (mask.reshape(shape) != 0).to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(24)
    salt = ((torch.rand(shape, generator=g, device=dev) < 0.01) | (brain != 0)).to(torch.uint8)
    random = (torch.rand(shape, generator=g, device=dev) < 0.31).to(torch.uint8)
    rec = {"repeats": REPEATS, "statistic": "median", "device": torch.cuda.get_device_name(dev), "shape": list(shape), "connectivity": 1,
           "tile": list(cc.TILE), "hbm_bytes_per_s": HBM_BYTES_PER_S, "hbm_ms": 5.0 * n_vox / HBM_BYTES_PER_S * 1e3, "inputs": []}
    for name, vol in (("brain mask", brain), ("brain mask + 1 % salt", salt), ("random p = 0.31", random)):
        lab, n = cc.label(vol)
        sizes = cc.stats(lab, n)[0]

        row = {"input": name, "foreground": float(vol.float().mean()), "components": n,
               "largest": int(sizes[1:].max()) if n else 0,
               "label_ms": median_ms(lambda: cc.label(vol)),
               "stats_ms": median_ms(lambda: cc.stats(lab, n)),
               "lut_ms": median_ms(lambda: cc.lut(sizes, largest=True, renumber=True)),
               "select_ms": median_ms(lambda: cc.select(lab, n, largest=True, renumber=True))}
        if not args.no_scipy:
            from scipy import ndimage

            host = vol.cpu().numpy()
            t0 = time.time()
            ref, n_ref = ndimage.label(host)
            row["scipy_label_ms"] = (time.time() - t0) * 1e3
            row["equal_to_scipy"] = bool(n_ref == n and np.array_equal(ref, lab.cpu().numpy()))
            del host, ref
        rec["inputs"].append(row)
        print(json.dumps(row), flush=True)
        del lab, sizes
    out = torch.empty_like(brain)
    rec["fill_holes_call_ms"] = median_ms(lambda: t2.fill_holes(brain, out=out))
    print(json.dumps({"hbm_ms": rec["hbm_ms"], "fill_holes_call_ms": rec["fill_holes_call_ms"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
