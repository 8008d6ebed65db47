"""
Times the `neighbors` family (aliby_amd/csrc/feat_neighbors.hip: both kernels of one call) with device events at distance None
(adjacent), 5 and 16 on a config-2-like label block resident on the device: 64 tiles of 1024 x 1024 with about 250 touching cells
each (aliby_amd.synth.make_labels; 8 distinct tiles, each 8 times).  Beside it `sizeshape` on the same object table in the same run.
Median, minimum and maximum of several windows of `reps` calls.  Prints one JSON line.

    python scripts/bench_neighbors.py [--reps 5] [--windows 5] [--tiles 64]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import torch

    from aliby_amd import synth
    from aliby_amd.extraction.engine import FeatureEngine

    assert torch.cuda.is_available(), "needs the GPU: there is no fallback to time"
    eng = FeatureEngine(0)
    distinct = [synth.make_labels(np.random.default_rng(synth.fov_seed(2, k)), (args.size, args.size), 250)[1] for k in range(min(8, args.tiles))]
    labels = torch.from_numpy(np.stack([distinct[k % len(distinct)] for k in range(args.tiles)])).cuda()
    table = eng.object_table(labels)
    out = eng.new_output(table.n_obj, 78)
    calls = {"sizeshape": lambda: eng.sizeshape(labels, table, out, 0)}
    for d in (None, 5, 16):
        calls[f"neighbors_{'adjacent' if d is None else d}"] = lambda d=d: eng.neighbors(labels, table, out, 0, distance=d)
    result = {"labels": list(labels.shape), "objects": table.n_obj, "max_box": [table.max_h, table.max_w], "max_area": table.max_area,
              "reps": args.reps, "windows": args.windows}
    for what, call in calls.items():
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                call()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / args.reps)
        result[what + "_ms"] = {"median": round(float(np.median(per_call)), 3), "min": round(min(per_call), 3), "max": round(max(per_call), 3)}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
