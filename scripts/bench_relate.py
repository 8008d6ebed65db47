"""
Times `FeatureEngine.relate` (aliby_amd/csrc/feat_relate.hip: both directions, four launches and two memsets of one call) and
`FeatureEngine.tertiary_labels` with device events on the benchmark's config-2 geometry resident on the device: 64 tiles of
1024 x 1024 with about 256 nuclei and 256 cells each (aliby_amd.synth.make_labels; 8 distinct tiles, each 8 times).  Beside them
`sizeshape` on the nuclei table in the same run.  After a warm-up, `windows` windows of `reps` calls (at least 50 calls in all):
median, minimum and maximum per call.  The tertiary kernel's algorithmic bytes (2 reads + 1 write x 2 B per pixel) over its time
are given as a share of the HBM peak (8.0 TB/s by specification; 6.29 TB/s is what a float4 copy reaches), which is the bound that
holds for it: it does no arithmetic to speak of.  Prints one JSON line and writes it to --out.

    python scripts/bench_relate.py [--reps 5] [--windows 10] [--tiles 64] [--out profiles/relate_summary.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_PEAK_SPEC = 8.0e12      # bytes / s
HBM_PEAK_COPY = 6.29e12     # measured with a float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "relate_summary.json"))
    args = ap.parse_args()
    if args.reps * args.windows < 50:
        ap.error("at least 50 timed calls (reps x windows)")
    import torch

    from aliby_amd import synth
    from aliby_amd.extraction.engine import FeatureEngine

    assert torch.cuda.is_available(), "needs the GPU: there is no fallback to time"
    eng = FeatureEngine(0)
    distinct = [synth.make_labels(np.random.default_rng(synth.fov_seed(2, k)), (args.size, args.size), 256)[:2] for k in range(min(8, args.tiles))]
    nuclei = torch.from_numpy(np.stack([distinct[k % len(distinct)][0] for k in range(args.tiles)])).cuda()
    cells = torch.from_numpy(np.stack([distinct[k % len(distinct)][1] for k in range(args.tiles)])).cuda()
    tn, tc = eng.object_table(nuclei), eng.object_table(cells)
    out_n, out_c, out_s = eng.new_output(tn.n_obj, 5), eng.new_output(tc.n_obj, 5), eng.new_output(tn.n_obj, 78)
    calls = {
        "sizeshape": lambda: eng.sizeshape(nuclei, tn, out_s, 0),
        "relate": lambda: eng.relate(nuclei, tn, cells, tc, out_a=out_n, out_b=out_c),
        "tertiary_shrink": lambda: eng.tertiary_labels(cells, nuclei, shrink_inner=True),
        "tertiary_plain": lambda: eng.tertiary_labels(cells, nuclei, shrink_inner=False),
    }
    result = {"labels": list(nuclei.shape), "nuclei": tn.n_obj, "cells": tc.n_obj, "max_box_nuclei": [tn.max_h, tn.max_w],
              "max_box_cells": [tc.max_h, tc.max_w], "reps": args.reps, "windows": args.windows}
    for what, call in calls.items():
        for _ in range(3):
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
        result[what + "_ms"] = {"median": round(float(np.median(per_call)), 4), "min": round(min(per_call), 4), "max": round(max(per_call), 4)}
    tertiary_bytes = 6 * nuclei.numel()  # 2 reads + 1 write x 2 B per pixel
    result["tertiary_algorithmic_bytes"] = tertiary_bytes
    for what in ("tertiary_shrink", "tertiary_plain"):
        rate = tertiary_bytes / (result[what + "_ms"]["median"] * 1e-3)
        result[what + "_bytes_per_s"] = round(rate, -9)
        result[what + "_share_of_hbm_peak"] = {"of_8.0_TB/s_spec": round(rate / HBM_PEAK_SPEC, 3), "of_6.29_TB/s_copy": round(rate / HBM_PEAK_COPY, 3)}
    result["tertiary_bound"] = "HBM bandwidth"
    result["relate_over_sizeshape"] = round(result["relate_ms"]["median"] / result["sizeshape_ms"]["median"], 3)
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
