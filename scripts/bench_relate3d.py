"""
Times `FeatureEngine.relate3d` (aliby_amd/csrc/feat_relate3d.hip: both directions; two object tables with their read-backs, two
overlap launches, two finish launches and the wait of one call) and `FeatureEngine.tertiary_volume` with device events on the
benchmark's config-5 geometry resident on the device: one stack 32 x 512 x 512 with about 100 nuclei and 100 cells, ellipsoids over the
objects of aliby_amd.synth.make_fov(5, 0).  Beside them `sizeshape3d` and `intensity3d` on the nuclei in the same run, for scale.  After
a warm-up, `windows` windows of `reps` calls (at least 50 calls in all): median, minimum and maximum per call.  The tertiary pass's
algorithmic bytes (2 reads + 1 write x 2 B per voxel) over its time are given beside the HBM peak; `relate3d` is given beside the
largest boxes of the two sets (each walked by one workgroup) and beside the time that reading the label volumes at HBM speed would
take.  Which kernels the call's time lies in is a kernel trace's to say (rocprofv3 --kernel-trace --stats on this script, a run of its
own; the README has the figures).  Prints one JSON line and writes it to --out.

    python scripts/bench_relate3d.py [--reps 5] [--windows 10] [--out profiles/relate3d_summary.json]
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


def largest_box(vol):
    from scipy import ndimage

    boxes = [s for s in ndimage.find_objects(vol) if s is not None]
    sizes = [[int(a.stop - a.start) for a in s] for s in boxes]
    return max(sizes, key=lambda d: d[0] * d[1] * d[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "relate3d_summary.json"))
    args = ap.parse_args()
    if args.reps * args.windows < 50:
        ap.error("at least 50 timed calls (reps x windows)")
    import torch

    from aliby_amd import synth
    from aliby_amd.extraction.engine import FeatureEngine

    assert torch.cuda.is_available(), "needs the GPU: there is no fallback to time"
    eng = FeatureEngine(0)
    f = synth.make_fov(5, 0)
    n_z = f["pixels"].shape[1]
    nuclei_host = synth.ellipsoid_planes(f["nuclei"], n_z, seed=0)  # (the same seed: a cell's ellipsoid has its nucleus's depth)
    cells_host = synth.ellipsoid_planes(f["cells"], n_z, seed=0)
    nuclei, cells = torch.from_numpy(nuclei_host).cuda()[None], torch.from_numpy(cells_host).cuda()[None]
    px = torch.from_numpy(np.ascontiguousarray(f["pixels"][:2])).cuda()[None]
    cn, cc = [int(nuclei_host.max())], [int(cells_host.max())]
    out_n, out_c = eng.new_output(cn[0], 5), eng.new_output(cc[0], 5)
    out_s, out_i = eng.new_output(cn[0], 19), eng.new_output(cn[0], 12)
    calls = {
        "sizeshape3d": lambda: eng.sizeshape3d(nuclei, cn, out=out_s),
        "intensity3d": lambda: eng.intensity3d(nuclei, px, 0, cn, out=out_i),
        "relate3d": lambda: eng.relate3d(nuclei, cn, cells, cc, out_a=out_n, out_b=out_c),
        "tertiary_volume_shrink": lambda: eng.tertiary_volume(cells, nuclei, shrink_inner=True),
        "tertiary_volume_plain": lambda: eng.tertiary_volume(cells, nuclei, shrink_inner=False),
    }
    result = {"labels": list(nuclei.shape), "nuclei": cn[0], "cells": cc[0], "largest_box_nuclei": largest_box(nuclei_host),
              "largest_box_cells": largest_box(cells_host), "reps": args.reps, "windows": args.windows}
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
    rows = eng.to_host(out_n)
    result["nuclei_with_a_parent"] = int((rows[:, 0] > 0).sum())
    tertiary_bytes = 6 * nuclei.numel()  # 2 reads + 1 write x 2 B per voxel
    result["tertiary_algorithmic_bytes"] = tertiary_bytes
    for what in ("tertiary_volume_shrink", "tertiary_volume_plain"):
        rate = tertiary_bytes / (result[what + "_ms"]["median"] * 1e-3)
        result[what + "_bytes_per_s"] = round(rate, -9)
        result[what + "_share_of_hbm_peak"] = {"of_8.0_TB/s_spec": round(rate / HBM_PEAK_SPEC, 3), "of_6.29_TB/s_copy": round(rate / HBM_PEAK_COPY, 3)}
    result["tertiary_2d_bytes_per_s_config_2"] = {"shrink": 3.8e12, "plain": 5.8e12}  # profiles/relate_summary.json, for comparison
    # what relate3d would take if the two reads of each label volume by the table kernels and the box walks ran at HBM speed
    label_bytes = 2 * nuclei.numel()
    result["relate3d_label_bytes_read_at_least"] = 2 * label_bytes
    result["relate3d_ms_if_hbm_bound"] = round(2 * label_bytes / HBM_PEAK_COPY * 1e3, 4)
    result["relate3d_over_sizeshape3d"] = round(result["relate3d_ms"]["median"] / result["sizeshape3d_ms"]["median"], 3)
    result["relate3d_over_intensity3d"] = round(result["relate3d_ms"]["median"] / result["intensity3d_ms"]["median"], 3)
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
