"""
Times `FeatureEngine.auto_threshold` (aliby_amd/csrc/feat_threshold.hip: the histogram launch of csrc/tile_crop.hip and the search)
with device events on the scene of scripts/bench_propagate.py resident on the device: 64 tiles of 1024 x 1024 with about 256 nuclei
each and the synthetic stain (8 distinct tiles, each 8 times).  Two forms, two and three classes, beside — in the same run — the
`propagate_labels` call thresholded at the stain's median (the scalar form), the same call fed the per-tile thresholds from the
device, the two calls chained (auto_threshold, then propagate_labels(thresholds=...)), and a plain device copy of 1 GiB (512 MiB a side,
beyond the Infinity Cache).  The traffic the threshold implies — the histogram launch reads every plane twice at 2 B per pixel (its two
workgroup roles), then zeroes, adds into and reads back 256 KiB of bins per tile — is set against the time a copy of as many bytes
takes at that rate; at 134 MB a side the planes fit the Infinity Cache between calls, so the threshold's own rate is no HBM figure.
After a warm-up, `windows` windows of `reps` calls (at least 50 calls in all): median, minimum and maximum per call.  Prints one JSON
line and writes it to --out.

    python scripts/bench_threshold.py [--reps 5] [--windows 10] [--tiles 64] [--out profiles/threshold_summary.json]
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
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "threshold_summary.json"))
    args = ap.parse_args()
    if args.reps * args.windows < 50:
        ap.error("at least 50 timed calls (reps x windows)")
    import torch

    from aliby_amd import synth
    from aliby_amd.extraction.engine import FeatureEngine

    assert torch.cuda.is_available(), "needs the GPU: there is no fallback to time"
    eng = FeatureEngine(0)
    rng = np.random.default_rng(5)
    distinct = []
    for k in range(min(8, args.tiles)):
        nuc, cell = synth.make_labels(np.random.default_rng(synth.fov_seed(2, k)), (args.size, args.size), 256)[:2]
        stain = np.where(cell != 0, 12000, 1500) + rng.integers(0, 2000, cell.shape)
        distinct.append((nuc, stain.astype(np.uint16)))
    nuclei = torch.from_numpy(np.stack([distinct[k % len(distinct)][0] for k in range(args.tiles)])).cuda()
    image = torch.from_numpy(np.stack([distinct[k % len(distinct)][1] for k in range(args.tiles)])).cuda()
    threshold = int(np.median(np.stack([d[1] for d in distinct])))
    pixels = nuclei.numel()
    F, Y, X = nuclei.shape
    forms = {"auto_threshold_2": dict(classes=2), "auto_threshold_3": dict(classes=3)}
    result = {"image": [F, Y, X], "reps": args.reps, "windows": args.windows, "median_threshold": threshold,
              "workspace_bytes": int(eng.lib.aliby_auto_threshold_workspace_bytes(F))}
    for what, kw in forms.items():
        thresholds, details = eng.auto_threshold(image, return_details=True, **kw)
        result[what] = {"thresholds_of_the_distinct_tiles": thresholds.cpu().tolist()[:len(distinct)],
                        "details_of_tile_0": details.cpu().tolist()[0]}
    per_tile = eng.auto_threshold(image, classes=2)
    eng.propagate_labels(nuclei, image, threshold=threshold)
    result["propagate_rounds"] = {"scalar": eng.propagate_stats[0]}
    eng.propagate_labels(nuclei, image, thresholds=per_tile)
    result["propagate_rounds"]["per_tile"] = eng.propagate_stats[0]
    # the planes twice, the bins zeroed, added into (at most once per bin, role and slice) and read by the search
    algorithmic = 2 * 2 * pixels + 3 * 4 * 65536 * F
    result["auto_threshold_algorithmic_bytes"] = {"planes_read_twice": 4 * pixels, "bins_zeroed_added_read": 12 * 65536 * F, "total": algorithmic}
    half = 512 << 20
    src = torch.randint(0, 255, (half,), dtype=torch.uint8, device=nuclei.device)
    dst = torch.empty_like(src)
    calls = {what: (lambda kw=kw: eng.auto_threshold(image, **kw)) for what, kw in forms.items()}
    calls |= {"propagate_scalar": lambda: eng.propagate_labels(nuclei, image, threshold=threshold),
              "propagate_per_tile": lambda: eng.propagate_labels(nuclei, image, thresholds=per_tile),
              "auto_threshold_2_then_propagate": lambda: eng.propagate_labels(nuclei, image, thresholds=eng.auto_threshold(image, classes=2)),
              "copy": lambda: dst.copy_(src)}
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
    copy_rate = 2 * half / (result["copy_ms"]["median"] * 1e-3)
    result["copy_bytes"] = 2 * half
    result["copy_bytes_per_s"] = round(copy_rate, -9)
    result["copy_of_algorithmic_bytes_ms"] = round(algorithmic / copy_rate * 1e3, 4)
    for what in forms:
        ms = result[what + "_ms"]["median"]
        result[what + "_share_of_propagate_scalar"] = round(ms / result["propagate_scalar_ms"]["median"], 4)
        result[what + "_bytes_per_s"] = round(algorithmic / (ms * 1e-3), -9)
        result[what + "_share_of_copy_rate"] = round(algorithmic / (ms * 1e-3) / copy_rate, 3)
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
