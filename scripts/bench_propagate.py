"""
Times `FeatureEngine.propagate_labels` (aliby_amd/csrc/feat_propagate.hip: the weights pass, the rounds between reads of the change
flags, the unpacking) with device events on the table of scripts/bench_secondary.py resident on the device: 64 tiles of 1024 x 1024
with about 256 nuclei each (aliby_amd.synth.make_labels; 8 distinct tiles, each 8 times), plus a synthetic stain: bright where the
synthetic cell of a nucleus lies, dark elsewhere, noise on both, and the threshold at the stain's median, which keeps about half the
pixels.  Three forms: "Propagation" with the threshold, the same within 16 pixels, and "Distance - B" (threshold 0, distance 16).
Beside them, in the same run: `secondary_labels` at N = 16 and a plain device copy of 1 GiB (512 MiB a side, beyond the Infinity
Cache), whose rate gives the time a copy of the algorithmic bytes of one thresholded call would take (per pixel 6 B of labels and
image in and out, 24 B of keys and weights written once, and per executed round 8 B + 8 B of keys and 16 B of weights; the rounds
executed are the changing ones and the one that finds nothing to change).  After a warm-up, `windows`
windows of `reps` calls (at least 50 calls in all): median, minimum and maximum per call; the call waits on its stream at every read
of the flags, so the events bracket those waits too.  Prints one JSON line and writes it to --out.

    python scripts/bench_propagate.py [--reps 5] [--windows 10] [--tiles 64] [--out profiles/propagate_summary.json]
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "propagate_summary.json"))
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
    forms = {"propagate": dict(threshold=threshold), "propagate_within_16": dict(threshold=threshold, distance=16),
             "distance_b_16": dict(threshold=0, distance=16)}
    result = {"labels": [F, Y, X], "nuclei": int(eng.object_table(nuclei).n_obj), "reps": args.reps, "windows": args.windows,
              "threshold": threshold, "workspace_bytes": int(eng.lib.aliby_propagate_workspace_bytes(F, Y, X)),
              "labelled_share": {"primary": round(int((nuclei.view(torch.int16) != 0).sum().item()) / pixels, 4),
                                 "at_or_above_threshold": round(int((image.to(torch.int32) >= threshold).sum().item()) / pixels, 4)}}
    for what, kw in forms.items():
        out = eng.propagate_labels(nuclei, image, **kw)
        rounds, reads = eng.propagate_stats
        result[what] = {"rounds": rounds, "flag_reads": reads, "labelled_share": round(int((out.view(torch.int16) != 0).sum().item()) / pixels, 4)}
        del out
    executed = result["propagate"]["rounds"] + 1
    algorithmic = (6 + 24 + 32 * executed) * pixels
    result["propagate_algorithmic_bytes"] = {"labels_image_in_and_out": 6 * pixels, "keys_and_weights_written": 24 * pixels,
                                             "per_executed_round": 32 * pixels, "executed_rounds": executed, "total": algorithmic}
    # a copy reads and writes: half the bytes each way.  512 MiB a side is twice the 256 MB Infinity Cache, so the rate is HBM's, and
    # the time of a copy of the call's algorithmic bytes follows from the rate: no need to hold gigabytes on a shared device
    half = min(algorithmic // 2, 512 << 20)
    src = torch.randint(0, 255, (half,), dtype=torch.uint8, device=nuclei.device)
    dst = torch.empty_like(src)
    calls = {what: (lambda kw=kw: eng.propagate_labels(nuclei, image, **kw)) for what, kw in forms.items()}
    calls |= {"secondary_16": lambda: eng.secondary_labels(nuclei, 16), "copy": lambda: dst.copy_(src)}
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
    result["propagate_bytes_per_s"] = round(algorithmic / (result["propagate_ms"]["median"] * 1e-3), -9)
    result["propagate_share_of_copy_rate"] = round(result["propagate_bytes_per_s"] / copy_rate, 3)
    result["propagate_ms_per_executed_round"] = round(result["propagate_ms"]["median"] / executed, 4)
    result["propagate_over_secondary_16"] = round(result["propagate_ms"]["median"] / result["secondary_16_ms"]["median"], 1)
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
