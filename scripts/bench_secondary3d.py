"""
Times `FeatureEngine.secondary_volume` (aliby_amd/csrc/feat_secondary3d.hip: the z walk, the y scan and the x scan of one call) with
device events on one stack of the benchmark's config-5 geometry resident on the device: 32 x 512 x 512 voxels with the 100 ellipsoid
nuclei of aliby_amd.synth.make_fov(5, 0).  At unit spacing N = 1, 5 and 16; at spacing (13, 5, 5) — 0.6 um per plane over 0.23 um per
pixel — N = 50, ten pixels.  Beside it, in the same run: a plain device copy that moves the bytes one call moves (20 B per voxel: 2 B
read, the 4-byte z words written and read, the 4-byte y words written and read, 2 B written — so 10 B per voxel read and 10 B
written), `secondary_labels` over the same 32 planes taken as 32 tiles at N = 5 (the 2-D kernels: one intermediate, 12 B per pixel),
and `tertiary_volume` of the cells and the nuclei.  After a warm-up, `windows` windows of `reps` calls (at least 50 calls in all):
median, minimum and maximum per call.  The call's algorithmic bytes over its time are given as a share of the rate the copy reaches in
this run.  The stack is 16.8 MB of labels and 67 MB of words: everything stays in the 256 MiB Infinity Cache, so neither the copy's
rate nor the call's is an HBM figure.  Prints one JSON line and writes it to --out.

    python scripts/bench_secondary3d.py [--reps 5] [--windows 10] [--out profiles/secondary3d_summary.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

RUNS = (("unit_1", 1, (1, 1, 1)), ("unit_5", 5, (1, 1, 1)), ("unit_16", 16, (1, 1, 1)), ("13_5_5_50", 50, (13, 5, 5)))
BYTES_PER_VOXEL = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "secondary3d_summary.json"))
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
    planes = nuclei[0]  # the same 32 planes as 32 tiles
    voxels = nuclei.numel()
    src = torch.randint(0, 255, (BYTES_PER_VOXEL // 2 * voxels,), dtype=torch.uint8, device=nuclei.device)
    dst = torch.empty_like(src)
    calls = {f"secondary_volume_{tag}": (lambda n=n, sp=sp: eng.secondary_volume(nuclei, n, sp)) for tag, n, sp in RUNS}
    calls |= {
        "secondary_labels_32_tiles_5": lambda: eng.secondary_labels(planes, 5),
        "tertiary_volume": lambda: eng.tertiary_volume(cells, nuclei, shrink_inner=True),
        "copy": lambda: dst.copy_(src),
    }
    result = {"labels": list(nuclei.shape), "nuclei": int(nuclei_host.max()), "reps": args.reps, "windows": args.windows}
    result["labelled_share"] = {"primary": round(int((nuclei.view(torch.int16) != 0).sum().item()) / voxels, 4)} | {
        f"secondary_volume_{tag}": round(int((eng.secondary_volume(nuclei, n, sp).view(torch.int16) != 0).sum().item()) / voxels, 4)
        for tag, n, sp in RUNS}
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
    # 2 B read and 2 B written per voxel, and two 4-byte intermediates each written once and read once
    result["secondary_volume_algorithmic_bytes"] = {"labels_in_and_out": 4 * voxels, "intermediates_write_and_read": 16 * voxels,
                                                    "total": BYTES_PER_VOXEL * voxels}
    result["copy_bytes_moved"] = 2 * src.numel()
    copy_rate = 2 * src.numel() / (result["copy_ms"]["median"] * 1e-3)
    result["copy_bytes_per_s"] = round(copy_rate, -9)
    for tag, _, _ in RUNS:
        rate = BYTES_PER_VOXEL * voxels / (result[f"secondary_volume_{tag}_ms"]["median"] * 1e-3)
        result[f"secondary_volume_{tag}_bytes_per_s"] = round(rate, -9)
        result[f"secondary_volume_{tag}_share_of_copy_rate"] = round(rate / copy_rate, 3)
    result["note"] = "labels 16.8 MB and words 67 MB stay in the 256 MiB Infinity Cache: not an HBM figure"
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
