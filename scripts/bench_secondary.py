"""
Times `FeatureEngine.secondary_labels` (aliby_amd/csrc/feat_secondary.hip: the column walk and the row scan of one call) at
N = 1, 5, 16 and 64 with device events on the benchmark's config-2 geometry resident on the device: 64 tiles of 1024 x 1024 with
about 256 nuclei each (aliby_amd.synth.make_labels; 8 distinct tiles, each 8 times).  Beside it, in the same run: `tertiary_labels`
of the cells and the nuclei, `neighbors` on the nuclei table at distances 5 and 16 (the (2N+1)^2 scan the linear one is to leave
behind), and a plain device copy that moves the same bytes as one secondary call (6 B per pixel read and 6 B written, against the
call's 2 B read + 4 B written + 4 B read + 2 B written).  After a warm-up, `windows` windows of `reps` calls (at least 50 calls in
all): median, minimum and maximum per call.  The call's algorithmic bytes over its time at N = 1 are given as a share of the rate the
copy reaches in this run: at N = 1 the kernels do next to no arithmetic, so that share is what the two launches cost over a copy; the
growth with N is the row scan's LDS reads and the column walk's halo rows.  Prints one JSON line and writes it to --out.

    python scripts/bench_secondary.py [--reps 5] [--windows 10] [--tiles 64] [--out profiles/secondary_summary.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

DISTANCES = (1, 5, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "secondary_summary.json"))
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
    tn = eng.object_table(nuclei)
    out_nb = eng.new_output(tn.n_obj, 7)
    pixels = nuclei.numel()
    src = torch.randint(0, 255, (6 * pixels,), dtype=torch.uint8, device=nuclei.device)
    dst = torch.empty_like(src)
    calls = {f"secondary_{n}": (lambda n=n: eng.secondary_labels(nuclei, n)) for n in DISTANCES}
    calls |= {
        "tertiary_shrink": lambda: eng.tertiary_labels(cells, nuclei, shrink_inner=True),
        "tertiary_plain": lambda: eng.tertiary_labels(cells, nuclei, shrink_inner=False),
        "neighbors_5": lambda: eng.neighbors(nuclei, tn, out_nb, 0, distance=5),
        "neighbors_16": lambda: eng.neighbors(nuclei, tn, out_nb, 0, distance=16),
        "copy": lambda: dst.copy_(src),
    }
    result = {"labels": list(nuclei.shape), "nuclei": tn.n_obj, "reps": args.reps, "windows": args.windows}
    grown = {n: int((eng.secondary_labels(nuclei, n).view(torch.int16) != 0).sum().item()) for n in DISTANCES}
    result["labelled_share"] = {"primary": round(int((nuclei.view(torch.int16) != 0).sum().item()) / pixels, 4)} | {
        f"secondary_{n}": round(g / pixels, 4) for n, g in grown.items()}
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
    # 2 B read and 2 B written per pixel, and the 4-byte intermediate written once and read once
    result["secondary_algorithmic_bytes"] = {"labels_in_and_out": 4 * pixels, "intermediate_write_and_read": 8 * pixels, "total": 12 * pixels}
    copy_rate = 2 * src.numel() / (result["copy_ms"]["median"] * 1e-3)
    result["copy_bytes_per_s"] = round(copy_rate, -9)
    for n in DISTANCES:
        rate = 12 * pixels / (result[f"secondary_{n}_ms"]["median"] * 1e-3)
        result[f"secondary_{n}_bytes_per_s"] = round(rate, -9)
    result["secondary_1_share_of_copy_rate"] = round(result["secondary_1_bytes_per_s"] / copy_rate, 3)
    for n in (5, 16):
        result[f"neighbors_{n}_over_secondary_{n}"] = round(result[f"neighbors_{n}_ms"]["median"] / result[f"secondary_{n}_ms"]["median"], 1)
    line = json.dumps(result)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
