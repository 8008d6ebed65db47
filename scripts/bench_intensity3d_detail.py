"""
Cost of `FeatureEngine.intensity3d_detail` on the BASELINE config-5 stack that profiles/features3d_config5_summary.json was measured
on (uint16 labels [32, 512, 512], the synthetic ground-truth ellipsoids relabelled 1..n; pixels of channel 0, as uint16 and as
float32 in [0, 1]): the call with and without the edge columns, beside `FeatureEngine.intensity3d` and a one-pair
`FeatureEngine.coloc3d` (all four metrics) IN THE SAME RUN, the calls alternating.  Times are the engine's own `timed(...)` device
events around each call (object table, read-back, kernels), warm-up calls discarded.  Writes profiles/intensity3d_detail_summary.json
and prints it as one JSON line.  No gate: the expectation that the call costs about what a one-pair coloc3d costs (both are bounded
by the sorts of the largest object) is only that until this file exists; DESIGN.md discusses the measured ratio.

    python scripts/bench_intensity3d_detail.py [--out PATH] [--warmup 3] [--reps 20]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from aliby_amd import synth  # noqa: E402
from aliby_amd.extraction.engine import FeatureEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "intensity3d_detail_summary.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_intensity3d_detail needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    f = synth.make_fov(5, 0)
    gt = synth.ellipsoid_planes(f["nuclei"], f["pixels"].shape[1], seed=0)
    present = np.unique(gt[gt > 0])
    lut = np.zeros(int(gt.max()) + 1, np.uint16)
    lut[present] = np.arange(1, len(present) + 1)
    lab = lut[gt]
    sizes = np.bincount(lab.ravel())[1:]
    vol = torch.from_numpy(lab).cuda()[None]                       # [1, 32, 512, 512]
    px2 = torch.from_numpy(f["pixels"][:2]).cuda()[None]           # [1, 2, 32, 512, 512]: channel 0, and the pair of coloc3d
    pxf = (px2[:, :1].to(torch.float32) / 65535.0).contiguous()    # [1, 1, 32, 512, 512] float32
    counts = [int(len(present))]
    eng = FeatureEngine(0)

    calls = {
        "intensity3d": lambda: eng.intensity3d(vol, px2, 0, counts),
        "coloc3d_one_pair": lambda: eng.coloc3d(vol, px2, [(0, 1)], counts),
        "detail_u16_edge": lambda: eng.intensity3d_detail(vol, px2, 0, counts, True),
        "detail_u16_no_edge": lambda: eng.intensity3d_detail(vol, px2, 0, counts, False),
        "detail_f32_edge": lambda: eng.intensity3d_detail(vol, pxf, 0, counts, True),
        "detail_f32_no_edge": lambda: eng.intensity3d_detail(vol, pxf, 0, counts, False),
    }
    ms = {k: [] for k in calls}
    for rep in range(args.warmup + args.reps):
        for name, call in calls.items():
            eng.profile = {}
            call()
            torch.cuda.synchronize()
            (pair,) = [p for v in eng.profile.values() for p in v]
            if rep >= args.warmup:
                ms[name].append(pair[0].elapsed_time(pair[1]))
    eng.profile = None

    budget = eng.intensity3d_detail_lds_voxels
    res = {
        "what": "FeatureEngine.intensity3d_detail beside intensity3d and a one-pair coloc3d (four metrics) in the same run, on the labels of a "
                "BASELINE config-5 stack uint16 [32,512,512] (synthetic ellipsoids), MI355X; per-call ms by the engine's timed(...) device "
                "events (object table, read-back and kernels), the calls alternating, warm-ups discarded (scripts/bench_intensity3d_detail.py)",
        "shape": list(lab.shape), "objects": int(len(present)), "foreground_fraction": round(float((lab > 0).mean()), 4),
        "largest_object_voxels": int(sizes.max()), "median_object_voxels": int(np.median(sizes)),
        "lds_budget_voxels": budget, "objects_in_global_scratch_form": int((sizes > budget).sum()),
        "coloc3d_lds_budget_voxels": eng.coloc3d_lds_voxels, "coloc3d_objects_in_global_scratch_form": int((sizes > eng.coloc3d_lds_voxels).sum()),
        "warmup": args.warmup, "reps": args.reps, "ms": {},
    }
    for name, v in ms.items():
        res["ms"][name] = dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    base = res["ms"]["coloc3d_one_pair"]["median"]
    res["over_coloc3d_one_pair"] = {k: round(v["median"] / base, 3) for k, v in res["ms"].items() if k.startswith("detail")}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
