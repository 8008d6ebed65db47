"""
Cost of the volume instruction tree and of `FeatureEngine.projection3d` on the BASELINE config-5 stack the other volume summaries
were measured on (uint16 labels [32, 512, 512], the synthetic ground-truth ellipsoids relabelled 1..n; pixels uint16, C = 2):

  * `projection3d` beside `intensity3d` (the nearest yardstick: it reads labels and pixels once) IN THE SAME RUN, the calls
    alternating, each timed by the engine's own `timed(...)` device events;
  * the example tree (sizeshape3d, neighbors3d, projection3d / intensity3d, intensity3d_detail, texture3d on channel 0 /
    intensity3d, granularity3d on channel 1 / the four colocalisation metrics of the pair) through `process_tree_volumes`, beside
    the same families called one by one, joined with torch.cat and downloaded with the same `to_host`, in the same run: device
    events around each whole call on the main stream (both sides wait on their stream in between, so the events span the host's
    share too).  The tree launches the same kernels and drops the copies; it should stay within 5 % of the sum.

Warm-up calls discarded; the median over the repetitions is the figure.  Writes profiles/volume_tree_summary.json and prints it as
one JSON line.  No gate: nothing here had been timed before.

    python scripts/bench_volume_tree.py [--out PATH] [--warmup 3] [--reps 15]
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
from aliby_amd.extraction.extract import process_tree_volumes  # noqa: E402

TREE = {"None": {"None": ["sizeshape3d", "neighbors3d", "projection3d"]},
        0: {"None": ["intensity3d", "intensity3d_detail", "texture3d"]},
        1: {"None": ["intensity3d", "granularity3d"]},
        (0, 1): {"None": ["pearson", "manders_fold", "rwc", "costes"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "volume_tree_summary.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_tree needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    f = synth.make_fov(5, 0)
    gt = synth.ellipsoid_planes(f["nuclei"], f["pixels"].shape[1], seed=0)
    present = np.unique(gt[gt > 0])
    lut = np.zeros(int(gt.max()) + 1, np.uint16)
    lut[present] = np.arange(1, len(present) + 1)
    lab = lut[gt]                                                   # [32, 512, 512]
    n = int(len(present))
    vol = torch.from_numpy(lab).cuda()[None]                        # [1, 32, 512, 512]
    px = torch.from_numpy(np.ascontiguousarray(f["pixels"][:2])).cuda()[None]  # [1, 2, 32, 512, 512]
    counts = [n]
    eng = FeatureEngine(0)

    def one_by_one():
        blocks = [eng.sizeshape3d(vol, counts), eng.neighbors3d(vol, counts), eng.projection3d(vol, counts),
                  eng.intensity3d(vol, px, 0, counts), eng.intensity3d_detail(vol, px, 0, counts), eng.texture3d(vol, px, 0, counts),
                  eng.intensity3d(vol, px, 1, counts), eng.granularity3d(vol, px, 1, counts),
                  eng.coloc3d(vol, px, [(0, 1)], counts)]
        return eng.to_host(torch.cat(blocks, 1))

    def tree():
        return process_tree_volumes(TREE, vol, px, counts=counts)[1].matrix

    a, b = one_by_one(), tree()
    same = a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))

    # 1. the new kernel beside its yardstick, by the engine's own events
    single = {"projection3d": lambda: eng.projection3d(vol, counts), "intensity3d": lambda: eng.intensity3d(vol, px, 0, counts)}
    ms = {k: [] for k in (*single, "tree", "one_by_one_and_cat")}
    for rep in range(args.warmup + args.reps):
        for name, call in single.items():
            eng.profile = {}
            call()
            torch.cuda.synchronize()
            (pair,) = [p for v in eng.profile.values() for p in v]
            if rep >= args.warmup:
                ms[name].append(pair[0].elapsed_time(pair[1]))
    eng.profile = None
    # 2. the tree beside the same families one by one, whole calls between two events
    whole = {"tree": tree, "one_by_one_and_cat": one_by_one}
    for rep in range(args.warmup + args.reps):
        for name, call in whole.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[name].append(t0.elapsed_time(t1))

    res = {
        "what": "FeatureEngine.projection3d beside intensity3d (per-call ms by the engine's timed(...) device events), and the example "
                "volume tree through process_tree_volumes beside the same families called one by one + torch.cat + the same download "
                "(device events around each whole call), on the labels of a BASELINE config-5 stack uint16 [32,512,512] (synthetic "
                "ellipsoids), C = 2, MI355X; the calls alternating in the same run, warm-ups discarded, median over the repetitions "
                "(scripts/bench_volume_tree.py)",
        "shape": list(lab.shape), "objects": n, "columns": int(b.shape[1]), "tree_equals_one_by_one_bitwise": same,
        "label_bytes": int(lab.size * 2), "warmup": args.warmup, "reps": args.reps, "ms": {},
    }
    for name, v in ms.items():
        res["ms"][name] = dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    res["projection3d_label_GBps"] = round(res["label_bytes"] / (res["ms"]["projection3d"]["median"] * 1e-3) / 1e9, 1)
    res["projection3d_over_intensity3d"] = round(res["ms"]["projection3d"]["median"] / res["ms"]["intensity3d"]["median"], 3)
    res["tree_over_one_by_one"] = round(res["ms"]["tree"]["median"] / res["ms"]["one_by_one_and_cat"]["median"], 4)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
