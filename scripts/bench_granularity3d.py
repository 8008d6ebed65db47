"""
Cost of `FeatureEngine.granularity3d` on the BASELINE config-5 stack that profiles/features3d_config5_summary.json was measured on
(uint16 labels [32, 512, 512], the synthetic ground-truth ellipsoids relabelled 1..n; pixels of channel 0, uint16) at the defaults
(sample sizes 0.25 / 0.25, ball(10), 16 spectrum steps): one stack, and a batch of 8 (the same stack, its pixels rolled by another
amount in each), beside `FeatureEngine.texture3d`, a one-pair `FeatureEngine.coloc3d` and the 2-D `FeatureEngine.granularity` over
the same 32 planes given as 32 frames (the same voxel count: the yardstick) IN THE SAME RUN, the calls alternating.  Times are the
engine's own `timed(...)` device events around each call (object table, kernels, and the waits on the change flag), warm-up calls
discarded; the median over the repetitions is the figure.  Also records the Jacobi sweeps of every spectrum step (flag reads =
sweeps / 16).  Writes profiles/granularity3d_summary.json and prints it as one JSON line.  No gate: nothing here had been timed before.

    python scripts/bench_granularity3d.py [--out PATH] [--warmup 3] [--reps 20]
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
from aliby_amd.extraction.engine import FeatureEngine, to_device_planes, to_device_u16  # noqa: E402

BATCH = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "granularity3d_summary.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_granularity3d needs the GPU: nothing here can be measured without one")
    torch.cuda.set_device(0)
    f = synth.make_fov(5, 0)
    gt = synth.ellipsoid_planes(f["nuclei"], f["pixels"].shape[1], seed=0)
    present = np.unique(gt[gt > 0])
    lut = np.zeros(int(gt.max()) + 1, np.uint16)
    lut[present] = np.arange(1, len(present) + 1)
    lab = lut[gt]                                                   # [32, 512, 512]
    px = np.ascontiguousarray(f["pixels"][:2])                      # [2, 32, 512, 512]: channel 0, and the pair of coloc3d
    n = int(len(present))
    vol = torch.from_numpy(lab).cuda()[None]                        # [1, 32, 512, 512]
    px2 = torch.from_numpy(px).cuda()[None]                         # [1, 2, 32, 512, 512]
    vol8 = vol.expand(BATCH, -1, -1, -1).contiguous()
    px8 = torch.from_numpy(np.stack([np.roll(px[:1], (k, 5 * k, 9 * k), (1, 2, 3)) for k in range(BATCH)])).cuda()  # [8, 1, 32, 512, 512]
    # the 2-D yardstick: the 32 planes as 32 frames, their labels as they are
    dl = to_device_u16(lab)
    dp, dt = to_device_planes(np.ascontiguousarray(px[0][:, None]))  # [32, 1, 512, 512]
    eng = FeatureEngine(0)
    tab = eng.object_table(dl)
    out2d = eng.new_output(tab.n_obj, 16)

    sweeps = {}

    def g3(name, v, p, counts):
        def call():
            eng.granularity3d(v, p, 0, counts)
            sweeps[name] = list(eng.granularity3d_sweeps)
        return call

    calls = {
        "granularity3d_one_stack": g3("granularity3d_one_stack", vol, px2, [n]),
        "granularity3d_batch_of_8": g3("granularity3d_batch_of_8", vol8, px8, [n] * BATCH),
        "granularity_2d_32_frames": lambda: eng.granularity(dl, dp, dt, 0, tab, out2d, 0),
        "texture3d": lambda: eng.texture3d(vol, px2, 0, [n]),
        "coloc3d_one_pair": lambda: eng.coloc3d(vol, px2, [(0, 1)], [n]),
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

    sub, back = FeatureEngine._granularity3d_shapes(*lab.shape, 0.25, 0.25)
    res = {
        "what": "FeatureEngine.granularity3d at the defaults (0.25 / 0.25, ball(10), 16 steps) on the labels of a BASELINE config-5 stack "
                "uint16 [32,512,512] (synthetic ellipsoids), one stack and a batch of 8, beside texture3d, a one-pair coloc3d (four metrics) "
                "and the 2-D granularity over the same 32 planes as 32 frames in the same run, MI355X; per-call ms by the engine's timed(...) "
                "device events (object table, kernels and the waits on the change flag), the calls alternating, warm-ups discarded, median "
                "over the repetitions (scripts/bench_granularity3d.py)",
        "shape": list(lab.shape), "objects": n, "rows_2d": int(tab.n_obj), "subsampled_shape": list(sub), "background_shape": list(back),
        "sweep_cap": sub[0] * sub[1] * sub[2] // 2 + 64, "warmup": args.warmup, "reps": args.reps, "ms": {},
        "sweeps_per_step": sweeps, "flag_reads_per_step": {k: [s // 16 for s in v] for k, v in sweeps.items()},
    }
    for name, v in ms.items():
        res["ms"][name] = dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    base = res["ms"]["granularity_2d_32_frames"]["median"]
    res["over_granularity_2d_32_frames"] = {k: round(v["median"] / base, 3) for k, v in res["ms"].items() if k.startswith("granularity3d")}
    res["ms_per_stack_in_the_batch"] = round(res["ms"]["granularity3d_batch_of_8"]["median"] / BATCH, 4)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
