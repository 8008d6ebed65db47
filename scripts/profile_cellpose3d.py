"""
Cost of cellpose's do_3D mode on a BASELINE config-5 stack (uint16 [32, 512, 512]): `CellposeModel.eval(do_3D=True)` with the
fused bf16 network (random weights: cellpose's checkpoints cannot be fetched offline), one stack and a batch of 8.  Prints one JSON
line with event-timed milliseconds of the network leg (normalisation + three orthogonal passes) and of the 3-D dynamics, the
latter on the network's flows and on analytic flows of the synthetic ground truth (what trained weights would resemble).
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/profile_cellpose3d.py` for the per-kernel summary.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from aliby_amd import synth  # noqa: E402
from aliby_amd.segment import dynamics  # noqa: E402
from aliby_amd.segment.cellpose_hip import CellposeModel  # noqa: E402


def timed(fn, reps=3):
    out, best = None, float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return out, best


def main():
    torch.cuda.set_device(0)
    f = synth.make_fov(5, 0)
    gt = synth.ellipsoid_planes(f["nuclei"], f["pixels"].shape[1], seed=0)
    stack = torch.from_numpy(f["pixels"][0]).cuda()  # [32, 512, 512]
    dP_a, prob_a = (torch.from_numpy(a).cuda() for a in synth.analytic_flows_3d(gt))
    model = CellposeModel(seed=0)
    res = {"shape": list(stack.shape), "batch_size": model.batch_size}
    for F in (1, 8):
        vol = stack[None].expand(F, -1, -1, -1).contiguous()
        model.eval(vol, do_3D=True, normalize=dict(norm3D=False))  # warm-up (weight packing, workspaces)
        (dP, prob), t_net = timed(lambda: model.run_network_3d(model.normalize_3d(vol, False)))
        (_, n), t_dyn = timed(lambda: dynamics.masks_from_flows_3d(model.eng, dP, prob))
        dPa, proba = dP_a[None].expand(F, -1, -1, -1, -1).contiguous(), prob_a[None].expand(F, -1, -1, -1).contiguous()
        (_, na), t_dyn_a = timed(lambda: dynamics.masks_from_flows_3d(model.eng, dPa, proba))
        res[f"F{F}"] = dict(network_ms=round(t_net, 2), dynamics_network_flows_ms=round(t_dyn, 2),
                            dynamics_analytic_flows_ms=round(t_dyn_a, 2), network_ms_per_stack=round(t_net / F, 2),
                            dynamics_analytic_ms_per_stack=round(t_dyn_a / F, 2), objects_analytic=[int(v) for v in na],
                            objects_network_flows=[int(v) for v in n])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
