"""
Cost of the volume feature families on a BASELINE config-5 stack (uint16 labels [32, 512, 512], the synthetic ground-truth
ellipsoids relabelled 1..n; pixels of channel 0): `FeatureEngine.intensity3d` (4 bytes per voxel: labels + pixels) and
`FeatureEngine.sizeshape3d` (2 bytes per voxel, 2.57 with the low-side halo of its 8 x 8 x 64 tiles), one stack and a batch of 8,
and `FeatureEngine.coloc3d` on both channels (one pair, all four metrics: the labels once for the object table, then per object
the labels of its bounding box and its voxels of both channels; `coloc3d_bytes`), and `FeatureEngine.texture3d` on channel 0
(scale 3, 256 grey levels: the labels once for the object table, then labels and pixels of every bounding box; `texture3d_bytes`),
and `FeatureEngine.sizeshape3d(..., surface_area=True)`: the same sizeshape3d launch followed by the SurfaceArea pass (section
"surface3d": histogram memset, table and offsets upload, k_surface3d and its finish; 2 bytes per voxel again).
Times are the engine's own `timed(...)` events around each call (memsets, offsets upload, accumulation and finalise kernels), the
families alternating, warm-up calls discarded; prints one JSON line.  The 16.8 MB of labels of one stack stay resident in
the 256 MB Infinity Cache between repeats, so the "fraction of HBM peak" of F = 1 is a rate against the HBM figure, not proof of
HBM traffic; the batch of 8 (134 MB labels + 134 MB pixels) does not fit for intensity3d.
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/profile_features3d.py` for the per-kernel times.
"""

from __future__ import annotations

import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from aliby_amd import synth  # noqa: E402
from aliby_amd.extraction.engine import FeatureEngine  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X specification
TILE = (8, 8, 64)


def staged_bytes(F, Z, Y, X):
    """What sizeshape3d's workgroups read: every tile of the corner grid with its one-voxel low-side halo, clipped to the volume."""
    per_axis = []
    for n, t in zip((Z, Y, X), TILE):
        reads = 0
        for k in range(n // t + 1):
            lo, hi = max(k * t - 1, 0), min(k * t + t, n)
            reads += max(hi - lo, 0)
        per_axis.append(reads)
    return 2 * F * per_axis[0] * per_axis[1] * per_axis[2]


def coloc3d_bytes(labels, n, F, n_pairs=1, px_bytes=2):
    """Bytes coloc3d asks for: the label volume once (object table), then per object and pair the labels of the bounding box and
    the object's voxels of two channels.  -> (bytes, largest object in voxels)."""
    from scipy import ndimage as ndi

    lab = labels.cpu().numpy()
    counts = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    boxes = sum(int(np.prod([s.stop - s.start for s in sl])) for sl in ndi.find_objects(lab.astype(np.int32), n) if sl is not None)
    return F * (2 * lab.size + n_pairs * (2 * boxes + 2 * px_bytes * int(counts.sum()))), int(counts.max())


def texture3d_bytes(labels, n, F, px_bytes=2):
    """Bytes texture3d asks for: the label volume once (object table), then labels and pixels of every bounding box.
    -> (bytes, voxels of every box)."""
    from scipy import ndimage as ndi

    lab = labels.cpu().numpy()
    boxes = np.asarray([int(np.prod([s.stop - s.start for s in sl])) for sl in ndi.find_objects(lab.astype(np.int32), n) if sl is not None])
    return F * (2 * lab.size + (2 + px_bytes) * int(boxes.sum())), boxes


def main(warmup=3, reps=20):
    torch.cuda.set_device(0)
    f = synth.make_fov(5, 0)
    gt = synth.ellipsoid_planes(f["nuclei"], f["pixels"].shape[1], seed=0)
    present = np.unique(gt[gt > 0])
    lut = np.zeros(int(gt.max()) + 1, np.uint16)
    lut[present] = np.arange(1, len(present) + 1)
    labels = torch.from_numpy(lut[gt]).cuda()              # [32, 512, 512]
    pixels = torch.from_numpy(f["pixels"][:1]).cuda()      # [1, 32, 512, 512]
    pixels2 = torch.from_numpy(f["pixels"][:2]).cuda()     # [2, 32, 512, 512]: the pair of coloc3d
    eng = FeatureEngine(0)
    res = {"shape": list(labels.shape), "objects": int(len(present)), "foreground_fraction": round(float((gt > 0).mean()), 4),
           "hbm_peak_bytes_per_s": HBM_PEAK, "warmup": warmup, "reps": reps}
    for F in (1, 8):
        vol = labels[None].expand(F, -1, -1, -1).contiguous()
        px = pixels[None].expand(F, -1, -1, -1, -1).contiguous()
        px2 = pixels2[None].expand(F, -1, -1, -1, -1).contiguous()
        counts = [int(len(present))] * F
        eng.profile = {}
        for _ in range(warmup):
            eng.intensity3d(vol, px, 0, counts)
            eng.sizeshape3d(vol, counts)
            eng.sizeshape3d(vol, counts, surface_area=True)
            eng.coloc3d(vol, px2, [(0, 1)], counts)
            eng.texture3d(vol, px, 0, counts)
        torch.cuda.synchronize()
        eng.profile = {}
        for _ in range(reps):
            eng.intensity3d(vol, px, 0, counts)
            eng.sizeshape3d(vol, counts)
            eng.sizeshape3d(vol, counts, surface_area=True)
            eng.coloc3d(vol, px2, [(0, 1)], counts)
            eng.texture3d(vol, px, 0, counts)
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in eng.profile.items()}
        eng.profile = None
        # "sizeshape3d" was bracketed twice per repeat: the plain call, then the same launch inside the call with surface_area
        plain, flagged = ms["sizeshape3d"][0::2], ms["sizeshape3d"][1::2]
        ms["sizeshape3d"] = plain
        with_area = [a + b for a, b in zip(flagged, ms["surface3d"])]
        voxels = vol.numel()
        c3_bytes, c3_largest = coloc3d_bytes(labels, len(present), F)
        t3_bytes, t3_boxes = texture3d_bytes(labels, len(present), F)
        moved = {"intensity3d": 4 * voxels, "sizeshape3d": 2 * voxels, "surface3d": 2 * voxels, "coloc3d": c3_bytes, "texture3d": t3_bytes}
        out = {}
        for name in ("intensity3d", "sizeshape3d", "surface3d", "coloc3d", "texture3d"):
            med, best = statistics.median(ms[name]), min(ms[name])
            out[name] = dict(ms_median=round(med, 4), ms_min=round(best, 4), ms_max=round(max(ms[name]), 4), bytes_algorithmic=moved[name],
                             fraction_of_hbm_peak=round(moved[name] / (med * 1e-3) / HBM_PEAK, 4))
        out["sizeshape3d"]["bytes_staged_with_halo"] = staged_bytes(F, *labels.shape)
        out["coloc3d"].update(largest_object_voxels=c3_largest, lds_budget_voxels=eng.coloc3d_lds_voxels,
                              objects_in_global_scratch_form=int((np.bincount(lut[gt].ravel())[1:] > eng.coloc3d_lds_voxels).sum()) * F)
        out["texture3d"].update(largest_box_voxels=int(t3_boxes.max()), lds_budget_box_voxels=eng.texture3d_lds_voxels,
                                objects_in_global_scratch_form=int((t3_boxes > eng.texture3d_lds_voxels).sum()) * F)
        out["sizeshape3d_with_surface_area"] = dict(ms_median=round(statistics.median(with_area), 4), ms_min=round(min(with_area), 4),
                                                    ms_max=round(max(with_area), 4),
                                                    over_plain=round(statistics.median(with_area) / out["sizeshape3d"]["ms_median"], 3))
        out["sizeshape3d_over_intensity3d"] = round(out["sizeshape3d"]["ms_median"] / out["intensity3d"]["ms_median"], 3)
        res[f"F{F}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
