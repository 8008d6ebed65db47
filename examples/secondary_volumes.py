"""
Nuclei, cells and the cytoplasm of one Z-stack from the nuclear stain alone, in 3-D, through the step API on one MI355X.

`secondary={"cell": ("nuclei", N)}` grows a cell around every nucleus (CellProfiler's IdentifySecondaryObjects, method
"Distance - N"), but on the collapsed 2-D masks, where every nucleus hides the cytoplasm above and below it.  One more keyword grows
the volume labels themselves, on an integer lattice (csrc/feat_secondary3d.hip; the definition is pinned in include/aliby_hip.h):

    build_pipeline_steps(channels_to_segment={"nuclei": 0}, volume_features=("intensity3d",),
                         secondary={"cell": ("nuclei", 4)}, tertiary={"cytoplasm": ("cell", "nuclei")},
                         relate=[("nuclei", "cell")], volume_relate=True,
                         volume_secondary=(13, 5))   # a plane step is 13/5 pixels: 0.6 um per plane over 0.23 um per pixel

`profiles3d/` then has nuclei, cell and cytoplasm rows keyed by the nucleus's volume label: one network pass, three kinds of row.
`volume_secondary=True` is unit spacing.  Such a pipeline runs position by position through `run_pipeline_and_post` (the batched
`run_positions` refuses it).

Segmentation needs Cellpose weights; none are obtainable offline.  The script draws a synthetic two-channel stack of ellipsoid nuclei
and feeds the 3-D dynamics the analytic flow fields of its ground truth through `flows_override`.

    python examples/secondary_volumes.py [--planes 8] [--size 96] [--distance 4] [--isotropic] [--out DIR]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path
from tempfile import mkdtemp

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

VOLUME, MEAN = "None/None/sizeshape3d/Volume", "1/None/intensity3d/Intensity_MeanIntensity"


def synthetic_stack(planes: int, size: int, seed: int = 7):
    """-> (pixels uint16 [T=1,C=2,Z,Y,X], nuclei uint16 [Z,Y,X]): a 3 x 3 grid of ellipsoid nuclei; channel 1 is brighter near them."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.mgrid[0:planes, 0:size, 0:size]
    nuclei, near = np.zeros((planes, size, size), np.uint16), np.zeros((planes, size, size), bool)
    pitch = size / 3.0
    label = 0
    for gy in range(3):
        for gx in range(3):
            label += 1
            c = (planes / 2.0 + rng.uniform(-0.5, 0.5), (gy + 0.5) * pitch + rng.uniform(-2, 2), (gx + 0.5) * pitch + rng.uniform(-2, 2))
            r = (planes * rng.uniform(0.18, 0.25), pitch * rng.uniform(0.14, 0.2), pitch * rng.uniform(0.14, 0.2))
            nuclei[sum(((g - ci) / ri) ** 2 for g, ci, ri in zip((zz, yy, xx), c, r)) <= 1.0] = label
            near |= sum(((g - ci) / (ri + gi)) ** 2 for g, ci, ri, gi in zip((zz, yy, xx), c, r, (1.5, 4.0, 4.0))) <= 1.0
    base = rng.integers(200, 1200, size=nuclei.shape)
    pixels = np.stack([base + np.where(nuclei > 0, 9000, 0) + rng.integers(0, 3000, size=nuclei.shape),
                       base // 2 + np.where(near, 5000, 0) + rng.integers(0, 6000, size=nuclei.shape)]).astype(np.uint16)
    return pixels[None], nuclei


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--distance", type=int, default=4, help="N, in pixels")
    ap.add_argument("--isotropic", action="store_true", help="volume_secondary=True (unit spacing) instead of (13, 5)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    pixels, nuclei = synthetic_stack(args.planes, args.size)
    dP, prob = synth.analytic_flows_3d(nuclei)

    pipeline = build_pipeline_steps(
        channels_to_segment={"nuclei": 0},             # one network pass
        channels_to_extract=[0, 1],
        features_to_extract=("intensity",),
        volume_features=("intensity3d",),              # a 3-D segment step, volume_<obj> steps, profiles3d/
        secondary={"cell": ("nuclei", args.distance)},
        tertiary={"cytoplasm": ("cell", "nuclei")},
        relate=[("nuclei", "cell")],
        volume_relate=True,                            # the tertiary volume and the relate3d rows ...
        volume_secondary=True if args.isotropic else (13, 5),  # ... of the cell volume grown from the nuclei volume
    )
    print("pipeline steps:", list(pipeline["steps"]))
    print("volumesecondary_cell:", pipeline["steps"]["volumesecondary_cell"])
    pipeline["save"] = [*pipeline["save"], "volumesecondary_cell"]  # steps/position/volumesecondary_cell/<tp>.npz
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": pixels}  # an in-memory [T,C,Z,Y,X] image
    pipeline["steps"]["segment_nuclei"]["segmenter_kwargs"].update(volume_mode="flows3d", setup_params=dict(
        flows_override=lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda())))

    out = Path(args.out) if args.out else Path(mkdtemp(prefix="aliby_secondary_volumes_out_"))
    _, extras = run_pipeline_and_post(pipeline=pipeline, pipeline_name="position", output_path=out)
    table = extras["profiles3d"]
    print(f"profiles3d/position.parquet: {table.num_rows} rows x {len(table.column_names)} columns -> {out}")

    # rows by (object set, volume label): the three compartments of a nucleus share its label
    cols = ("metadata_object", "metadata_label", VOLUME, MEAN, "None/None/relate3d/Parent_cell")
    rows = {(r[0], r[1]): r for r in zip(*(table.column(c).to_pylist() for c in cols))}
    print("label | nucleus volume, mean ch1 | cell volume, mean ch1 | cytoplasm volume, mean ch1 | Parent_cell")
    for (obj, label), (_, _, volume, mean, parent) in rows.items():
        if obj != "nuclei":
            continue
        cell, cyto = rows[("cell", label)], rows.get(("cytoplasm", label))
        cyto_text = f"{cyto[2]:6.0f} {cyto[3]:8.1f}" if cyto else "   (none left)"
        print(f"  {label:3d} | {volume:6.0f} {mean:8.1f} | {cell[2]:6.0f} {cell[3]:8.1f} | {cyto_text} | {int(parent):3d}")


if __name__ == "__main__":
    main()
