"""
Nuclei, cells and the cytoplasm of one Z-stack, linked in 3-D, through the step API on one MI355X.

`volume_features` makes the segment steps segment the stack as a volume and writes one row per volume object to
`profiles3d/<name>.parquet`; `relate` and `tertiary` alone would link only the collapsed 2-D masks, where every nucleus hides the
cytoplasm above and below it.  One more keyword takes both to the volume labels (CellProfiler's RelateObjects and
IdentifyTertiaryObjects on volumes; parity with CellProfiler is unpinned, include/aliby_hip.h):

    build_pipeline_steps(..., volume_features=("intensity3d",), relate=[("nuclei", "cell")],
                         tertiary={"cytoplasm": ("cell", "nuclei")}, volume_relate=True)

`profiles3d/` then has nuclei, cell and cytoplasm rows: `None/None/relate3d/Parent_cell`, ... on the nuclei rows, `..._nuclei` on the
cell rows, and the cytoplasm (the cell's volume minus its nuclei, plane by plane) under the cell's volume label.  Such a pipeline runs
position by position through `run_pipeline_and_post` (the batched `run_positions` refuses it).

Segmentation needs Cellpose weights; none are obtainable offline.  The script draws a synthetic two-channel stack, ellipsoid nuclei
inside ellipsoid cells, and feeds the 3-D dynamics the analytic flow fields of its ground truth through `flows_override`.

    python examples/related_volumes.py [--planes 8] [--size 96] [--out DIR]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path
from tempfile import mkdtemp

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

VOLUME, MEAN = "None/None/sizeshape3d/Volume", "0/None/intensity3d/Intensity_MeanIntensity"


def synthetic_stack(planes: int, size: int, seed: int = 7):
    """-> (pixels uint16 [T=1,C=2,Z,Y,X], nuclei uint16 [Z,Y,X], cells uint16 [Z,Y,X]): a 3 x 3 grid of ellipsoids."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.mgrid[0:planes, 0:size, 0:size]
    nuclei, cells = np.zeros((planes, size, size), np.uint16), np.zeros((planes, size, size), np.uint16)
    pitch = size / 3.0
    label = 0
    for gy in range(3):
        for gx in range(3):
            label += 1
            c = (planes / 2.0 + rng.uniform(-0.5, 0.5), (gy + 0.5) * pitch + rng.uniform(-2, 2), (gx + 0.5) * pitch + rng.uniform(-2, 2))
            r = (planes * rng.uniform(0.18, 0.25), pitch * rng.uniform(0.14, 0.2), pitch * rng.uniform(0.14, 0.2))
            for vol, grow in ((cells, (planes * 0.15, pitch * 0.2, pitch * 0.2)), (nuclei, (0.0, 0.0, 0.0))):
                vol[sum(((g - ci) / (ri + gi)) ** 2 for g, ci, ri, gi in zip((zz, yy, xx), c, r, grow)) <= 1.0] = label
    base = rng.integers(200, 1200, size=nuclei.shape)
    pixels = np.stack([base + np.where(nuclei > 0, 9000, 0) + np.where(cells > 0, 1500, 0) + rng.integers(0, 3000, size=nuclei.shape),
                       base // 2 + np.where(cells > 0, 5000, 0) + rng.integers(0, 6000, size=nuclei.shape)]).astype(np.uint16)
    return pixels[None], nuclei, cells


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    pixels, nuclei, cells = synthetic_stack(args.planes, args.size)
    flows = {"nuclei": synth.analytic_flows_3d(nuclei), "cell": synth.analytic_flows_3d(cells)}

    pipeline = build_pipeline_steps(
        channels_to_segment={"nuclei": 0, "cell": 1},
        channels_to_extract=[0, 1],
        features_to_extract=("intensity",),
        volume_features=("intensity3d",),              # 3-D segment steps, volume_<obj> steps, profiles3d/
        relate=[("nuclei", "cell")],
        tertiary={"cytoplasm": ("cell", "nuclei")},
        volume_relate=True,                            # ... and both of them on the volume labels
    )
    print("pipeline steps:", list(pipeline["steps"]))
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": pixels}  # an in-memory [T,C,Z,Y,X] image
    for obj, (dP, prob) in flows.items():
        pipeline["steps"][f"segment_{obj}"]["segmenter_kwargs"].update(volume_mode="flows3d", setup_params=dict(
            flows_override=lambda x, dP=dP, prob=prob: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda())))

    out = Path(args.out) if args.out else Path(mkdtemp(prefix="aliby_related_volumes_out_"))
    _, extras = run_pipeline_and_post(pipeline=pipeline, pipeline_name="position", output_path=out)
    table = extras["profiles3d"]
    print(f"profiles3d/position.parquet: {table.num_rows} rows x {len(table.column_names)} columns -> {out}")

    # rows by (object set, volume label): a nucleus finds its cell through Parent_cell, the cytoplasm shares the cell's label
    cols = ("metadata_object", "metadata_label", VOLUME, MEAN, "None/None/relate3d/Parent_cell", "None/None/relate3d/Distance_Centroid_cell",
            "None/None/relate3d/Distance_Minimum_cell", "None/None/relate3d/Children_nuclei_Count")
    rows = {(r[0], r[1]): r for r in zip(*(table.column(c).to_pylist() for c in cols))}
    print("nucleus -> cell | nucleus volume, mean ch0 | cell volume, nuclei in it | cytoplasm volume, mean ch0 | centre, outline distance")
    for (obj, label), (_, _, volume, mean, parent, dist, dmin, _) in rows.items():
        if obj != "nuclei":
            continue
        if not parent:
            print(f"  {label:3d} ->  no cell | {volume:6.0f} {mean:8.1f}")
            continue
        cell, cyto = rows[("cell", int(parent))], rows.get(("cytoplasm", int(parent)))
        cyto_text = f"{cyto[2]:6.0f} {cyto[3]:8.1f}" if cyto else "   (none left)"
        print(f"  {label:3d} -> {int(parent):3d}     | {volume:6.0f} {mean:8.1f} | {cell[2]:6.0f} {int(cell[7]):2d} | {cyto_text} | {dist:6.2f} {dmin:6.2f}")


if __name__ == "__main__":
    main()
