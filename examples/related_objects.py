"""
Nuclei, cells and the cytoplasm of one position, linked, through the step API on one MI355X.

The two segment steps of the default pipeline are independent runs: their labels have nothing to do with each other, so the
`nuclei` and `cell` rows of `profiles/<name>.parquet` share no key.  Two keywords of `build_pipeline_steps` close the gap
(CellProfiler's RelateObjects and IdentifyTertiaryObjects; parity with CellProfiler is unpinned, include/aliby_hip.h):

    build_pipeline_steps(..., relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")})

`relate` adds `None/None/relate/Parent_cell`, ... to the nuclei rows and `..._nuclei` to the cell rows; `tertiary` adds a third object
set, the cell minus its nuclei, under the cell's labels.  Such a pipeline runs position by position through `run_pipeline_and_post`
(the batched `run_positions` refuses it).

Segmentation needs Cellpose weights; none are obtainable offline.  The script draws a synthetic field of view and feeds the
dynamics the analytic flow fields of its ground truth through `flows_override`.

    python examples/related_objects.py [--size 256] [--cells 12] [--out DIR]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path
from tempfile import mkdtemp

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

AREA, MEAN = "None/None/sizeshape/Area", "0/max/intensity/Intensity_MeanIntensity"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cells", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    fov = synth.make_fov(2, 3, shape=(args.size, args.size), n_channels=2, n_target=args.cells)
    flows = {"nuclei": synth.analytic_flows(fov["nuclei"]), "cell": synth.analytic_flows(fov["cells"])}

    pipeline = build_pipeline_steps(
        channels_to_segment={"nuclei": 0, "cell": 1},
        channels_to_extract=[0, 1],
        features_to_extract=("intensity",),
        relate=[("nuclei", "cell")],                   # the two lines that link the object sets
        tertiary={"cytoplasm": ("cell", "nuclei")},    # name: (outer, inner)
    )
    print("pipeline steps:", list(pipeline["steps"]))
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": fov["pixels"][None]}  # an in-memory [T,C,Z,Y,X] image
    for obj, (dP, prob) in flows.items():
        pipeline["steps"][f"segment_{obj}"]["segmenter_kwargs"]["setup_params"] = dict(
            flows_override=lambda x, dP=dP, prob=prob: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()))

    out = Path(args.out) if args.out else Path(mkdtemp(prefix="aliby_related_out_"))
    profiles, _ = run_pipeline_and_post(pipeline=pipeline, pipeline_name="position", output_path=out)
    print(f"profiles/position.parquet: {profiles.num_rows} rows x {len(profiles.column_names)} columns -> {out}")

    # rows by (object set, label): a nucleus finds its cell through Parent_cell, the cytoplasm shares the cell's label
    cols = ("metadata_object", "metadata_label", AREA, MEAN, "None/None/relate/Parent_cell", "None/None/relate/Distance_Centroid_cell",
            "None/None/relate/Children_nuclei_Count")
    rows = {(r[0], r[1]): r for r in zip(*(profiles.column(c).to_pylist() for c in cols))}
    print("nucleus -> cell | nucleus area, mean ch0 | cell area, nuclei in it | cytoplasm area, mean ch0 | centre distance")
    for (obj, label), (_, _, area, mean, parent, dist, _) in rows.items():
        if obj != "nuclei":
            continue
        if not parent:
            print(f"  {label:3d} ->  no cell | {area:6.0f} {mean:8.1f}")
            continue
        cell, cyto = rows[("cell", int(parent))], rows.get(("cytoplasm", int(parent)))
        cyto_text = f"{cyto[2]:6.0f} {cyto[3]:8.1f}" if cyto else "   (none left)"
        print(f"  {label:3d} -> {int(parent):3d}     | {area:6.0f} {mean:8.1f} | {cell[2]:6.0f} {int(cell[6]):2d} | {cyto_text} | {dist:6.2f}")


if __name__ == "__main__":
    main()
