"""
Nuclei, cells and the cytoplasm of one position from ONE segmentation, through the step API on one MI355X.

Where only the nuclear channel segments well, CellProfiler's IdentifySecondaryObjects grows a cell around every nucleus; its
"Distance - N" method needs no second stain and no second network pass.  One keyword of `build_pipeline_steps` adds it, and the
tertiary keyword takes the grown set as its outer one:

    build_pipeline_steps(channels_to_segment={"nuclei": 0}, ...,
                         secondary={"cell": ("nuclei", 10)}, tertiary={"cytoplasm": ("cell", "nuclei")})

A grown pixel takes the label of the nearest nucleus pixel (exact integer distances, ties to the smaller label: scipy's
distance_transform_edt index gather, which is what CellProfiler runs, except on exact ties), so `nuclei`, `cell` and `cytoplasm`
rows of `profiles/<name>.parquet` join on `metadata_label` by construction, with no parent search.  Such a pipeline runs position by
position through `run_pipeline_and_post` (the batched `run_positions` refuses it).

Segmentation needs Cellpose weights; none are obtainable offline.  The script draws a synthetic field of view and feeds the
dynamics the analytic flow fields of its ground truth through `flows_override`.

    python examples/secondary_objects.py [--size 256] [--cells 12] [--distance 10] [--out DIR]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path
from tempfile import mkdtemp

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

AREA, MEAN = "None/None/sizeshape/Area", "1/max/intensity/Intensity_MeanIntensity"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cells", type=int, default=12)
    ap.add_argument("--distance", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    fov = synth.make_fov(2, 3, shape=(args.size, args.size), n_channels=2, n_target=args.cells)
    dP, prob = synth.analytic_flows(fov["nuclei"])

    pipeline = build_pipeline_steps(
        channels_to_segment={"nuclei": 0},                  # one network pass
        channels_to_extract=[0, 1],
        features_to_extract=("intensity",),
        secondary={"cell": ("nuclei", args.distance)},      # name: (primary, N pixels)
        tertiary={"cytoplasm": ("cell", "nuclei")},         # name: (outer, inner)
    )
    print("pipeline steps:", list(pipeline["steps"]))
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": fov["pixels"][None]}  # an in-memory [T,C,Z,Y,X] image
    pipeline["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(
        flows_override=lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()))

    out = Path(args.out) if args.out else Path(mkdtemp(prefix="aliby_secondary_out_"))
    profiles, _ = run_pipeline_and_post(pipeline=pipeline, pipeline_name="position", output_path=out)
    print(f"profiles/position.parquet: {profiles.num_rows} rows x {len(profiles.column_names)} columns -> {out}")
    print("saved masks:", sorted(p.name for p in (out / "steps" / "position").iterdir()))

    # rows by (object set, label): the three compartments of one object share its label
    cols = ("metadata_object", "metadata_label", AREA, MEAN)
    rows = {(r[0], r[1]): r for r in zip(*(profiles.column(c).to_pylist() for c in cols))}
    print("label | nucleus area, mean ch1 | cell area, mean ch1 | cytoplasm area, mean ch1")
    for (obj, label), (_, _, area, mean) in rows.items():
        if obj != "nuclei":
            continue
        cell, cyto = rows[("cell", label)], rows.get(("cytoplasm", label))
        cyto_text = f"{cyto[2]:6.0f} {cyto[3]:8.1f}" if cyto else "   (none left)"
        print(f"  {label:3d} | {area:6.0f} {mean:8.1f} | {cell[2]:6.0f} {cell[3]:8.1f} | {cyto_text}")


if __name__ == "__main__":
    main()
