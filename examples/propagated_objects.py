"""
Nuclei, cells and the cytoplasm of one position from ONE segmentation plus the cell stain, through the step API on one MI355X.

CellProfiler's IdentifySecondaryObjects, method "Propagation" (its default), grows a cell around every nucleus along the cell
channel: the nuclei are the seeds, grey-level differences in the stain make a step expensive (a membrane between two cells is where
they part), and a threshold on the stain says where the cells end.  One keyword of `build_pipeline_steps` adds it, and the tertiary
keyword takes the grown set as its outer one:

    build_pipeline_steps(channels_to_segment={"nuclei": 0}, ...,
                         propagate={"cell": ("nuclei", 1, {"threshold": 400})}, tertiary={"cytoplasm": ("cell", "nuclei")})

The stain is channel 1 of the tile's pixels, max-projected over Z.  The metric is an exact integer (sixteenths of a grey level, ties
to the smaller label: include/aliby_hip.h), so a tile carries the same bits whatever the batch; against CellProfiler's float64
priority queue the parity is unpinned.  Grown pixels carry the nucleus's label, so `nuclei`, `cell` and `cytoplasm` rows of
`profiles/<name>.parquet` join on `metadata_label` by construction.  Such a pipeline runs position by position through
`run_pipeline_and_post` (the batched `run_positions` refuses it).

With --auto nothing is hand-picked: the options become {"auto_threshold": {"classes": 3, "middle": "foreground"}} and every tile is
thresholded at its own three-class Otsu level (times --correction), computed on the device and read there by the propagation; the
step keeps the thresholds it chose, which the script prints.

Segmentation needs Cellpose weights; none are obtainable offline.  The script draws a synthetic field of view (nuclei, and a cell
stain in channel 1) and feeds the dynamics the analytic flow fields of its ground truth through `flows_override`.

    python examples/propagated_objects.py [--size 256] [--cells 12] [--percentile 60 | --auto [--correction 1.0]] [--distance 0] [--out DIR]
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
    ap.add_argument("--percentile", type=float, default=60.0, help="the threshold, as a percentile of the stain")
    ap.add_argument("--auto", action="store_true", help="an automatic threshold per tile (three-class Otsu) in place of the percentile")
    ap.add_argument("--correction", type=float, default=1.0, help="with --auto: the threshold correction factor")
    ap.add_argument("--distance", type=int, default=0, help="keep the cells within this many pixels of their nuclei (0: no bound)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from aliby_amd import synth
    from aliby_amd.pipe import init_step, run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    fov = synth.make_fov(2, 3, shape=(args.size, args.size), n_channels=2, n_target=args.cells)
    dP, prob = synth.analytic_flows(fov["nuclei"])
    if args.auto:
        options = {"auto_threshold": {"classes": 3, "middle": "foreground", "correction": args.correction}}
    else:
        options = {"threshold": int(np.percentile(fov["pixels"][1].max(axis=0), args.percentile))}
    if args.distance:
        options["distance"] = args.distance

    pipeline = build_pipeline_steps(
        channels_to_segment={"nuclei": 0},                  # one network pass
        channels_to_extract=[0, 1],
        features_to_extract=("intensity",),
        propagate={"cell": ("nuclei", 1, options)},         # name: (primary, stain channel, options)
        tertiary={"cytoplasm": ("cell", "nuclei")},         # name: (outer, inner)
    )
    print("pipeline steps:", list(pipeline["steps"]))
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": fov["pixels"][None]}  # an in-memory [T,C,Z,Y,X] image
    pipeline["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(
        flows_override=lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()))

    out = Path(args.out) if args.out else Path(mkdtemp(prefix="aliby_propagate_out_"))
    made = {}  # the step callables, by name: the propagate step keeps the thresholds of its last call

    def keep(name, parameters, other_steps=None):
        made[name] = init_step(name, parameters, other_steps)
        return made[name]

    profiles, _ = run_pipeline_and_post(pipeline=pipeline, pipeline_name="position", output_path=out, init_step_fn=keep)
    print("propagate_cell options:", pipeline["steps"]["propagate_cell"], "-> thresholds per tile:", made["propagate_cell"].thresholds)
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
