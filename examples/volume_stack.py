"""
A Z-stack measured twice through the step API on one MI355X: as the reference measures it — the 3-D segmentation collapsed to 2-D
(maximum over z, sequential relabel), features on the z-projected pixels, `profiles/<name>.parquet` — and as a volume — the 3-D
labels kept on the device, the volume families over them, `profiles3d/<name>.parquet`.  The two tables join on
(metadata_tp, metadata_tile, metadata_object, Projection_Label = metadata_label): `Projection_Label` is the label a volume object
carries in the collapsed image, 0 when it is hidden under other objects everywhere.

The switch is two keywords of `build_pipeline_steps`:

    build_pipeline_steps(..., volume_features=("intensity3d", "intensity3d_detail"), volume_coloc=True)

which sets `do_3D=True` on every segment step and adds a `volume_<obj>` step per object set.  Such a pipeline runs position by
position through `run_pipeline_and_post` (the batched `run_positions` has no volume form and refuses it).

Segmentation needs Cellpose weights; none are obtainable offline.  The script writes a synthetic stack of ellipsoids, two of them
stacked in z so that the collapse hides part of one, and feeds cellpose's 3-D dynamics (`volume_mode="flows3d"`) the analytic 3-D
flow field of that ground truth through `flows_override`.

    python examples/volume_stack.py [--size 128] [--planes 12] [--out DIR]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path
from tempfile import mkdtemp

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def synthetic_stack(size: int, planes: int, seed: int = 0):
    """-> (pixels uint16 [T=1, C=2, Z, Y, X], ground-truth volume labels uint16 [Z, Y, X]): a grid of ellipsoids in the lower half
    of the stack, and one more above the first of them."""
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.mgrid[0:planes, 0:size, 0:size]
    labels = np.zeros((planes, size, size), np.uint16)

    def paint(label, centre, radii):
        labels[sum(((g - c) / r) ** 2 for g, c, r in zip((zz, yy, xx), centre, radii)) <= 1.0] = label

    step, label = size // 3, 0
    for cy in range(step // 2, size, step):
        for cx in range(step // 2, size, step):
            label += 1
            paint(label, (planes * 0.3, cy + rng.uniform(-3, 3), cx + rng.uniform(-3, 3)),
                  (planes * 0.2, step * rng.uniform(0.25, 0.38), step * rng.uniform(0.25, 0.38)))
    paint(label + 1, (planes * 0.8, step // 2 + 4, step // 2 + 6), (planes * 0.15, step * 0.3, step * 0.3))  # above object 1
    glow = np.where(labels > 0, 3000 + 500 * labels.astype(np.int64), 0)
    pixels = np.stack([400 + glow + rng.integers(0, 2000, labels.shape), 300 + glow // 2 + rng.integers(0, 4000, labels.shape)])
    return pixels.astype(np.uint16)[None], labels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--planes", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import pyarrow.parquet
    import torch

    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    pixels, truth = synthetic_stack(args.size, args.planes)
    dP, prob = synth.analytic_flows_3d(truth)

    pipeline = build_pipeline_steps(
        channels_to_segment={"nuclei": 0},
        channels_to_extract=[0, 1],
        features_to_extract=("intensity",),
        volume_features=("intensity3d", "intensity3d_detail"),   # the two lines that make the position a volume
        volume_coloc=True,
    )
    print("pipeline steps:", list(pipeline["steps"]))
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": pixels}  # an in-memory [T,C,Z,Y,X] image
    pipeline["steps"]["segment_nuclei"]["segmenter_kwargs"].update(
        volume_mode="flows3d",  # cellpose's own 3-D mode; the default, "stitch", segments the planes and stitches them along z
        setup_params=dict(flows_override=lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda())))

    out = Path(args.out) if args.out else Path(mkdtemp(prefix="aliby_volume_out_"))
    profiles, post = run_pipeline_and_post(pipeline=pipeline, pipeline_name="stack", output_path=out)
    profiles3d = post["profiles3d"]
    for sub in ("profiles", "profiles3d"):
        table = pyarrow.parquet.read_table(out / sub / "stack.parquet")
        print(f"{sub}/stack.parquet: {table.num_rows} rows x {len(table.column_names)} columns")

    # the two tables side by side: a volume row finds its 2-D row through Projection_Label
    flat = {label: k for k, label in enumerate(profiles.column("metadata_label").to_pylist())}
    mean2d = profiles.column("0/max/intensity/Intensity_MeanIntensity").to_pylist()
    cols = {c: profiles3d.column(c).to_pylist() for c in (
        "metadata_label", "None/None/projection3d/Projection_Label", "None/None/projection3d/Projection_VisibleFraction",
        "None/None/sizeshape3d/Volume", "0/None/intensity3d/Intensity_MeanIntensity")}
    print("volume label -> label in the collapse, visible fraction, volume, mean intensity 3-D | 2-D (of the z-maximum)")
    for label, key, frac, volume, mean3d in zip(*cols.values()):
        flat_mean = f"{mean2d[flat[int(key)]]:9.1f}" if key else "   hidden"
        print(f"  {label:3d} -> {int(key):3d}   {frac:5.2f}   {volume:8.0f}   {mean3d:9.1f} | {flat_mean}")
    assert sorted(int(k) for k in cols["None/None/projection3d/Projection_Label"] if k) == sorted(flat)
    print(f"{profiles3d.num_rows} volume objects, {profiles.num_rows} objects in the collapse -> {out}")


if __name__ == "__main__":
    main()
