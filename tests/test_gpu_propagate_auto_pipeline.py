"""
One position of two tiles through run_pipeline_and_post with the builder's `propagate` keyword and nothing hand-tuned:
propagate={"cell": ("nuclei", channel, {"auto_threshold": {"classes": 3}})} and a tertiary cytoplasm (the crop tiler cuts a 128 x 256
frame into two tiles; the segmenter is fed analytic flows per tile through flows_override, as the other pipeline tests do).  The saved
cell masks of each tile are the restatement (tests/propagate_ref.py) of the saved nuclei masks and the tile's max-projected cell channel
at the threshold tests/threshold_ref.py gives for that tile, the step's `thresholds` are those values, and the profile carries
nuclei, cell and cytoplasm rows per tile that join on the label.
"""
import numpy as np
import pyarrow.compute as pc
import pytest

from tests import propagate_ref as ref
from tests import relate_ref, threshold_ref

pytestmark = pytest.mark.gpu

AREA = "None/None/sizeshape/Area"
CHANNEL = 1
TS = 128


def _saved(tmp_path, name, step):
    with np.load(tmp_path / "steps" / name / step / "0000.npz") as z:
        assert list(z.keys()) == ["arr_0"]
        return z["arr_0"]


def _relabel(labels):
    uniq = np.unique(labels)
    uniq = uniq[uniq != 0]
    fwd = np.zeros(int(labels.max()) + 1, labels.dtype)
    fwd[uniq] = np.arange(1, len(uniq) + 1)
    return fwd[labels]


def test_three_compartments_at_automatic_thresholds(tmp_path, engine):
    import torch
    from aliby_amd import pipe, synth
    from aliby_amd.pipe_builder import build_pipeline_steps

    f = synth.make_fov(2, 7, shape=(TS, 2 * TS), n_channels=2, n_target=14)
    pixels = f["pixels"].copy()
    pixels[CHANNEL, :, :, TS:] = pixels[CHANNEL, :, :, TS:] // 2 + 900  # the right tile: another background, another brightness
    flows = [synth.analytic_flows(_relabel(f["nuclei"][:, k * TS:(k + 1) * TS])) for k in range(2)]

    def override(x):
        assert x.shape[0] == 2  # the two tiles, left then right
        return (torch.from_numpy(np.stack([dP for dP, _ in flows])).cuda(), torch.from_numpy(np.stack([prob for _, prob in flows])).cuda())

    p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("intensity",),
                             propagate={"cell": ("nuclei", CHANNEL, {"auto_threshold": {"classes": 3}})},
                             tertiary={"cytoplasm": ("cell", "nuclei")})
    assert p["steps"]["propagate_cell"] == {"channel": CHANNEL, "auto_threshold": {"classes": 3}}
    p["steps"]["tile"] = {"kind": "crop", "tile_size": TS, "standard_scale": False, "image_kwargs": {"source": pixels[None]}}  # T = 1
    p["steps"]["segment_nuclei"]["segmenter_kwargs"].update(per_tile=True, setup_params=dict(flows_override=override))

    made = {}

    def init_step(name, parameters, other_steps=None):
        made[name] = pipe.init_step(name, parameters, other_steps)
        return made[name]

    table, extras = pipe.run_pipeline_and_post(pipeline=p, pipeline_name="pos", output_path=tmp_path, init_step_fn=init_step)
    assert extras == {}

    nuclei = _saved(tmp_path, "pos", "segment_nuclei")
    cells = _saved(tmp_path, "pos", "propagate_cell")
    cyto = _saved(tmp_path, "pos", "tertiary_cytoplasm")
    assert nuclei.shape == cells.shape == cyto.shape == (2, TS, TS) and cells.dtype == np.uint16 and cyto.dtype == np.uint16
    stains = np.stack([pixels[CHANNEL, :, :, k * TS:(k + 1) * TS].max(axis=0) for k in range(2)])  # what the "max" reducer measures
    thresholds = threshold_ref.otsu_batch(stains, classes=3)[0]
    assert thresholds[0] != thresholds[1]
    assert made["propagate_cell"].thresholds == thresholds.tolist()
    for k in range(2):
        assert nuclei[k].max() > 2
        want = ref.propagate_labels(nuclei[k:k + 1], stains[k:k + 1], threshold=int(thresholds[k]))[0][0]
        assert np.array_equal(cells[k], want), k
        assert (cells[k] != 0).sum() > (nuclei[k] != 0).sum() and (cells[k] == 0).any()
        assert np.array_equal(cyto[k], relate_ref.tertiary(cells[k], nuclei[k], True))

    # three object sets per tile; the derived ones carry the nuclei's labels
    for k in range(2):
        rows = {o: table.filter(pc.and_(pc.equal(table["metadata_object"], o), pc.equal(table["metadata_tile"], k)))
                for o in ("nuclei", "cell", "cytoplasm")}
        labels = {o: rows[o]["metadata_label"].to_pylist() for o in rows}
        assert labels["nuclei"] == list(range(1, int(nuclei[k].max()) + 1))
        assert labels["cell"] == labels["nuclei"]  # labelled pixels keep their label: growing loses no object
        assert labels["cytoplasm"] and set(labels["cytoplasm"]) <= set(labels["nuclei"])
        area = {o: dict(zip(labels[o], rows[o][AREA].to_pylist())) for o in rows}
        for label in labels["cytoplasm"]:
            assert area["cell"][label] == float((cells[k] == label).sum()) > area["nuclei"][label] == float((nuclei[k] == label).sum())
            assert area["cytoplasm"][label] == float((cyto[k] == label).sum()) < area["cell"][label]
