"""
One position through run_pipeline_and_post with the builder's `propagate` and `tertiary` keywords and ONE segmented object set (the
segmenter fed analytic flows through flows_override, as the other pipeline tests do): the saved cell masks are the restatement
(tests/propagate_ref.py) of the saved nuclei masks and the max-projected cell channel, the cytoplasm is tests/relate_ref.py's tertiary
image of the two, and the profile carries nuclei, cell and cytoplasm rows that join on the label.
"""
import numpy as np
import pyarrow.compute as pc
import pytest

from tests import propagate_ref as ref
from tests import relate_ref

pytestmark = pytest.mark.gpu

AREA = "None/None/sizeshape/Area"
CHANNEL = 1


def _saved(tmp_path, name, step):
    with np.load(tmp_path / "steps" / name / step / "0000.npz") as z:
        assert list(z.keys()) == ["arr_0"]
        return z["arr_0"]


def test_three_compartments_along_a_stain(tmp_path, engine):
    import torch
    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    f = synth.make_fov(2, 7, shape=(192, 224), n_channels=2, n_target=12)
    dP, prob = synth.analytic_flows(f["nuclei"])
    stain = f["pixels"][CHANNEL].max(axis=0)  # [Y,X]: what the "max" reducer measures
    options = {"threshold": int(np.percentile(stain, 60)), "distance": 20}
    p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("intensity",),
                             propagate={"cell": ("nuclei", CHANNEL, options)}, tertiary={"cytoplasm": ("cell", "nuclei")})
    p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}  # T = 1
    p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(
        flows_override=lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()))
    table, extras = run_pipeline_and_post(pipeline=p, pipeline_name="pos", output_path=tmp_path)
    assert extras == {}

    nuclei = _saved(tmp_path, "pos", "segment_nuclei")
    cells = _saved(tmp_path, "pos", "propagate_cell")
    cyto = _saved(tmp_path, "pos", "tertiary_cytoplasm")
    assert nuclei.max() > 3 and cells.dtype == np.uint16 and cells.shape == nuclei.shape
    tiles = nuclei.reshape(-1, *nuclei.shape[-2:])
    assert tiles.shape[0] == 1  # one tile: the whole field of view
    want_cells = ref.propagate_labels(tiles, stain[None], **options)[0].reshape(nuclei.shape)
    assert np.array_equal(cells, want_cells)
    assert (cells != 0).sum() > (nuclei != 0).sum() and (cells == 0).any()
    assert cyto.dtype == np.uint16 and np.array_equal(cyto, relate_ref.tertiary(cells, nuclei, True))

    # three object sets, in the extract steps' order; the derived ones carry the nuclei's labels
    rows = {o: table.filter(pc.equal(table["metadata_object"], o)) for o in ("nuclei", "cell", "cytoplasm")}
    assert table["metadata_object"].to_pylist() == [o for o in ("nuclei", "cell", "cytoplasm") for _ in range(rows[o].num_rows)]
    labels = {o: rows[o]["metadata_label"].to_pylist() for o in rows}
    assert labels["nuclei"] == list(range(1, int(nuclei.max()) + 1))
    assert labels["cell"] == labels["nuclei"]  # labelled pixels keep their label: growing loses no object
    assert labels["cytoplasm"] and set(labels["cytoplasm"]) <= set(labels["nuclei"])
    area = {o: dict(zip(labels[o], rows[o][AREA].to_pylist())) for o in rows}
    for label in labels["cytoplasm"]:
        assert area["cell"][label] == float((cells == label).sum()) > area["nuclei"][label] == float((nuclei == label).sum())
        assert area["cytoplasm"][label] == float((cyto == label).sum()) < area["cell"][label]
