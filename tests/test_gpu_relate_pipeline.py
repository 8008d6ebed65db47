"""
One position through run_pipeline_and_post with the builder's `relate` and `tertiary` keywords (segmenters fed analytic flows through
flows_override, as the other pipeline tests do): the profile table carries nuclei, cell and cytoplasm rows, the cytoplasm rows join
the cell rows on the label, the relate columns equal tests/relate_ref.py on the saved masks, and without the keywords the table of
the same position is the one the untouched path builds.
"""
import numpy as np
import pyarrow.compute as pc
import pyarrow.parquet
import pytest

from tests import relate_ref as ref
from tests.test_gpu_relate import compare

pytestmark = pytest.mark.gpu

AREA = "None/None/sizeshape/Area"


def _saved(tmp_path, name, step):
    with np.load(tmp_path / "steps" / name / step / "0000.npz") as z:
        assert list(z.keys()) == ["arr_0"]
        return z["arr_0"]


def test_three_compartments_linked(tmp_path, engine):
    import torch
    from aliby_amd import synth
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    f = synth.make_fov(2, 7, shape=(192, 224), n_channels=2, n_target=12)
    flows = {k: synth.analytic_flows(f[k]) for k in ("nuclei", "cells")}

    def override_for(key):
        dP, prob = flows[key]
        return lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda())

    def pipeline(**kw):
        p = build_pipeline_steps(channels_to_segment={"nuclei": 0, "cell": 1}, channels_to_extract=[0, 1],
                                 features_to_extract=("intensity",), **kw)
        p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}  # T = 1
        p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override_for("nuclei"))
        p["steps"]["segment_cell"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override_for("cells"))
        return p

    full, extras = run_pipeline_and_post(pipeline=pipeline(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}),
                                         pipeline_name="full", output_path=tmp_path)
    plain, _ = run_pipeline_and_post(pipeline=pipeline(), pipeline_name="plain", output_path=tmp_path)
    assert extras == {}

    nuclei, cells = _saved(tmp_path, "full", "segment_nuclei"), _saved(tmp_path, "full", "segment_cell")
    assert np.array_equal(nuclei, _saved(tmp_path, "plain", "segment_nuclei")) and nuclei.max() > 3 and cells.max() > 3
    cyto = _saved(tmp_path, "full", "tertiary_cytoplasm")
    assert cyto.dtype == np.uint16 and np.array_equal(cyto, ref.tertiary(cells, nuclei, True))

    # three object sets, in the extract steps' order
    objects = full["metadata_object"].to_pylist()
    n_n, n_c, n_t = int(nuclei.max()), int(cells.max()), int(cyto.max())
    assert objects == ["nuclei"] * n_n + ["cell"] * n_c + ["cytoplasm"] * n_t
    rows = {o: full.filter(pc.equal(full["metadata_object"], o)) for o in ("nuclei", "cell", "cytoplasm")}

    # cytoplasm rows join cell rows on (tp, tile, label): the label is the cell's, the area what the nuclei left of it
    cell_area = dict(zip(rows["cell"]["metadata_label"].to_pylist(), rows["cell"][AREA].to_pylist()))
    for label, area, tile, tp in zip(*(rows["cytoplasm"][c].to_pylist() for c in ("metadata_label", AREA, "metadata_tile", "metadata_tp"))):
        assert label in cell_area and (tile, tp) == (0, 0)
        assert area == float((cyto == label).sum()) and 0 < area < cell_area[label] == float((cells == label).sum())

    # the relate columns against the restatement on the saved masks
    want_n, want_c = ref.relate(nuclei, cells)
    for obj, other, want in (("nuclei", "cell", want_n), ("cell", "nuclei", want_c)):
        keys = [f"None/None/relate/{n}" for n in ref.names(other)]
        got = np.stack([np.asarray(rows[obj][k].to_numpy(zero_copy_only=False), float) for k in keys], axis=1)
        assert rows[obj]["metadata_label"].to_pylist() == list(range(1, len(want) + 1))
        compare(got, want, f"pipeline {obj}")
        assert all(rows["cytoplasm"][k].null_count == rows["cytoplasm"].num_rows for k in keys)  # no relation: nulls
        foreign = [f"None/None/relate/{n}" for n in ref.names(obj)]
        assert all(rows[obj][k].null_count == rows[obj].num_rows for k in foreign)
    parent = rows["nuclei"]["None/None/relate/Parent_cell"].to_numpy(zero_copy_only=False)
    assert (parent > 0).all() and set(parent.astype(int)) <= set(cell_area)  # every nucleus of this scene lies in a cell

    # the file holds the same table
    on_disk = pyarrow.parquet.read_table(tmp_path / "profiles" / "full.parquet")
    assert on_disk.num_rows == full.num_rows and set(on_disk.column_names) == set(full.column_names)
    assert on_disk["None/None/relate/Parent_cell"].to_pylist() == full["None/None/relate/Parent_cell"].to_pylist()

    # without the keywords: the table of the untouched path, and the rows and columns it shares with the full one are equal
    assert set(plain["metadata_object"].to_pylist()) == {"nuclei", "cell"}
    assert not any("/relate/" in c for c in plain.column_names)
    shared = full.filter(pc.is_in(full["metadata_object"], value_set=pyarrow.array(["nuclei", "cell"]))).select(plain.column_names)
    assert shared.schema.equals(plain.schema) and shared.num_rows == plain.num_rows
    for name in plain.column_names:  # (Table.equals holds a NaN unequal to itself: float columns are compared by their bits)
        a, b = shared[name].combine_chunks(), plain[name].combine_chunks()
        if pyarrow.types.is_float64(a.type):
            assert a.null_count == b.null_count == 0
            assert np.array_equal(a.to_numpy().view(np.int64), b.to_numpy().view(np.int64)), name  # the same bits
        else:
            assert a.equals(b), name
