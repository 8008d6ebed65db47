"""
tests/relate_ref.py, the NumPy restatement of the `relate` family and the tertiary image, pinned to the hand values of the worked
example in include/aliby_hip.h and to an independent formulation (a pair histogram from np.bincount, scipy.ndimage.center_of_mass, a
brute-force outline); then the surface that needs no device: the column names and their refusals, the builder's dicts, the step
initialisers' errors, the run_positions refusal and the profile table's pivot of `extractrelate` steps.  Parity with CellProfiler is
unpinned (it cannot be run here).
"""
import numpy as np
import pyarrow as pa
import pytest

from tests import relate_ref as ref


# ------------------------------------------------------------------------------------------------ the restatement
def test_worked_example_hand_values():
    a, b = ref.worked()
    rows_a, rows_b = ref.relate(a, b)
    assert rows_a.shape == (3, 5) and rows_b.shape == (2, 5)
    assert np.array_equal(rows_a[:, :3], ref.WORKED_NUCLEI[:, :3])
    np.testing.assert_allclose(rows_a[:, 3:], ref.WORKED_NUCLEI[:, 3:], rtol=ref.RTOL, atol=ref.ATOL)
    assert np.array_equal(rows_b[:, :3], ref.WORKED_CELLS)
    # cell 1 holds nuclei 1 (centre (1.5, 1.5)) as its parent: centre (2.5, 1.5) -> 1; cell 2's parent is nucleus 2 at (3.5, 3.5)
    np.testing.assert_allclose(rows_b[:, 3], [1.0, np.sqrt(1.0 + 4.0)], rtol=ref.RTOL, atol=ref.ATOL)
    for shrink, areas in ref.WORKED_TERTIARY_AREAS.items():
        t = ref.tertiary(b, a, shrink_inner=shrink)
        assert t.dtype == np.uint16 and (int((t == 1).sum()), int((t == 2).sum())) == areas
        assert np.array_equal(t[t > 0], b[t > 0])  # it keeps the outer labels


def test_three_by_three_nucleus_loses_its_interior_pixel():
    outer, inner = ref.tertiary_scenes()["three_by_three_w16"]
    shrunk, plain = ref.tertiary(outer, inner, True), ref.tertiary(outer, inner, False)
    assert int((plain == 1).sum()) == 49 - 9 and int((shrunk == 1).sum()) == 49 - 1 and shrunk[4, 4] == 0
    assert not (shrunk == 2).any() and not (plain == 2).any()  # the cell under the large nucleus is left empty


def _brute_outline(lab):
    Y, X = lab.shape
    out = np.zeros(lab.shape, bool)
    for y in range(Y):
        for x in range(X):
            if lab[y, x] == 0:
                continue
            if y in (0, Y - 1) or x in (0, X - 1):
                out[y, x] = True
                continue
            out[y, x] = any(lab[y + dy, x + dx] != lab[y, x] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
    return out


def _independent(a, b, na, nb):
    """Rows of A relative to B from a pair histogram, scipy's centres and the brute-force outline."""
    from scipy import ndimage

    a, b = a.astype(np.int64), b.astype(np.int64)
    hist = np.bincount((a * (nb + 1) + b).ravel(), minlength=(na + 1) * (nb + 1)).reshape(na + 1, nb + 1)[1:, 1:]  # [na, nb]
    out = np.full((na, 5), np.nan)
    has = hist.max(axis=1) > 0 if nb else np.zeros(na, bool)
    parent = np.where(has, hist.argmax(axis=1) + 1, 0) if nb else np.zeros(na, np.int64)
    out[:, 0] = parent
    out[:, 1] = hist.max(axis=1) if nb else 0
    back = hist.T  # [nb, na]
    back_parent = np.where(back.max(axis=1) > 0, back.argmax(axis=1) + 1, 0) if na and nb else np.zeros(nb, np.int64)
    out[:, 2] = [(back_parent == L).sum() for L in range(1, na + 1)]
    edge = _brute_outline(b)
    for L in range(1, na + 1):
        p = int(parent[L - 1])
        if p == 0:
            continue
        cy, cx = ndimage.center_of_mass(a == L)
        py, px = ndimage.center_of_mass(b == p)
        out[L - 1, 3] = np.hypot(py - cy, px - cx)
        ys, xs = np.nonzero(edge & (b == p))
        out[L - 1, 4] = np.hypot(ys - cy, xs - cx).min()
    return out


@pytest.mark.parametrize("name", [*ref.scenes(), "strip"])
def test_independent_formulation(name):
    a, b, na, nb = ref.scenes()[name] if name != "strip" else (*ref.strip(), 2, 259)
    rows_a, rows_b = ref.relate(a, b, na, nb)
    for got, want in ((rows_a, _independent(a, b, na, nb)), (rows_b, _independent(b, a, nb, na))):
        assert np.array_equal(got[:, :3], want[:, :3])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got[:, 3:], want[:, 3:], rtol=1e-12, atol=1e-12)
    assert np.array_equal(ref.outline(b), _brute_outline(b)) and np.array_equal(ref.outline(a), _brute_outline(a))


def test_strip_ties_go_to_the_smallest_label():
    a, b = ref.strip()
    rows_a, rows_b = ref.relate(a, b)
    assert rows_a[0, :2].tolist() == [258.0, 21.0] and rows_a[1, :2].tolist() == [1.0, 1.0]
    assert rows_b[:, 0].tolist() == [1.0] * 259 and rows_a[:, 2].tolist() == [259.0, 0.0]


def test_absent_rows_and_tables_longer_than_the_labels():
    a, b, na, nb = ref.scenes()["absent"]
    rows_a, rows_b = ref.relate(a, b, na, nb)
    for rows, lab in ((rows_a, a), (rows_b, b)):
        for L in range(1, len(rows) + 1):
            if not (lab == L).any():
                assert rows[L - 1, :3].tolist() == [0, 0, 0] and np.isnan(rows[L - 1, 3:]).all()


def test_single_pixel_parents_scene():
    a, many, few, old = ref.single_pixel_parents()
    assert int(many.max()) == 65534 and int(few.max()) == len(old) and (many > 0).sum() == 65534
    assert np.array_equal(old[few[few > 0].astype(np.int64) - 1], many[few > 0])


# ------------------------------------------------------------------------------------------------ surface without a device
def test_relate_names_and_refusals():
    from aliby_amd.extraction import features

    assert features.relate_names("cell") == ["Parent_cell", "ParentOverlap_cell", "Children_cell_Count", "Distance_Centroid_cell",
                                             "Distance_Minimum_cell"] == ref.names("cell")
    for bad in ("", "my_cell", "a/b", None, 3):
        with pytest.raises(ValueError):
            features.relate_names(bad)


def test_header_declares_the_entries():
    from aliby_amd import _lib

    for name in ("aliby_features_relate", "aliby_tertiary_labels", "aliby_relate_workspace_bytes"):
        assert name in _lib.exported_symbols()


def test_builder_unchanged_without_the_keywords():
    from aliby_amd.pipe_builder import build_pipeline_steps

    plain = build_pipeline_steps()
    assert build_pipeline_steps(relate=None, tertiary=None) == plain
    assert list(plain["steps"]) == ["tile", "segment_nuclei", "segment_cell", "extract_nuclei", "extract_cell", "extractmulti_nuclei",
                                    "extractmulti_cell"]
    assert plain["save"] == ["segment_nuclei", "segment_cell"]
    assert not any(k.startswith(("tertiary", "extractrelate")) for k in plain["passed_data"])


def test_builder_with_the_keywords():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")})
    assert list(p["steps"]) == ["tile", "segment_nuclei", "segment_cell", "tertiary_cytoplasm",
                                "extract_nuclei", "extract_cell", "extract_cytoplasm",
                                "extractmulti_nuclei", "extractmulti_cell", "extractmulti_cytoplasm",
                                "extractrelate_nuclei", "extractrelate_cell"]
    assert p["steps"]["tertiary_cytoplasm"] == {"shrink_inner": True}
    assert p["steps"]["extract_cytoplasm"] is p["steps"]["extract_cell"]  # the shared spec dicts
    assert p["steps"]["extractmulti_cytoplasm"] is p["steps"]["extractmulti_cell"]
    assert p["steps"]["extractrelate_nuclei"]["others"] == ["cell"] and p["steps"]["extractrelate_cell"]["others"] == ["nuclei"]
    pd = p["passed_data"]
    assert pd["tertiary_cytoplasm"] == [("masks", "segment_cell", "outer"), ("masks", "segment_nuclei", "inner")]
    assert pd["extract_cytoplasm"] == pd["extractmulti_cytoplasm"] == [("masks", "tertiary_cytoplasm"), ("pixels", "tile")]
    assert pd["extractrelate_nuclei"] == [("masks", "segment_nuclei"), ("masks", "segment_cell", "masks_cell")]
    assert pd["extractrelate_cell"] == [("masks", "segment_cell"), ("masks", "segment_nuclei", "masks_nuclei")]
    assert p["save"] == ["segment_nuclei", "segment_cell", "tertiary_cytoplasm"]
    validate_pipeline(p)
    # everything the plain dict has is still there, unchanged
    plain = build_pipeline_steps()
    for key in plain["steps"]:
        assert p["steps"][key] == plain["steps"][key]
    for key in plain["passed_data"]:
        assert pd[key] == plain["passed_data"][key]


@pytest.mark.parametrize("kw", [
    dict(relate=[("nuclei", "membrane")]),
    dict(relate=[("nuclei", "nuclei")]),
    dict(relate=["nuclei"]),
    dict(tertiary={"cytoplasm": ("cell", "vacuole")}),
    dict(tertiary={"cell": ("cell", "nuclei")}),
    dict(tertiary={"cyto_plasm": ("cell", "nuclei")}),
    dict(tertiary={"cytoplasm": ("cell",)}),
])
def test_builder_refuses_names_that_are_not_object_sets(kw):
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError):
        build_pipeline_steps(**kw)


def test_write_dispatch_knows_tertiary():
    from aliby_amd.io.write import dispatch_write_fn, write_ndarray

    assert dispatch_write_fn("tertiary_cytoplasm") is write_ndarray


def test_init_step_errors():
    from aliby_amd.pipe import init_step

    with pytest.raises(ValueError, match="others"):
        init_step("extractrelate_nuclei", {})
    for others in ([], "cell", ["cell", "cell"], ["my_cell"]):
        with pytest.raises(ValueError):
            init_step("extractrelate_nuclei", {"others": others})
    with pytest.raises(ValueError):
        init_step("tertiary_cytoplasm", {"shrink_inner": 1})
    with pytest.raises(ValueError):
        init_step("tertiary_cytoplasm", {"shrink": True})
    # a step whose aliased input never arrives says so (before it touches a device)
    relate = init_step("extractrelate_nuclei", {"others": ["cell"]})
    with pytest.raises(ValueError, match="masks_cell"):
        relate(masks=np.zeros((4, 4), np.uint16))
    tertiary = init_step("tertiary_cytoplasm", {})
    with pytest.raises(ValueError, match="inner"):
        tertiary(outer=np.zeros((4, 4), np.uint16))


def test_validate_pipeline_checks_the_aliased_inputs():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")})
    p["passed_data"]["extractrelate_nuclei"] = [("masks", "segment_nuclei"), ("masks", "segment_cell")]  # alias lost
    with pytest.raises(ValueError, match="masks_cell"):
        validate_pipeline(p)
    p = build_pipeline_steps(tertiary={"cytoplasm": ("cell", "nuclei")})
    p["passed_data"]["tertiary_cytoplasm"] = [("masks", "segment_cell", "outer")]
    with pytest.raises(ValueError, match="inner"):
        validate_pipeline(p)
    p = build_pipeline_steps(relate=[("nuclei", "cell")])
    del p["steps"]["extractrelate_cell"]["others"]
    with pytest.raises(ValueError, match="others"):
        validate_pipeline(p)


def test_run_positions_refuses_the_new_steps(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    for kw in (dict(relate=[("nuclei", "cell")]), dict(tertiary={"cytoplasm": ("cell", "nuclei")})):
        with pytest.raises(NotImplementedError, match="tertiary_|extractrelate_"):
            parallel.run_positions([build_pipeline_steps(**kw)], ["p0"], tmp_path)
    with pytest.raises(NotImplementedError, match="volume"):  # the volume refusal stays as it is
        parallel.run_positions([build_pipeline_steps(volume_features=["intensity3d"])], ["p0"], tmp_path)


# ------------------------------------------------------------------------------------------------ the profile table
def _output(objects, instruction, keys, seed):
    from aliby_amd.extraction.extract import DeviceResults, LazyProduct

    matrix = np.random.default_rng(seed).random((len(objects), len(keys)))
    return tuple(LazyProduct(objects, [instruction])), DeviceResults(matrix, objects, [instruction], [(0, list(keys))])


def _state():
    nuclei, cells, cyto = [(0, 1), (0, 2), (0, 3)], [(0, 1), (0, 2)], [(0, 1), (0, 2)]
    size = ("None", "None", "sizeshape")
    rel = ("None", "None", "relate")
    data = {
        "extract_nuclei": [_output(nuclei, size, ["Area", "Perimeter"], 1)],
        "extract_cell": [_output(cells, size, ["Area", "Perimeter"], 2)],
        "extract_cytoplasm": [_output(cyto, size, ["Area", "Perimeter"], 3)],
        "extractrelate_nuclei": [_output(nuclei, rel, ref.names("cell"), 4)],
        "extractrelate_cell": [_output(cells, rel, ref.names("nuclei"), 5)],
    }
    return {"data": data, "tps": {}, "fn": {}}, {"steps": {k: {} for k in data}}


def _profiles_as_before(state, pipeline):
    """get_profiles_from_state as it stood before the `extractrelate` prefix: concatenate per prefix, join the prefixes."""
    from aliby_amd import pipe_core as core

    by_prefix = {}
    for name in pipeline["steps"]:
        if not (name.startswith("extract") or name.startswith("nahual_embed")):
            continue
        bucket = by_prefix.setdefault(name.split("_")[0], [])
        for tp, output in enumerate(state["data"][name]):
            table = core._wide_table(name, tp, output)
            if table is not None:
                bucket.append(table)
    merged = [pa.concat_tables(tables) for tables in by_prefix.values() if tables]
    profiles = merged[0]
    for other in merged[1:]:
        profiles = core._join_on_metadata(profiles, other)
    return profiles


def test_profile_pivot_of_two_relate_outputs():
    from aliby_amd.pipe_core import get_profiles_from_state

    state, pipeline = _state()
    table = get_profiles_from_state(state, pipeline)
    assert table.num_rows == 7
    assert table["metadata_object"].to_pylist() == ["nuclei"] * 3 + ["cell"] * 2 + ["cytoplasm"] * 2  # the extract rows' order
    assert table["metadata_label"].to_pylist() == [1, 2, 3, 1, 2, 1, 2]
    to_cell = [f"None/None/relate/{n}" for n in ref.names("cell")]
    to_nuclei = [f"None/None/relate/{n}" for n in ref.names("nuclei")]
    for col in to_cell + to_nuclei + ["None/None/sizeshape/Area", "None/None/sizeshape/Perimeter"]:
        assert col in table.column_names
        assert table.schema.field(col).type == pa.float64()
    null = {c: np.asarray(table[c].is_null().to_pylist()) for c in to_cell + to_nuclei}
    for c in to_cell:  # on nuclei rows only
        assert null[c].tolist() == [False] * 3 + [True] * 4
    for c in to_nuclei:  # on cell rows only; cytoplasm rows get nulls
        assert null[c].tolist() == [True] * 3 + [False] * 2 + [True] * 2
    assert not any(table["None/None/sizeshape/Area"].is_null().to_pylist())
    want = state["data"]["extractrelate_nuclei"][0][1].matrix[:, 0]
    assert table[to_cell[0]].to_pylist()[:3] == want.tolist()
    want = state["data"]["extractrelate_cell"][0][1].matrix[:, 4]
    assert table[to_nuclei[4]].to_pylist()[3:5] == want.tolist()


def test_profile_table_without_relate_steps_is_what_it_was():
    from aliby_amd.pipe_core import get_profiles_from_state

    state, pipeline = _state()
    for name in [n for n in pipeline["steps"] if n.startswith("extractrelate")]:
        del pipeline["steps"][name]
    got, want = get_profiles_from_state(state, pipeline), _profiles_as_before(state, pipeline)
    assert got.schema.equals(want.schema, check_metadata=True) and got.equals(want)
    assert [c.num_chunks for c in got.columns] == [c.num_chunks for c in want.columns]
