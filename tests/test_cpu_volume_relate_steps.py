"""
The pipeline layer of `relate3d` without a device: the builder's `volume_relate` keyword (the dict without it is what it was; the
steps and wiring with it; its refusals), `validate_pipeline`'s checks of the wiring, the set-up and run-time errors of the
`volumetertiary_` / `volumerelate_` steps and of a `volume_` step fed by one (fake segment objects carrying `last_volume`), the join of
the `volumerelate_` rows in the volume profile table, and `run_positions`' refusal.
"""
import numpy as np
import pyarrow as pa
import pytest
import torch

from tests import relate3d_ref as ref

ARGUMENT_SETS = [
    dict(),
    dict(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}),
    dict(volume_features=("intensity3d",)),
    dict(volume_features=("intensity3d", "texture3d"), volume_coloc=True, relate=[("nuclei", "cell")]),
    dict(channels_to_segment={"nuclei": 0, "cell": 1}, channels_to_extract=[0, 1, 2], features_to_extract=("intensity",),
         volume_features=("intensity3d",), relate=[("nuclei", "cell"), ("cytoplasm", "nuclei")], tertiary={"cytoplasm": ("cell", "nuclei")},
         cp_measure_feature_kwargs={"texture3d": {"scale": 2}}, steps_to_write=["segment_cell"]),
]
ON = dict(volume_features=("intensity3d",), relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}, volume_relate=True)


# ------------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize("kw", ARGUMENT_SETS)
def test_builder_without_the_keyword_is_unchanged(kw):
    from aliby_amd.pipe_builder import build_pipeline_steps

    plain, off = build_pipeline_steps(**kw), build_pipeline_steps(**kw, volume_relate=False)
    assert plain == off and repr(plain) == repr(off)
    assert not any(n.startswith(("volumetertiary_", "volumerelate_")) for n in plain["steps"])
    assert not any(n.startswith(("volumetertiary_", "volumerelate_")) for n in plain["passed_data"])
    assert "volume_cytoplasm" not in plain["steps"]


def test_the_dicts_of_today_step_by_step():
    """What the builder returned before the keyword existed, written out: the step order of three argument sets."""
    from aliby_amd.pipe_builder import build_pipeline_steps

    assert list(build_pipeline_steps()["steps"]) == ["tile", "segment_nuclei", "segment_cell", "extract_nuclei", "extract_cell",
                                                     "extractmulti_nuclei", "extractmulti_cell"]
    p = build_pipeline_steps(**ARGUMENT_SETS[1], volume_features=("intensity3d",))
    assert list(p["steps"]) == ["tile", "segment_nuclei", "segment_cell", "tertiary_cytoplasm", "extract_nuclei", "extract_cell",
                                "extract_cytoplasm", "extractmulti_nuclei", "extractmulti_cell", "extractmulti_cytoplasm",
                                "extractrelate_nuclei", "extractrelate_cell", "volume_nuclei", "volume_cell"]
    assert sorted(p["passed_data"]) == sorted(n for n in p["steps"] if n not in ("tile", "segment_nuclei", "segment_cell"))
    assert p["save"] == ["segment_nuclei", "segment_cell", "tertiary_cytoplasm"]
    with pytest.raises(TypeError):  # keyword-only
        build_pipeline_steps(None, None, ("intensity",), None, None, None, None, None, None, None, False, None, None, True)


def test_builder_with_the_keyword():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    off = build_pipeline_steps(**{k: v for k, v in ON.items() if k != "volume_relate"})
    p = build_pipeline_steps(**ON)
    assert list(p["steps"]) == ["tile", "segment_nuclei", "segment_cell", "tertiary_cytoplasm", "volumetertiary_cytoplasm",
                                "extract_nuclei", "extract_cell", "extract_cytoplasm",
                                "extractmulti_nuclei", "extractmulti_cell", "extractmulti_cytoplasm",
                                "extractrelate_nuclei", "extractrelate_cell", "volume_nuclei", "volume_cell", "volume_cytoplasm",
                                "volumerelate_nuclei", "volumerelate_cell"]
    assert p["steps"]["volumetertiary_cytoplasm"] == {"outer": "segment_cell", "inner": "segment_nuclei", "shrink_inner": True}
    assert p["steps"]["volume_cytoplasm"] == {"tree": p["steps"]["volume_cell"]["tree"], "volume_from": "volumetertiary_cytoplasm",
                                              "kwargs": p["steps"]["volume_cell"]["kwargs"]}
    assert p["steps"]["volume_cytoplasm"]["tree"] is p["steps"]["volume_cell"]["tree"]  # the shared volume tree
    assert p["steps"]["volumerelate_nuclei"] == {"volume_from": "segment_nuclei", "others": {"cell": "segment_cell"},
                                                 "spacing": (1.0, 1.0, 1.0)}
    assert p["steps"]["volumerelate_cell"] == {"volume_from": "segment_cell", "others": {"nuclei": "segment_nuclei"},
                                               "spacing": (1.0, 1.0, 1.0)}
    assert p["passed_data"]["volume_cytoplasm"] == [("pixels", "tile")]
    assert not any(n.startswith(("volumetertiary_", "volumerelate_")) for n in p["passed_data"])  # they read the kept volumes
    validate_pipeline(p)
    # everything the dict without the keyword has is still there, unchanged
    for key in off["steps"]:
        assert p["steps"][key] == off["steps"][key]
    assert {k: v for k, v in p["passed_data"].items() if k != "volume_cytoplasm"} == off["passed_data"]
    assert p["save"] == off["save"] and p["passed_methods"] == off["passed_methods"]
    # a tertiary name among the related sets: its producer is the volumetertiary step
    q = build_pipeline_steps(volume_features=("intensity3d",), relate=[("cytoplasm", "nuclei")], tertiary={"cytoplasm": ("cell", "nuclei")},
                             volume_relate=True)
    assert q["steps"]["volumerelate_cytoplasm"]["volume_from"] == "volumetertiary_cytoplasm"
    assert q["steps"]["volumerelate_nuclei"]["others"] == {"cytoplasm": "volumetertiary_cytoplasm"}
    validate_pipeline(q)
    # one of the two suffices
    only_relate = build_pipeline_steps(volume_features=("intensity3d",), relate=[("nuclei", "cell")], volume_relate=True)
    assert [n for n in only_relate["steps"] if n.startswith("volume")] == ["volume_nuclei", "volume_cell", "volumerelate_nuclei", "volumerelate_cell"]
    only_tertiary = build_pipeline_steps(volume_features=("intensity3d",), tertiary={"cytoplasm": ("cell", "nuclei")}, volume_relate=True)
    assert [n for n in only_tertiary["steps"] if n.startswith("volume")] == ["volumetertiary_cytoplasm", "volume_nuclei", "volume_cell", "volume_cytoplasm"]


@pytest.mark.parametrize("kw", [
    dict(relate=[("nuclei", "cell")], volume_relate=True),  # no volume_features
    dict(volume_features=("intensity3d",), volume_relate=True),  # neither relate nor tertiary
    dict(volume_features=("intensity3d",), relate=[], tertiary={}, volume_relate=True),
    dict(volume_features=("intensity3d",), relate=[("nuclei", "cell")], volume_relate=1),
])
def test_builder_refusals(kw):
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError, match="volume_relate"):
        build_pipeline_steps(**kw)


def test_prefixes_and_write_dispatch():
    from aliby_amd import pipe
    from aliby_amd.io.write import dispatch_write_fn, write_ndarray

    prefixes = [p for p, _ in pipe._PREFIXES]
    assert "volumetertiary_" in prefixes and "volumerelate_" in prefixes
    for p in ("volumetertiary_", "volumerelate_"):
        assert not p.startswith("extract") and not p.startswith("volume_")
    assert dispatch_write_fn("volumetertiary_cytoplasm") is write_ndarray


# ------------------------------------------------------------------------------------------------ validation
def test_validate_pipeline_checks_the_wiring():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    def broken(change):
        p = build_pipeline_steps(**ON)
        change(p["steps"])
        return p

    with pytest.raises(ValueError, match="inner"):
        validate_pipeline(broken(lambda s: s["volumetertiary_cytoplasm"].pop("inner")))
    with pytest.raises(ValueError, match="segment_membrane"):
        validate_pipeline(broken(lambda s: s["volumetertiary_cytoplasm"].update(outer="segment_membrane")))
    with pytest.raises(ValueError, match="segment step"):
        validate_pipeline(broken(lambda s: s["volumerelate_nuclei"].update(volume_from="tile")))
    with pytest.raises(ValueError, match="others"):
        validate_pipeline(broken(lambda s: s["volumerelate_nuclei"].pop("others")))
    with pytest.raises(ValueError, match="others"):
        validate_pipeline(broken(lambda s: s["volumerelate_nuclei"].update(others=["cell"])))
    with pytest.raises(ValueError, match="segment_vacuole"):
        validate_pipeline(broken(lambda s: s["volumerelate_nuclei"].update(others={"vacuole": "segment_vacuole"})))
    with pytest.raises(ValueError, match="volumetertiary_cytoplasm"):
        validate_pipeline(broken(lambda s: s.pop("volumetertiary_cytoplasm")))  # volume_cytoplasm has lost its source
    with pytest.raises(ValueError, match="do_3D"):
        validate_pipeline(broken(lambda s: s["segment_cell"]["segmenter_kwargs"].pop("do_3D")))

    def late(steps):  # the tertiary volume after the step that measures it
        steps["volumetertiary_cytoplasm"] = steps.pop("volumetertiary_cytoplasm")

    with pytest.raises(ValueError, match="before"):
        validate_pipeline(broken(late))


# ------------------------------------------------------------------------------------------------ the steps
class Segment:
    last_volume = None

    def __init__(self, volume=None, counts=None):
        if volume is not None:
            self.last_volume = (torch.from_numpy(np.ascontiguousarray(volume)), np.asarray(counts))


def test_volumetertiary_step_errors():
    from aliby_amd.pipe import init_step

    ok = {"outer": "segment_cell", "inner": "segment_nuclei"}
    for params, match in (({"inner": "segment_nuclei"}, "outer"), ({"outer": "segment_cell"}, "inner"),
                          ({**ok, "outer": "tile"}, "segment step"), ({**ok, "inner": 3}, "segment step"),
                          ({**ok, "inner": "segment_cell"}, "different"), ({**ok, "shrink_inner": 1}, "shrink_inner"),
                          ({**ok, "shrink": True}, "unknown")):
        with pytest.raises(ValueError, match=match):
            init_step("volumetertiary_cytoplasm", params, {})
    a, b, _, _ = ref.scenes()["worked"]
    # at run time: a source is missing, is no segmenter, kept no volume, or the two volumes differ in shape
    step = init_step("volumetertiary_cytoplasm", dict(ok), {"segment_nuclei": Segment(a[None], [3])})
    assert step.last_volume is None
    with pytest.raises(ValueError, match="volumetertiary_cytoplasm.*segment_cell"):
        step()
    step = init_step("volumetertiary_cytoplasm", dict(ok), {"segment_cell": object(), "segment_nuclei": Segment(a[None], [3])})
    with pytest.raises(ValueError, match="not a segment step"):
        step()
    step = init_step("volumetertiary_cytoplasm", dict(ok), {"segment_cell": Segment(b[None], [2]), "segment_nuclei": Segment()})
    with pytest.raises(ValueError, match="segment_nuclei.*do_3D"):
        step()
    step = init_step("volumetertiary_cytoplasm", dict(ok), {"segment_cell": Segment(b[None], [2]), "segment_nuclei": Segment(a[None, :2], [3])})
    with pytest.raises(ValueError, match="do not match"):
        step()
    assert step.last_volume is None


def test_volumerelate_step_errors():
    from aliby_amd.pipe import init_step

    ok = {"volume_from": "segment_nuclei", "others": {"cell": "segment_cell"}}
    for params, match in (({"others": {"cell": "segment_cell"}}, "volume_from"), ({"volume_from": "segment_nuclei"}, "others"),
                          ({**ok, "volume_from": "tile"}, "segment step"), ({**ok, "others": {}}, "others"),
                          ({**ok, "others": ["cell"]}, "others"), ({**ok, "others": {"my_cell": "segment_cell"}}, "my_cell"),
                          ({**ok, "others": {"cell": "extract_cell"}}, "segment step"), ({**ok, "spacing": (1, 0, 1)}, "spacing"),
                          ({**ok, "spacing": (1, 1)}, "volumerelate_nuclei"), ({**ok, "kwargs": {}}, "unknown")):
        with pytest.raises(ValueError, match=match):
            init_step("volumerelate_nuclei", params, {})
    a, b, _, _ = ref.scenes()["worked"]
    step = init_step("volumerelate_nuclei", dict(ok), {"segment_cell": Segment(b[None], [2])})
    with pytest.raises(ValueError, match="volumerelate_nuclei.*segment_nuclei"):
        step()
    step = init_step("volumerelate_nuclei", dict(ok), {"segment_nuclei": Segment(a[None], [3]), "segment_cell": Segment()})
    with pytest.raises(ValueError, match="segment_cell.*single plane"):
        step()
    step = init_step("volumerelate_nuclei", dict(ok), {"segment_nuclei": Segment(a[None], [3]), "segment_cell": Segment(b[None, :, :5], [2])})
    with pytest.raises(ValueError, match="do not match"):
        step()


def test_volume_step_takes_a_volumetertiary_source():
    from aliby_amd.pipe import init_step

    tree = {"None": {"None": ["projection3d"]}}
    init_step("volume_cytoplasm", {"tree": tree, "volume_from": "volumetertiary_cytoplasm"})
    for source in ("tile", "tertiary_cytoplasm", "volumerelate_cell", "volume_cell", 7):
        with pytest.raises(ValueError, match="segment step"):
            init_step("volume_cytoplasm", {"tree": tree, "volume_from": source})

    class Pixels:
        shape = (1, 2, 3, 6, 8)

    a, b, _, _ = ref.scenes()["worked"]
    tertiary = init_step("volumetertiary_cytoplasm", {"outer": "segment_cell", "inner": "segment_nuclei"}, {})
    step = init_step("volume_cytoplasm", {"tree": tree, "volume_from": "volumetertiary_cytoplasm"}, {"volumetertiary_cytoplasm": tertiary})
    with pytest.raises(ValueError, match="kept no volume"):  # the tertiary step has not run (or failed) at this timepoint
        step(pixels=Pixels())
    tertiary.last_volume = (torch.zeros((1, 3, 6, 9), dtype=torch.uint16), np.asarray([2]))
    with pytest.raises(ValueError, match="do not match"):
        step(pixels=Pixels())


# ------------------------------------------------------------------------------------------------ the profile table
def _output(objects, instruction, keys, seed):
    from aliby_amd.extraction.extract import DeviceResults, LazyProduct

    matrix = np.random.default_rng(seed).random((len(objects), len(keys)))
    return tuple(LazyProduct(objects, [instruction])), DeviceResults(matrix, objects, [instruction], [(0, list(keys))])


def _state():
    nuclei, cells, cyto = [(0, 1), (0, 2), (0, 3)], [(0, 1), (0, 2)], [(0, 1), (0, 2)]
    size, rel = ("None", "None", "sizeshape3d"), ("None", "None", "relate3d")
    data = {
        "volume_nuclei": [_output(nuclei, size, ["Volume", "Extent"], 1)],
        "volume_cell": [_output(cells, size, ["Volume", "Extent"], 2)],
        "volume_cytoplasm": [_output(cyto, size, ["Volume", "Extent"], 3)],
        "volumerelate_nuclei": [_output(nuclei, rel, ref.names("cell"), 4)],
        "volumerelate_cell": [_output(cells, rel, ref.names("nuclei"), 5)],
    }
    return {"data": data, "tps": {}, "fn": {}}, {"steps": {k: {} for k in data}}


def test_volume_profile_table_joins_the_relate3d_rows():
    from aliby_amd.extraction.extract import RELATE3D_INSTRUCTION
    from aliby_amd.pipe_core import get_profiles_from_state, get_volume_profiles_from_state

    assert RELATE3D_INSTRUCTION == ("None", "None", "relate3d")
    state, pipeline = _state()
    table = get_volume_profiles_from_state(state, pipeline)
    assert table.num_rows == 7
    assert table["metadata_object"].to_pylist() == ["nuclei"] * 3 + ["cell"] * 2 + ["cytoplasm"] * 2  # the volume rows' order
    assert table["metadata_label"].to_pylist() == [1, 2, 3, 1, 2, 1, 2]
    to_cell = [f"None/None/relate3d/{n}" for n in ref.names("cell")]
    to_nuclei = [f"None/None/relate3d/{n}" for n in ref.names("nuclei")]
    for col in to_cell + to_nuclei + ["None/None/sizeshape3d/Volume", "None/None/sizeshape3d/Extent"]:
        assert col in table.column_names and table.schema.field(col).type == pa.float64()
    null = {c: table[c].is_null().to_pylist() for c in to_cell + to_nuclei}
    for c in to_cell:  # on nuclei rows only
        assert null[c] == [False] * 3 + [True] * 4
    for c in to_nuclei:  # on cell rows only; cytoplasm rows get nulls
        assert null[c] == [True] * 3 + [False] * 2 + [True] * 2
    assert not any(table["None/None/sizeshape3d/Volume"].is_null().to_pylist())
    assert table[to_cell[0]].to_pylist()[:3] == state["data"]["volumerelate_nuclei"][0][1].matrix[:, 0].tolist()
    assert table[to_nuclei[4]].to_pylist()[3:5] == state["data"]["volumerelate_cell"][0][1].matrix[:, 4].tolist()
    # the cytoplasm rows join their cell on (tp, tile, label)
    rows = table.to_pylist()
    cells = {(r["metadata_tp"], r["metadata_tile"], r["metadata_label"]) for r in rows if r["metadata_object"] == "cell"}
    assert all((r["metadata_tp"], r["metadata_tile"], r["metadata_label"]) in cells for r in rows if r["metadata_object"] == "cytoplasm")
    assert get_profiles_from_state(state, pipeline).num_rows == 0  # nothing of these steps reaches the 2-D table


def test_volume_profile_table_without_relate_steps_is_what_it_was():
    from aliby_amd import pipe_core as core

    state, pipeline = _state()
    for name in [n for n in pipeline["steps"] if n.startswith("volumerelate_")]:
        del pipeline["steps"][name]
    got = core.get_volume_profiles_from_state(state, pipeline)
    want = pa.concat_tables([core._wide_table(n, 0, state["data"][n][0]) for n in pipeline["steps"]])  # (as it stood before)
    assert got.schema.equals(want.schema, check_metadata=True) and got.equals(want)
    assert [c.num_chunks for c in got.columns] == [c.num_chunks for c in want.columns]
    # relate3d rows without any volume_ rows: the empty table, as before
    state, pipeline = _state()
    for name in [n for n in pipeline["steps"] if n.startswith("volume_")]:
        del pipeline["steps"][name]
    assert core.get_volume_profiles_from_state(state, pipeline).num_rows == 0


# ------------------------------------------------------------------------------------------------ run_positions
def test_run_positions_refuses_the_new_steps(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(NotImplementedError, match="run_pipeline_and_post"):
        parallel.run_positions([build_pipeline_steps(**ON)], ["p0"], tmp_path)
    # by the step's own prefix, not only through the volume refusal: a dict by hand without do_3D and without a volume_ step
    for name, params in (("volumetertiary_cytoplasm", {"outer": "segment_cell", "inner": "segment_nuclei"}),
                         ("volumerelate_nuclei", {"volume_from": "segment_nuclei", "others": {"cell": "segment_cell"}})):
        p = build_pipeline_steps()
        p["steps"][name] = params
        with pytest.raises(NotImplementedError, match="volumetertiary_|volumerelate_") as e:
            parallel.run_positions([p], ["p0"], tmp_path)
        assert name in str(e.value)
    assert not list(tmp_path.iterdir())
