"""
The volume instruction tree without a device: `families.plan_volume` (blocks, column names, calls, every refusal, the separation of
manders_fold's and rwc's thresholds), `families.evaluate_volume` replayed on a recording engine, the builder's `volume_features`
switch, the `volume_` step's set-up errors and `run_positions`' refusal.
"""
import contextlib

import numpy as np
import pytest
import torch

from aliby_amd.extraction import families
from aliby_amd.extraction import features as feat
from aliby_amd.extraction.extract import column_names, flatten, kv

EXAMPLE = {"None": {"None": ["sizeshape3d", "neighbors3d", "projection3d"]},
           0: {"None": ["intensity3d", "intensity3d_detail", "texture3d"]},
           1: {"None": ["intensity3d", "granularity3d"]},
           (0, 1): {"None": ["pearson", "manders_fold", "rwc", "costes"]}}


def _inst(tree):
    return kv(flatten(tree))


# ------------------------------------------------------------------------------------------------ registry
def test_registry():
    assert set(families.VOLUME) == {"intensity3d", "intensity3d_detail", "texture3d", "granularity3d", "sizeshape3d", "neighbors3d",
                                    "projection3d"}
    assert {n for n, f in families.VOLUME.items() if not f.needs_pixels} == {"sizeshape3d", "neighbors3d", "projection3d"}
    assert list(families.VOLUME_PAIRS) == list(feat.COLOC)
    assert not set(families.VOLUME) & set(families.MONO) and set(families.VOLUME_PAIRS) == set(families.MULTI)
    for name in families.VOLUME:
        assert feat.family_names(name) == families.VOLUME[name].names({})
    assert feat.family_names("sizeshape3d", surface_area=True)[-1] == "SurfaceArea"
    assert feat.family_names("neighbors3d", distance=3) == feat.neighbors3d_names(3)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_of_the_example_tree():
    inst = _inst(EXAMPLE)
    p = families.plan_volume(inst, {})
    widths = [19, 7, 4, 12, 13, 169, 12, 16, 2, 2, 2, 2]
    assert [len(names) for _, names in p.blocks] == widths
    assert [c0 for c0, _ in p.blocks] == list(np.cumsum([0] + widths[:-1]))
    assert p.n_cols == sum(widths) == 260
    names = column_names(inst, p.blocks)
    assert len(names) == 260 and len(set(names)) == 260
    assert names[0] == "None/None/sizeshape3d/Volume"
    for want in ("0/None/intensity3d/Intensity_MeanIntensity", "1/None/intensity3d/Intensity_MeanIntensity",
                 "None/None/projection3d/Projection_Label", "None/None/neighbors3d/Neighbors_NumberOfNeighbors_Adjacent",
                 "1/None/granularity3d/Granularity_16", "0/None/texture3d/" + feat.texture3d_names()[0],
                 "(0, 1)/None/pearson/Correlation_Pearson", "(0, 1)/None/costes/Correlation_Costes_2"):
        assert want in names, want
    assert [(c.method, c.target, c.col0, c.ncols) for c in p.calls] == [
        ("sizeshape3d", None, 0, 19), ("neighbors3d", None, 19, 7), ("projection3d", None, 26, 4), ("intensity3d", 0, 30, 12),
        ("intensity3d_detail", 0, 42, 13), ("texture3d", 0, 55, 169), ("intensity3d", 1, 224, 12), ("granularity3d", 1, 236, 16),
        ("coloc3d", [(0, 1)], 252, 8)]
    assert p.calls[-1].kw == dict(metrics=("pearson", "manders_fold", "rwc", "costes"), thr=15.0, scale_max=255.0)


def test_plan_keywords_rename_and_resize_columns():
    kw = {"sizeshape3d": {"spacing": (2.0, 0.5, 0.5), "surface_area": True}, "intensity3d_detail": {"edge_measurements": False},
          "texture3d": {"scale": 2, "gray_levels": 64}, "granularity3d": {"granular_spectrum_length": 3, "element_size": 2},
          "neighbors3d": {"distance": 3}, "texture": {"distance": 9}}  # (the last: a family the tree does not use is ignored)
    inst = _inst(EXAMPLE)
    p = families.plan_volume(inst, kw)
    assert [len(n) for _, n in p.blocks] == [20, 7, 4, 12, 8, 169, 12, 3, 2, 2, 2, 2]
    names = column_names(inst, p.blocks)
    assert "None/None/sizeshape3d/SurfaceArea" in names and "None/None/neighbors3d/Neighbors_NumberOfNeighbors_3" in names
    assert "0/None/texture3d/" + feat.texture3d_names(2, 64)[0] in names
    by_method = {(c.method, c.target if not isinstance(c.target, list) else None): c.kw for c in p.calls}
    assert by_method[("sizeshape3d", None)] == kw["sizeshape3d"]
    assert by_method[("granularity3d", 1)] == kw["granularity3d"]
    assert by_method[("intensity3d", 0)] == {}


def test_thr_of_manders_fold_does_not_leak_into_rwc():
    inst = _inst({(0, 1): {"None": ["pearson", "manders_fold", "rwc", "costes"]}})
    p = families.plan_volume(inst, {"manders_fold": {"thr": 30}, "costes": {"scale_max": 4095}})
    assert [(c.method, c.target, c.kw, c.col0, c.ncols) for c in p.calls] == [
        ("coloc3d", [(0, 1)], dict(metrics=("pearson", "manders_fold"), thr=30.0, scale_max=255.0), 0, 4),
        ("coloc3d", [(0, 1)], dict(metrics=("rwc", "costes"), thr=15.0, scale_max=4095.0), 4, 4)]
    same = families.plan_volume(inst, {"manders_fold": {"thr": 30}, "rwc": {"thr": 30}})
    assert len(same.calls) == 1 and same.calls[0].kw["thr"] == 30.0


def test_pairs_with_the_same_metrics_share_a_call():
    metrics = ["pearson", "costes", "manders_fold", "rwc"]
    inst = _inst({(0, 1): {"None": metrics}, (0, 2): {"None": metrics}, (1, 2): {"None": metrics[:2]}, 0: {"None": ["intensity3d"]}})
    p = families.plan_volume(inst, {})
    assert [(c.method, c.target, c.col0, c.ncols) for c in p.calls] == [
        ("coloc3d", [(0, 1), (0, 2)], 0, 16), ("coloc3d", [(1, 2)], 16, 4), ("intensity3d", 0, 20, 12)]
    assert feat.coloc3d_names([(0, 1), (0, 2)], metrics) == [n.replace("/None/", "/") for n in column_names(inst, p.blocks)[:16]]


@pytest.mark.parametrize("tree, kwargs, error", [
    ({0: {"None": ["intensity3d", "no_such_family"]}}, {}, KeyError),
    ({0: {"None": ["intensity"]}}, {}, KeyError),  # a 2-D name
    ({0: {"max": ["intensity3d"]}}, {}, ValueError),  # a reducer
    ({"None": {"max": ["sizeshape3d"]}}, {}, ValueError),
    ({0: {"None": ["sizeshape3d"]}}, {}, ValueError),  # pixel-free under a channel
    ({1: {"None": ["projection3d"]}}, {}, ValueError),
    ({"None": {"None": ["intensity3d"]}}, {}, ValueError),  # a pixel family under "None"
    ({(0, 0): {"None": ["pearson"]}}, {}, ValueError),  # not two distinct channels
    ({(0, 1, 2): {"None": ["pearson"]}}, {}, ValueError),
    ({(0, "1"): {"None": ["pearson"]}}, {}, ValueError),
    ({0: {"None": ["pearson"]}}, {}, ValueError),  # a pair name under a single channel
    ({"None": {"None": ["rwc"]}}, {}, ValueError),
    ({(0, 1): {"None": ["intensity3d"]}}, {}, ValueError),  # and the reverse
    ({(0, 1): {"None": ["projection3d"]}}, {}, ValueError),
    ({0: {"None": {"max": ["intensity3d"]}}}, {}, ValueError),  # depth 4
    ({0: {"None": ["texture3d"]}}, {"texture3d": {"distance": 2}}, NotImplementedError),
    ({"None": {"None": ["projection3d"]}}, {"projection3d": {"anything": 1}}, NotImplementedError),
    ({(0, 1): {"None": ["pearson"]}}, {"pearson": {"thr": 3}}, NotImplementedError),
    ({(0, 1): {"None": ["costes"]}}, {"costes": {"thr": 3}}, NotImplementedError),
])
def test_refusals(tree, kwargs, error):
    with pytest.raises(error) as e:
        families.plan_volume(_inst(tree), kwargs)
    if error is NotImplementedError:
        assert next(iter(kwargs)) in str(e.value)  # names the family


# ------------------------------------------------------------------------------------------------ the evaluator, recorded
class RecordingVolumeEngine:
    """Stands in for FeatureEngine: logs every volume call, and fills the columns it owns with the column's own index."""

    def __init__(self):
        self.events, self.out = [], None

    def timed(self, name):
        return contextlib.nullcontext()

    def new_output(self, rows, cols):
        self.out = torch.full((max(rows, 1), max(cols, 1)), float("nan"), dtype=torch.float64)[:rows]
        return self.out

    def _mark(self, name, out, col0, n, **args):
        assert out is self.out
        self.events.append([name, col0, n, args])
        for j in range(n):
            out[:, col0 + j] = float(col0 + j)

    def sizeshape3d(self, volume, counts, spacing=(1.0, 1.0, 1.0), surface_area=False, out=None, col0=0):
        self._mark("sizeshape3d", out, col0, len(feat.sizeshape3d_names(surface_area)), spacing=spacing, surface_area=surface_area)

    def neighbors3d(self, volume, counts, distance=None, out=None, col0=0):
        self._mark("neighbors3d", out, col0, 7, distance=distance)

    def projection3d(self, volume, counts, out=None, col0=0):
        self._mark("projection3d", out, col0, 4)

    def intensity3d(self, volume, pixels, channel, counts, out=None, col0=0):
        self._mark("intensity3d", out, col0, 12, channel=channel)

    def intensity3d_detail(self, volume, pixels, channel, counts, edge_measurements=True, out=None, col0=0):
        self._mark("intensity3d_detail", out, col0, len(feat.intensity3d_detail_names(edge_measurements)), channel=channel,
                   edge_measurements=edge_measurements)

    def texture3d(self, volume, pixels, channel, counts, scale=3, gray_levels=256, out=None, col0=0):
        self._mark("texture3d", out, col0, 169, channel=channel, scale=scale, gray_levels=gray_levels)

    def granularity3d(self, volume, pixels, channel, counts, out=None, col0=0, **kw):
        self._mark("granularity3d", out, col0, kw.get("granular_spectrum_length", 16), channel=channel, **kw)

    def coloc3d(self, volume, pixels, pairs, counts, metrics=("pearson", "manders_fold", "rwc", "costes"), thr=15.0, scale_max=255.0,
                out=None, col0=0):
        self._mark("coloc3d", out, col0, len(feat.coloc3d_names(pairs, metrics)), pairs=list(pairs), metrics=tuple(metrics), thr=thr,
                   scale_max=scale_max)


def test_evaluate_volume_replays_the_plan():
    eng = RecordingVolumeEngine()
    volume = torch.zeros((2, 3, 8, 9), dtype=torch.uint16)
    pixels = torch.zeros((2, 2, 3, 8, 9), dtype=torch.uint16)
    kw = {"manders_fold": {"thr": 30}, "granularity3d": {"granular_spectrum_length": 3}, "neighbors3d": {"distance": 2}}
    inst = _inst(EXAMPLE)
    out, blocks = families.evaluate_volume(eng, volume, pixels, [3, 2], inst, kw)
    p = families.plan_volume(inst, kw)
    assert out is eng.out and tuple(out.shape) == (5, p.n_cols) and blocks == p.blocks
    assert out[0].tolist() == [float(j) for j in range(p.n_cols)]  # every column written once, by its own call, in place
    assert [(e[0], e[1], e[2]) for e in eng.events] == [(c.method, c.col0, c.ncols) for c in p.calls]
    assert [e[1] for e in eng.events] == sorted(e[1] for e in eng.events)
    coloc = [e[3] for e in eng.events if e[0] == "coloc3d"]
    assert coloc == [dict(pairs=[(0, 1)], metrics=("pearson", "manders_fold"), thr=30.0, scale_max=255.0),
                     dict(pairs=[(0, 1)], metrics=("rwc", "costes"), thr=15.0, scale_max=255.0)]
    assert [e[3] for e in eng.events if e[0] == "neighbors3d"] == [dict(distance=2)]


def test_evaluate_volume_without_pixels():
    eng = RecordingVolumeEngine()
    volume = torch.zeros((1, 3, 8, 9), dtype=torch.uint16)
    out, _ = families.evaluate_volume(eng, volume, None, [0], _inst({"None": {"None": ["sizeshape3d", "projection3d"]}}), {})
    assert tuple(out.shape) == (0, 23)
    with pytest.raises(Exception, match="pixels are required"):
        families.evaluate_volume(eng, volume, None, [2], _inst({0: {"None": ["intensity3d"]}}), {})


# ------------------------------------------------------------------------------------------------ the builder and the step
def test_builder_default_is_unchanged():
    from aliby_amd.pipe_builder import build_pipeline_steps

    assert build_pipeline_steps() == build_pipeline_steps(volume_features=None, volume_coloc=False)
    assert repr(build_pipeline_steps()) == repr(build_pipeline_steps(volume_features=None))
    assert repr(build_pipeline_steps(volume_coloc=True)) == repr(build_pipeline_steps())  # nothing without volume_features
    assert not any(n.startswith("volume_") for n in build_pipeline_steps()["steps"])
    assert "do_3D" not in build_pipeline_steps()["steps"]["segment_nuclei"]["segmenter_kwargs"]
    with pytest.raises(TypeError):
        build_pipeline_steps(None, None, ("intensity",), None, None, None, None, None, None, ("intensity3d",))  # keyword-only


def test_builder_volume_features():
    from aliby_amd import pipe_core
    from aliby_amd.pipe_builder import COLOC_METRICS, build_pipeline_steps

    plain = build_pipeline_steps(channels_to_segment={"nuclei": 0, "cell": 1}, channels_to_extract=[0, 1, 2], features_to_extract=("intensity",))
    p = build_pipeline_steps(channels_to_segment={"nuclei": 0, "cell": 1}, channels_to_extract=[0, 1, 2], features_to_extract=("intensity",),
                             volume_features=("intensity3d",))
    pipe_core.validate_pipeline(p)
    for obj in ("nuclei", "cell"):
        assert p["steps"][f"segment_{obj}"]["segmenter_kwargs"] == {"kind": "cellpose", "do_3D": True}
        step = p["steps"][f"volume_{obj}"]
        assert step["volume_from"] == f"segment_{obj}"
        assert step["tree"] == {"None": {"None": ["sizeshape3d", "projection3d"]}, 0: {"None": ["intensity3d"]},
                                1: {"None": ["intensity3d"]}, 2: {"None": ["intensity3d"]}}
        assert p["passed_data"][f"volume_{obj}"] == [("pixels", "tile")]
        # the 2-D steps stay, and measure the collapse
        for prefix in ("extract", "extractmulti"):
            assert p["steps"][f"{prefix}_{obj}"] == plain["steps"][f"{prefix}_{obj}"]
            assert p["passed_data"][f"{prefix}_{obj}"] == plain["passed_data"][f"{prefix}_{obj}"]
    assert list(p["steps"]).index("volume_nuclei") > list(p["steps"]).index("segment_nuclei")
    assert p["save"] == plain["save"]
    families.plan_volume(_inst(p["steps"]["volume_nuclei"]["tree"]), {})

    q = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1, 2], volume_features=("intensity3d", "texture3d"),
                             volume_coloc=True, cp_measure_feature_kwargs={"texture3d": {"scale": 2}})
    pipe_core.validate_pipeline(q)
    tree = q["steps"]["volume_nuclei"]["tree"]
    assert [k for k in tree if isinstance(k, tuple)] == [(0, 1), (0, 2), (1, 2)]
    assert all(tree[k] == {"None": list(COLOC_METRICS)} for k in tree if isinstance(k, tuple))
    assert q["steps"]["volume_nuclei"]["kwargs"]["cp_measure_kwargs"] == {"texture3d": {"scale": 2}}
    plan = families.plan_volume(_inst(tree), q["steps"]["volume_nuclei"]["kwargs"]["cp_measure_kwargs"])
    assert [c.target for c in plan.calls if c.method == "coloc3d"] == [[(0, 1), (0, 2), (1, 2)]]


def test_volume_step_setup_errors():
    from aliby_amd.pipe import init_step

    tree = {"None": {"None": ["projection3d"]}}
    with pytest.raises(ValueError, match="tree"):
        init_step("volume_x", {"volume_from": "segment_x"})
    with pytest.raises(ValueError, match="volume_from"):
        init_step("volume_x", {"tree": tree})
    with pytest.raises(ValueError, match="segment step"):
        init_step("volume_x", {"tree": tree, "volume_from": "tile"})
    with pytest.raises(KeyError):
        init_step("volume_x", {"tree": {"None": {"None": ["sizeshape"]}}, "volume_from": "segment_x"})
    with pytest.raises(NotImplementedError, match="projection3d"):
        init_step("volume_x", {"tree": tree, "volume_from": "segment_x", "kwargs": {"cp_measure_kwargs": {"projection3d": {"a": 1}}}})

    class Pixels:
        shape = (1, 2, 3, 8, 9)

    class Segment:
        last_volume = None

    # at run time: the segment step is missing, is no segmenter, kept no volume, or kept one of another shape
    step = init_step("volume_x", {"tree": tree, "volume_from": "segment_x"}, {"tile": object()})
    with pytest.raises(ValueError, match="segment_x"):
        step(pixels=Pixels())
    step = init_step("volume_x", {"tree": tree, "volume_from": "segment_x"}, {"segment_x": object()})
    with pytest.raises(ValueError, match="not a segment step"):
        step(pixels=Pixels())
    step = init_step("volume_x", {"tree": tree, "volume_from": "segment_x"}, {"segment_x": Segment()})
    with pytest.raises(ValueError, match="do_3D"):
        step(pixels=Pixels())
    seg = Segment()
    seg.last_volume = (torch.zeros((1, 3, 8, 10), dtype=torch.uint16), np.asarray([0]))
    step = init_step("volume_x", {"tree": tree, "volume_from": "segment_x"}, {"segment_x": seg})
    with pytest.raises(ValueError, match="do not match"):
        step(pixels=Pixels())


def test_volume_step_is_not_an_extract_step():
    """Every step that starts with "extract" is joined to the 2-D rows on metadata_label: the volume step must stay out of that."""
    import pyarrow as pa

    from aliby_amd import pipe_core
    from aliby_amd.extraction.extract import DeviceResults, LazyProduct
    from aliby_amd.pipe_builder import build_pipeline_steps

    p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0], volume_features=("intensity3d",))
    assert not [n for n in p["steps"] if n.startswith("extract") and "volume" in n]
    inst = _inst({"None": {"None": ["projection3d"]}})
    blocks = families.plan_volume(inst, {}).blocks
    objects = [(0, 1), (0, 2), (0, 3)]
    matrix = np.asarray([[4, 4, 1.0, 1], [6, 0, 0.0, 0], [5, 5, 1.0, 2]], np.float64)
    state = {"data": {n: [] for n in p["steps"]}}
    state["data"]["volume_nuclei"] = [(LazyProduct(objects, inst), DeviceResults(matrix, objects, inst, blocks))]
    table = pipe_core.get_volume_profiles_from_state(state, p)
    assert table.column("metadata_label").to_pylist() == [1, 2, 3] and table.column("metadata_object").to_pylist() == ["nuclei"] * 3
    assert table.column("metadata_tp").to_pylist() == [0, 0, 0] and table.column("metadata_tile").to_pylist() == [0, 0, 0]
    assert table.column("None/None/projection3d/Projection_Label").to_pylist() == [1.0, 0.0, 2.0]
    assert pipe_core.get_profiles_from_state(state, p).num_rows == 0  # (no extract output in this state: nothing of the volume step)
    empty = pipe_core.get_volume_profiles_from_state({"data": {n: [] for n in p["steps"]}}, p)
    assert isinstance(empty, pa.Table) and empty.num_rows == 0


def test_run_positions_refuses_volume_pipelines(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0], volume_features=("intensity3d",))
    with pytest.raises(NotImplementedError, match="run_pipeline_and_post"):
        parallel.run_positions([p], ["a"], tmp_path)
    q = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0])
    q["steps"]["segment_nuclei"]["segmenter_kwargs"]["do_3D"] = False  # the key alone: the batched segmenter has no such argument
    with pytest.raises(NotImplementedError, match="run_pipeline_and_post"):
        parallel.run_positions([q], ["a"], tmp_path)
    assert not list(tmp_path.iterdir())

