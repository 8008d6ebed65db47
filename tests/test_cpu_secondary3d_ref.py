"""
The volume form of `secondary` without a device: the brute-force restatement (tests/secondary3d_ref.py) against SciPy's distance
transform with `sampling=` on every voxel that is not a tie, against the 2-D restatement on one plane, and on the hand-worked tie
cases the GPU tests run (tests/secondary3d_cases.py); `features.secondary_volume_args`; the builder's `volume_secondary` keyword (the
dict without it is what it was; the steps and wiring with it; its refusals); `validate_pipeline`'s checks of the wiring; the set-up
and run-time errors of a `volumesecondary_` step (fake segment objects carrying `last_volume`); `run_positions`' refusal and the
write dispatch.
"""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import secondary3d_cases as cases
from tests import secondary3d_ref as ref
from tests import secondary_ref as ref2d

UNIT = (1, 1, 1)


# ------------------------------------------------------------------------------------------------ the restatement
def balls(seed, shape=(10, 40, 44), n=14):
    """A label stack of `n` balls of radius 1.5..3.5 voxels, labels 1..n (a later ball covers an earlier one where they meet)."""
    rng = np.random.default_rng(seed)
    grid = np.mgrid[tuple(slice(0, s) for s in shape)]
    vol = np.zeros(shape, np.uint16)
    for label in range(1, n + 1):
        centre = [rng.uniform(0, s - 1) for s in shape]
        r = rng.uniform(1.5, 3.5)
        vol[sum((g - c) ** 2 for g, c in zip(grid, centre)) <= r * r] = label
    return vol


SCIPY_RUNS = [(seed, spacing, n) for seed in range(3)
              for spacing, ns in ((UNIT, (1, 3, 5, 16)), ((3, 1, 1), (1, 3, 5, 16)), ((13, 5, 5), (5, 25, 60, 200))) for n in ns]


@functools.lru_cache(maxsize=None)
def both(seed, spacing, n):
    """(the scene, the restatement, its ties, SciPy): scipy.ndimage.distance_transform_edt(vol == 0, sampling=spacing,
    return_indices=True) and out[dist <= N] = vol[idx]."""
    vol = balls(seed)
    got, ties = ref.secondary_stack(vol, n, spacing)
    dist, idx = ndimage.distance_transform_edt(vol == 0, sampling=spacing, return_indices=True)
    return vol, got, ties, np.where(dist <= n, vol[tuple(idx)], 0).astype(np.uint16)


@pytest.mark.parametrize("seed, spacing, n", SCIPY_RUNS)
def test_restatement_against_scipy(seed, spacing, n):
    """Equal off ties; the ties are at most 5 % of the grown voxels (a condition on the scene, not a measurement)."""
    vol, got, ties, scipy_out = both(seed, spacing, n)
    grown = (got != 0) & (vol == 0)
    assert grown.sum() > 100 and np.array_equal(got[vol != 0], vol[vol != 0])
    assert np.array_equal(got[~ties], scipy_out[~ties]), f"{int((got != scipy_out)[~ties].sum())} voxels off ties differ"
    assert not ties[~grown].any() and ties.sum() <= 0.05 * grown.sum(), (int(ties.sum()), int(grown.sum()))
    # on a tie both answers are among the nearest labels, and the restatement's is the smaller
    assert (got[ties] <= scipy_out[ties]).all()


def test_scipy_differs_on_some_tie():
    """The tie rule matters: SciPy's sweep order picks the other label on some tie of these runs."""
    assert any((got != scipy_out)[ties].any() for _, got, ties, scipy_out in (both(*run) for run in SCIPY_RUNS))


@pytest.mark.parametrize("n", [1, 5, 64])
def test_one_plane_is_the_2d_restatement(n):
    vol = cases.CASES["one_plane"][0]
    assert np.array_equal(cases.want("one_plane", n)[:, 0], ref2d.secondary_labels(vol[:, 0], n))
    stack, ties = ref.secondary_stack(vol[0], n)
    tile, ties2d = ref2d.secondary_tile(vol[0, 0], n)
    assert np.array_equal(stack[0], tile) and np.array_equal(ties[0], ties2d)


def test_the_cases_hold_what_they_are_named_for():
    """The restatement on the content cases, by hand: the ties are ties and go to the smaller label."""
    want = cases.want
    assert not want("all_zero", 64).any() and np.array_equal(want("fully_labelled", 64), cases.CASES["fully_labelled"][0])
    assert want("65535_beside_1", 3)[0, 1, 1].tolist() == [1, 1, 1, 1, 1, 1, 65535, 65535, 65535, 65535, 65535, 65535]
    assert want("65535_alone", 5)[0, 4, 10, 15] == 65535 and want("65535_alone", 5)[0, 4, 10, 16] == 0
    assert want("65535_alone", 12, (3, 1, 1))[0, 8, 10, 10] == 65535 and want("65535_alone", 12, (3, 1, 1))[0, 0, 10, 11] == 0  # 144, 145
    for axis in range(3):
        for side in ("first", "second"):
            name = f"tie_along_{'zyx'[axis]}_smaller_{side}"
            assert want(name, 3)[0, 6, 6, 6] == 2 and want(name, 64)[0, 6, 6, 6] == 2
            _, ties = ref.secondary_stack(cases.CASES[name][0][0], 3)
            assert ties[6, 6, 6]
    for name in ("tie_z_against_y", "tie_z_against_x", "tie_y_against_x"):
        for suffix in ("", "_swapped"):
            assert want(name + suffix, 3)[0, 5, 5, 5] == 4 and want(name + suffix, 64)[0, 5, 5, 5] == 4
            assert ref.secondary_stack(cases.CASES[name + suffix][0][0], 3)[1][5, 5, 5]
    for name in ("diagonal_tie", "diagonal_tie_swapped"):
        assert want(name, 3)[0, 1, 1, 1] == 4 and want(name, 64)[0, 1, 1, 1] == 4
        assert ref.secondary_stack(cases.CASES[name][0][0], 3)[1][1, 1, 1]
    assert want("diagonal_tie", 2)[0, 1, 1, 1] == 0
    for name in ("anisotropic_tie", "anisotropic_tie_swapped"):
        assert want(name, 3, (3, 1, 1))[0, 1, 5, 5] == 2 and want(name, 3, (3, 1, 1))[0, 0, 5, 8] == 2
        assert ref.secondary_stack(cases.CASES[name][0][0], 3, (3, 1, 1))[1][1, 5, 5]
    # the header's worked example: (1, 5, 4) is 10 through the plane and 16 along the row
    w = want("anisotropic_tie", 3, (3, 1, 1))[0]
    assert w[1, 5, 4] == 0 and w[0, 5, 2] == 7 and w[2, 5, 8] == 2 and w[0, 5, 1] == 0
    assert want("anisotropic_tie", 2, (3, 1, 1))[0, 1, 5, 5] == 0
    for n, spacing in ((5, UNIT), (10, (2, 2, 2))):
        w = want("tie_at_the_last_step", n, spacing)[0]
        assert w[4, 6, 6] == 4 and w[4, 6, 16] == 4 and w[8, 6, 2] == 3 and w[4, 6, 5] == 0
    assert want("partial_sum_above_the_limit", 5)[0, 0, 0, 0] == 0 and want("partial_sum_above_the_limit", 6)[0, 0, 0, 0] == 6  # 32
    w = want("n255_on_4_4_4", 255, (4, 4, 4))[0]
    assert w[63, 0, 0] == 6 and w[63, 9, 0] == 6 and w[63, 10, 0] == 0 and w[63, 62, 0] == 0  # 63504, 64800, 65104; 2 * 252^2 wraps
    assert w[0, 63, 0] == 6 and w[0, 63, 2] == 6 and w[9, 63, 2] == 6 and w[10, 63, 0] == 0 and w[63, 63, 2] == 0  # 63504, 63568, 64864, 65104
    assert want("m_65025_is_reached", 255, (5, 5, 5))[0, 0, 0, 0] == 4 and want("m_65025_is_reached", 254, (5, 5, 5))[0, 0, 0, 0] == 0
    assert ref.secondary_stack(cases.CASES["m_65025_is_reached"][0][0], 255, (5, 5, 5))[1][0, 0, 0]
    for n, spacing in cases.CASES["batch_edges"][1]:
        w = want("batch_edges", n, spacing)
        assert not w[1].any() and w[0].any() and w[2].any()
    corners = want("eight_corners", 64)[0]
    assert len(np.unique(corners)) == 8 and corners.all() and corners[0, 0, 10] == 2 and corners[4, 0, 10] == 65535


# ------------------------------------------------------------------------------------------------ the arguments
def test_secondary_volume_args():
    from aliby_amd.extraction.features import secondary_volume_args as args

    assert args(5) == (5, (1, 1, 1)) and args(5.0, [13, 5, 5]) == (5, (13, 5, 5))
    assert args(255, (4, 4, 4)) == (255, (4, 4, 4)) and args(np.int64(64), np.array([1, 1, 1])) == (64, (1, 1, 1))
    assert args(200, (13, 5, 5)) == (200, (13, 5, 5)) and args(1, (255, 255, 255)) == (1, (255, 255, 255))
    assert all(type(v) is int for v in (args(np.int32(7), np.array([2, 3, 4]))[0], *args(np.int32(7), np.array([2, 3, 4]))[1]))
    for bad in (0, 256, -3, True, 2.5, None, "5", float("nan")):
        with pytest.raises(ValueError, match="1..255"):
            args(bad)
    for bad in ((1, 1), (1, 1, 1, 1), (0, 1, 1), (256, 1, 1), (1.0, 1.0, 1.0), (0.6, 0.23, 0.23), (True, 1, 1), "111", None, 1,
                ("1", "1", "1"), (1, 1, None)):
        with pytest.raises(ValueError, match="spacing"):
            args(5, bad)
    for n, spacing in ((65, UNIT), (255, (3, 3, 3)), (130, (2, 13, 13)), (200, (13, 5, 3))):
        with pytest.raises(ValueError, match="64 voxels"):
            args(n, spacing)


# ------------------------------------------------------------------------------------------------ the builder
ARGUMENT_SETS = [
    dict(),
    dict(channels_to_segment={"nuclei": 1}, secondary={"cell": ("nuclei", 10)}),
    dict(volume_features=("intensity3d",), secondary={"ring": ("nuclei", 3)}),
    dict(channels_to_segment={"nuclei": 1}, secondary={"cell": ("nuclei", 10)}, tertiary={"cytoplasm": ("cell", "nuclei")},
         relate=[("nuclei", "cell")], volume_features=("intensity3d",)),
    dict(volume_features=("intensity3d",), relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}, volume_relate=True),
]
ON = dict(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1], secondary={"cell": ("nuclei", 10)},
          tertiary={"cytoplasm": ("cell", "nuclei")}, relate=[("nuclei", "cell")], volume_features=("intensity3d",), volume_relate=True)


@pytest.mark.parametrize("kw", ARGUMENT_SETS)
def test_builder_without_the_keyword_is_unchanged(kw):
    from aliby_amd.pipe_builder import build_pipeline_steps

    plain, off = build_pipeline_steps(**kw), build_pipeline_steps(**kw, volume_secondary=False)
    assert plain == off and repr(plain) == repr(off)
    assert not any(n.startswith("volumesecondary_") for n in (*plain["steps"], *plain["passed_data"], *plain["save"]))
    for name in kw.get("secondary", ()):
        assert f"volume_{name}" not in plain["steps"]


def test_the_old_refusal_still_holds():
    from aliby_amd.pipe_builder import build_pipeline_steps

    for vs in ({}, {"volume_secondary": False}):
        with pytest.raises(ValueError, match="no volume form"):
            build_pipeline_steps(**ON, **vs)


@pytest.mark.parametrize("volume_secondary, distance, spacing", [(True, 10, (1, 1, 1)), ((13, 5), 50, (13, 5, 5)), ([2, 1], 10, (2, 1, 1))])
def test_builder_with_the_keyword(volume_secondary, distance, spacing):
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(**ON, volume_secondary=volume_secondary)
    assert list(p["steps"]) == ["tile", "segment_nuclei", "secondary_cell", "tertiary_cytoplasm", "volumesecondary_cell",
                                "volumetertiary_cytoplasm", "extract_nuclei", "extract_cell", "extract_cytoplasm",
                                "extractmulti_nuclei", "extractmulti_cell", "extractmulti_cytoplasm",
                                "extractrelate_nuclei", "extractrelate_cell", "volume_nuclei", "volume_cell", "volume_cytoplasm",
                                "volumerelate_nuclei", "volumerelate_cell"]
    assert p["steps"]["volumesecondary_cell"] == {"primary": "segment_nuclei", "distance": distance, "spacing": spacing}
    assert p["steps"]["volumetertiary_cytoplasm"] == {"outer": "volumesecondary_cell", "inner": "segment_nuclei", "shrink_inner": True}
    assert p["steps"]["volume_cell"] == {"tree": p["steps"]["volume_nuclei"]["tree"], "volume_from": "volumesecondary_cell",
                                         "kwargs": p["steps"]["volume_nuclei"]["kwargs"]}
    assert p["steps"]["volume_cell"]["tree"] is p["steps"]["volume_nuclei"]["tree"]  # the shared volume tree
    assert p["steps"]["volume_cytoplasm"]["volume_from"] == "volumetertiary_cytoplasm"
    assert p["steps"]["volumerelate_nuclei"] == {"volume_from": "segment_nuclei", "others": {"cell": "volumesecondary_cell"},
                                                 "spacing": (1.0, 1.0, 1.0)}
    assert p["steps"]["volumerelate_cell"] == {"volume_from": "volumesecondary_cell", "others": {"nuclei": "segment_nuclei"},
                                               "spacing": (1.0, 1.0, 1.0)}
    assert p["passed_data"]["volume_cell"] == [("pixels", "tile")] and p["passed_data"]["volume_cytoplasm"] == [("pixels", "tile")]
    assert not any(n.startswith(("volumesecondary_", "volumetertiary_", "volumerelate_")) for n in p["passed_data"])
    assert p["steps"]["segment_nuclei"]["segmenter_kwargs"]["do_3D"] is True
    validate_pipeline(p)
    # everything of the dict without the volume keywords is still there, unchanged
    plain = build_pipeline_steps(**{k: v for k, v in ON.items() if k != "volume_relate"})
    for key in plain["steps"]:
        assert p["steps"][key] == plain["steps"][key]
    assert {k: v for k, v in p["passed_data"].items() if k not in ("volume_cell", "volume_cytoplasm")} == plain["passed_data"]
    assert p["save"] == plain["save"] == ["segment_nuclei", "secondary_cell", "tertiary_cytoplasm"]
    assert p["passed_methods"] == plain["passed_methods"]


def test_builder_with_the_keyword_alone():
    """Without volume_relate: the grown volume and its rows, no tertiary volume and no relate3d rows."""
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    kw = dict(channels_to_segment={"nuclei": 0}, volume_features=("intensity3d",), secondary={"cell": ("nuclei", 4), "halo": ("nuclei", 64)},
              tertiary={"rest": ("cell", "nuclei")})
    off = build_pipeline_steps(**kw)
    p = build_pipeline_steps(**kw, volume_secondary=True)
    assert [n for n in p["steps"] if n.startswith("volume")] == ["volumesecondary_cell", "volumesecondary_halo", "volume_nuclei",
                                                                 "volume_cell", "volume_halo"]
    assert list(p["steps"]).index("volumesecondary_cell") == list(p["steps"]).index("tertiary_rest") + 1
    assert p["steps"]["volumesecondary_halo"] == {"primary": "segment_nuclei", "distance": 64, "spacing": (1, 1, 1)}
    assert [n for n in off["steps"] if n.startswith("volume")] == ["volume_nuclei"]
    validate_pipeline(p)


VF = dict(channels_to_segment={"nuclei": 1}, volume_features=("intensity3d",))


@pytest.mark.parametrize("kw, match", [
    (dict(channels_to_segment={"nuclei": 1}, secondary={"cell": ("nuclei", 10)}, volume_secondary=True), "volume_features"),
    (dict(**VF, volume_secondary=True), "secondary entry"),
    (dict(**VF, secondary={}, volume_secondary=(13, 5)), "secondary entry"),
    *[(dict(**VF, secondary={"cell": ("nuclei", 10)}, volume_secondary=bad), "volume_secondary must be")
      for bad in (1, 0, None, "yes", (13,), (13, 5, 5), (13.0, 5), (0, 5), (13, -5), (True, 1), 2.6)],
    (dict(**VF, secondary={"cell": ("nuclei", 52)}, volume_secondary=(13, 5)), "1..255"),  # q N = 260
    (dict(**VF, secondary={"cell": ("nuclei", 40)}, volume_secondary=(1, 2)), "64 voxels"),  # 80 planes
    (dict(**VF, secondary={"ok": ("nuclei", 3), "cell": ("nuclei", 10)}, volume_secondary=(256, 1)), "spacing"),
])
def test_builder_refusals(kw, match):
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError, match=match) as e:
        build_pipeline_steps(**kw)
    assert "volume_secondary" in str(e.value)


# ------------------------------------------------------------------------------------------------ validation, dispatch
def test_prefixes_and_write_dispatch():
    from aliby_amd import pipe
    from aliby_amd.io.write import dispatch_write_fn, write_ndarray
    from aliby_amd.pipe_core import _VOLUME_SOURCES, _VolumeSecondary

    prefixes = [p for p, _ in pipe._PREFIXES]
    assert "volumesecondary_" in prefixes and "volumesecondary_" in _VOLUME_SOURCES
    assert not "volumesecondary_".startswith(("extract", "volume_", "secondary_"))
    assert dispatch_write_fn("volumesecondary_x") is write_ndarray
    step = pipe.init_step("volumesecondary_cell", {"primary": "segment_nuclei", "distance": 10})
    assert isinstance(step, _VolumeSecondary) and step.last_volume is None and (step.distance, step.spacing) == (10, (1, 1, 1))


def test_validate_pipeline_checks_the_wiring():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    def broken(change):
        p = build_pipeline_steps(**ON, volume_secondary=True)
        change(p["steps"])
        return p

    with pytest.raises(ValueError, match="volumesecondary_cell.*primary"):
        validate_pipeline(broken(lambda s: s["volumesecondary_cell"].pop("primary")))
    with pytest.raises(ValueError, match="segment_membrane"):  # a source that is no step
        validate_pipeline(broken(lambda s: s["volumesecondary_cell"].update(primary="segment_membrane")))
    with pytest.raises(ValueError, match="segment step"):
        validate_pipeline(broken(lambda s: s["volumesecondary_cell"].update(primary="secondary_cell")))
    with pytest.raises(ValueError, match="volumesecondary_cell"):  # volume_cell and the others have lost their source
        validate_pipeline(broken(lambda s: s.pop("volumesecondary_cell")))
    with pytest.raises(ValueError, match="volumesecondary_cell.*do_3D"):
        validate_pipeline(broken(lambda s: s["segment_nuclei"]["segmenter_kwargs"].pop("do_3D")))

    def late(steps):  # the grown volume after the steps that read it
        steps["volumesecondary_cell"] = steps.pop("volumesecondary_cell")

    with pytest.raises(ValueError, match="before"):
        validate_pipeline(broken(late))

    def late_for_the_volume_step_alone(steps):  # only volume_cell reads it, and runs first
        for name in ("volumetertiary_cytoplasm", "volume_cytoplasm", "volumerelate_nuclei", "volumerelate_cell"):
            del steps[name]
        steps["volumesecondary_cell"] = steps.pop("volumesecondary_cell")

    with pytest.raises(ValueError, match="volume_cell.*before"):
        validate_pipeline(broken(late_for_the_volume_step_alone))

    def late_primary(steps):  # the segment step after the step that grows its volume
        steps["segment_nuclei"] = steps.pop("segment_nuclei")

    with pytest.raises(ValueError, match="volumesecondary_cell.*before"):
        validate_pipeline(broken(late_primary))


def test_run_positions_refuses_the_step(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(NotImplementedError, match="run_pipeline_and_post"):
        parallel.run_positions([build_pipeline_steps(**ON, volume_secondary=True)], ["p0"], tmp_path)
    # by the step's own prefix, not only through the volume refusal: a dict by hand without do_3D and without a volume_ step
    p = build_pipeline_steps()
    p["steps"]["volumesecondary_cell"] = {"primary": "segment_nuclei", "distance": 10}
    with pytest.raises(NotImplementedError, match="volumesecondary_cell.*volumesecondary_"):
        parallel.run_positions([p], ["p0"], tmp_path)
    assert not list(tmp_path.iterdir())


# ------------------------------------------------------------------------------------------------ the step
class Segment:
    last_volume = None

    def __init__(self, volume=None, counts=None):
        if volume is not None:
            self.last_volume = (torch.from_numpy(np.ascontiguousarray(volume).view(np.int16)).view(torch.uint16), np.asarray(counts))


def test_volumesecondary_step_errors():
    from aliby_amd.pipe import init_step

    ok = {"primary": "segment_nuclei", "distance": 10}
    for params, match in (({"distance": 10}, "primary"), ({"primary": "segment_nuclei"}, "distance"),
                          ({**ok, "primary": "tile"}, "segment step"), ({**ok, "primary": 3}, "segment step"),
                          ({**ok, "primary": "secondary_cell"}, "segment step"), ({**ok, "distance": 0}, "1..255"),
                          ({**ok, "distance": 256}, "1..255"), ({**ok, "distance": True}, "1..255"), ({**ok, "distance": "10"}, "1..255"),
                          ({**ok, "distance": None}, "1..255"), ({**ok, "distance": 65}, "64 voxels"),
                          ({**ok, "spacing": (1.0, 1.0, 1.0)}, "spacing"), ({**ok, "spacing": (13, 5)}, "spacing"),
                          ({**ok, "spacing": None}, "spacing"), ({**ok, "distance": 200, "spacing": (13, 5, 3)}, "64 voxels"),
                          ({**ok, "spacing": (1, 1, 1), "shrink_inner": True}, "unknown"), ({**ok, "kwargs": {}}, "unknown")):
        with pytest.raises(ValueError, match=match) as e:
            init_step("volumesecondary_cell", params, {})
        assert "volumesecondary_cell" in str(e.value)
    for source in ("segment_nuclei", "volumetertiary_rest", "volumesecondary_inner"):  # every step that keeps a volume
        assert init_step("volumesecondary_cell", {**ok, "primary": source}, {}).primary == source
    step = init_step("volumesecondary_cell", {**ok, "distance": 50.0, "spacing": [13, 5, 5]}, {})
    assert (step.distance, step.spacing) == (50, (13, 5, 5)) and type(step.distance) is int
    # at run time: the source is missing, is no segmenter, or kept no volume (every one stops before the launch)
    vol = cases.CASES["diagonal_tie"][0]
    step = init_step("volumesecondary_cell", dict(ok), {"segment_cell": Segment(vol, [9])})
    with pytest.raises(ValueError, match="volumesecondary_cell.*segment_nuclei"):
        step()
    step = init_step("volumesecondary_cell", dict(ok), {"segment_nuclei": object()})
    with pytest.raises(ValueError, match="not a segment step"):
        step()
    step = init_step("volumesecondary_cell", dict(ok), {"segment_nuclei": Segment()})
    with pytest.raises(ValueError, match="segment_nuclei.*do_3D"):
        step()
    assert step.last_volume is None


def test_volume_steps_take_a_volumesecondary_source():
    from aliby_amd.pipe import init_step

    tree = {"None": {"None": ["projection3d"]}}

    class Pixels:
        shape = (1, 2, 3, 6, 8)

    grown = init_step("volumesecondary_cell", {"primary": "segment_nuclei", "distance": 3}, {})
    done = {"volumesecondary_cell": grown, "segment_nuclei": Segment()}
    step = init_step("volume_cell", {"tree": tree, "volume_from": "volumesecondary_cell"}, done)
    with pytest.raises(ValueError, match="volume_cell.*kept no volume"):  # the step has not run (or failed) at this timepoint
        step(pixels=Pixels())
    grown.last_volume = (torch.zeros((1, 3, 6, 9), dtype=torch.uint16), np.asarray([2]))
    with pytest.raises(ValueError, match="do not match"):
        step(pixels=Pixels())
    tertiary = init_step("volumetertiary_cytoplasm", {"outer": "volumesecondary_cell", "inner": "segment_nuclei"}, done)
    with pytest.raises(ValueError, match="segment_nuclei.*do_3D"):
        tertiary()
    done["segment_nuclei"] = Segment(np.zeros((1, 3, 6, 8), np.uint16), [2])
    with pytest.raises(ValueError, match="do not match"):  # [1,3,6,9] against [1,3,6,8]
        tertiary()
    relate = init_step("volumerelate_nuclei", {"volume_from": "segment_nuclei", "others": {"cell": "volumesecondary_cell"}}, done)
    with pytest.raises(ValueError, match="do not match"):
        relate()
