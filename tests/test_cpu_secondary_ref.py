"""
tests/secondary_ref.py, the brute-force restatement of the `secondary` definition ("Distance - N" of CellProfiler's
IdentifySecondaryObjects), held against the function CellProfiler calls — scipy.ndimage.distance_transform_edt with return_indices
and the index gather — on every pixel that is not an exact tie, and pinned to hand values; then the surface that needs no device: the
distance check, the builder's dicts and refusals, the step initialiser's errors, validate_pipeline and the run_positions refusal.
"""
import functools

import numpy as np
import pytest
from scipy import ndimage

from tests import secondary_ref as ref

SCENE_SEEDS = (0, 1, 2, 3, 4, 5)
DISTANCES = (1, 3, 5, 16)


def disc_scene(seed, shape=(96, 128), n=14):
    """14 random discs (radius 3..9), label k + 1 for disc k, a later disc painted over an earlier one."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    lab = np.zeros(shape, np.uint16)
    for k in range(n):
        cy, cx, r = rng.integers(0, shape[0]), rng.integers(0, shape[1]), rng.integers(3, 10)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    return lab


def scipy_expand(labels, distance):
    """CellProfiler's code for "Distance - N" (and skimage.segmentation.expand_labels)."""
    dist, (i, j) = ndimage.distance_transform_edt(labels == 0, return_indices=True)
    out = np.zeros_like(labels)
    grown = dist <= distance
    out[grown] = labels[i[grown], j[grown]]
    return out


# ------------------------------------------------------------------------------------------------ the restatement
@functools.lru_cache(maxsize=None)
def _compared(seed, n):
    """(labels, restatement, tie mask, SciPy's result) of one scene at one distance, computed once."""
    labels = disc_scene(seed)
    out, ties = ref.secondary_tile(labels, n)
    return labels, out, ties, scipy_expand(labels, n)


@pytest.mark.parametrize("n", DISTANCES)
@pytest.mark.parametrize("seed", SCENE_SEEDS)
def test_restatement_is_scipy_off_ties(seed, n):
    labels, out, ties, sp = _compared(seed, n)
    assert ((out != 0) & (labels == 0)).any() and (out == 0).any()  # something grows, and the cap leaves something out
    assert np.array_equal(sp != 0, out != 0)  # the same pixels grow: the distance itself knows no ties
    assert np.array_equal(out[~ties], sp[~ties])
    assert not ties[labels != 0].any()
    # on a tie SciPy's label is one of the tied ones: a pixel of that label lies at exactly the minimum distance, and the
    # restatement's label is the smallest of them
    d2 = ndimage.distance_transform_edt(labels == 0) ** 2
    for y, x in zip(*np.nonzero(ties)):
        m = int(round(d2[y, x]))
        qy, qx = np.nonzero(labels == sp[y, x])
        assert ((qy - y) ** 2 + (qx - x) ** 2 == m).any()
        assert out[y, x] <= sp[y, x]


@pytest.mark.parametrize("n", DISTANCES)
def test_ties_are_rare_and_the_rule_bites(n):
    """Over the six scenes the tie pixels, which the comparison with SciPy leaves out, are at most 2 % of the expanded pixels (the
    exclusion cannot hide a failure), and on some of them SciPy does pick the other label (the rule is not vacuous)."""
    expanded = tied = differs = 0
    for seed in SCENE_SEEDS:
        labels, out, ties, sp = _compared(seed, n)
        expanded += int(((out != 0) & (labels == 0)).sum())
        tied += int(ties.sum())
        differs += int((sp[ties] != out[ties]).sum())
    print(f"N {n}: expanded {expanded}, ties {tied} ({100 * tied / expanded:.2f} %), SciPy picks the other label on {differs}")
    assert tied <= 0.02 * expanded
    assert 0 < differs <= tied


def test_hand_values():
    lone = np.zeros((12, 12), np.uint16)
    lone[0, 0] = 9
    out, ties = ref.secondary_tile(lone, 5)
    assert out[3, 4] == 9 and out[4, 3] == 9 and out[4, 4] == 0 and out[5, 0] == 9 and out[5, 1] == 0 and out[0, 6] == 0
    assert not ties.any() and int((out == 9).sum()) == int(((np.mgrid[:12, :12] ** 2).sum(0) <= 25).sum())
    row = np.array([[7, 0, 3]], np.uint16)
    out, ties = ref.secondary_tile(row, 1)
    assert out.tolist() == [[7, 3, 3]] and ties.tolist() == [[False, True, False]]
    # the header's row: pixel 2 is 2 from either object
    out, _ = ref.secondary_tile(np.array([[7, 0, 0, 0, 3, 0, 0, 0, 0]], np.uint16), 2)
    assert out.tolist() == [[7, 7, 3, 3, 3, 3, 3, 0, 0]]
    # 65535 is a label; an empty tile and a full one come back as they are
    edge = np.array([[65535, 0, 0, 1]], np.uint16)
    assert ref.secondary_tile(edge, 1)[0].tolist() == [[65535, 65535, 1, 1]]
    assert not ref.secondary_tile(np.zeros((3, 4), np.uint16), 64)[0].any()
    full = np.arange(1, 13, dtype=np.uint16).reshape(3, 4)
    assert np.array_equal(ref.secondary_tile(full, 7)[0], full)
    # tiles are apart
    pair = np.zeros((2, 3, 3), np.uint16)
    pair[0, 2, 1] = 4
    assert not ref.secondary_labels(pair, 3)[1].any() and ref.secondary_labels(pair, 3)[0].all()


# ------------------------------------------------------------------------------------------------ the surface without a device
def test_distance_check():
    from aliby_amd.extraction import features

    assert features.SECONDARY_MAX_DISTANCE == 64
    assert [features.secondary_distance(d) for d in (1, 64, np.int64(7), 5.0)] == [1, 64, 7, 5]
    for bad in (0, 65, -1, True, False, 2.5, float("nan"), None, "5", (5,)):
        with pytest.raises(ValueError, match="1..64"):
            features.secondary_distance(bad)


def test_library_binds_the_entries():
    from aliby_amd import _lib

    for name in ("aliby_secondary_labels", "aliby_secondary_workspace_bytes"):
        assert name in _lib.exported_symbols()


def test_builder_unchanged_without_the_keyword():
    from aliby_amd.pipe_builder import build_pipeline_steps

    for kw in ({}, dict(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}),
               dict(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1])):
        plain = build_pipeline_steps(**kw)
        assert build_pipeline_steps(secondary=None, **kw) == plain
        assert repr(build_pipeline_steps(secondary=None, **kw)) == repr(plain)  # order included
        assert not any(k.startswith("secondary") for k in (*plain["steps"], *plain["passed_data"], *plain["save"]))
    with pytest.raises(TypeError):  # keyword-only
        build_pipeline_steps(None, None, ("sizeshape",), None, None, None, None, None, None, {"cell": ("nuclei", 10)})


def test_builder_with_the_keyword():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1], secondary={"cell": ("nuclei", 10)},
                             tertiary={"cytoplasm": ("cell", "nuclei")}, relate=[("nuclei", "cell")])
    assert list(p["steps"]) == ["tile", "segment_nuclei", "secondary_cell", "tertiary_cytoplasm",
                                "extract_nuclei", "extract_cell", "extract_cytoplasm",
                                "extractmulti_nuclei", "extractmulti_cell", "extractmulti_cytoplasm",
                                "extractrelate_nuclei", "extractrelate_cell"]
    assert p["steps"]["secondary_cell"] == {"distance": 10}
    assert p["steps"]["extract_cell"] is p["steps"]["extract_nuclei"]  # the shared spec dicts
    assert p["steps"]["extractmulti_cell"] is p["steps"]["extractmulti_nuclei"]
    pd = p["passed_data"]
    assert pd["secondary_cell"] == [("masks", "segment_nuclei", "primary")]
    assert pd["tertiary_cytoplasm"] == [("masks", "secondary_cell", "outer"), ("masks", "segment_nuclei", "inner")]
    assert pd["extract_cell"] == pd["extractmulti_cell"] == [("masks", "secondary_cell"), ("pixels", "tile")]
    assert pd["extract_cytoplasm"] == [("masks", "tertiary_cytoplasm"), ("pixels", "tile")]
    assert pd["extractrelate_nuclei"] == [("masks", "segment_nuclei"), ("masks", "secondary_cell", "masks_cell")]
    assert pd["extractrelate_cell"] == [("masks", "secondary_cell"), ("masks", "segment_nuclei", "masks_nuclei")]
    assert p["save"] == ["segment_nuclei", "secondary_cell", "tertiary_cytoplasm"]
    assert p["passed_methods"] == {"segment_nuclei": ("tile", "get_fczyx")}
    validate_pipeline(p)
    # everything the plain dict has is still there, unchanged
    plain = build_pipeline_steps(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1])
    for key in plain["steps"]:
        assert p["steps"][key] == plain["steps"][key]
    for key in plain["passed_data"]:
        assert pd[key] == plain["passed_data"][key]
    # a secondary set beside two segmented ones; a float that holds an integer is that integer
    q = build_pipeline_steps(secondary={"ring": ("cell", 3.0)})
    assert list(q["steps"])[:4] == ["tile", "segment_nuclei", "segment_cell", "secondary_ring"]
    assert q["steps"]["secondary_ring"] == {"distance": 3} and q["save"] == ["segment_nuclei", "segment_cell", "secondary_ring"]
    assert q["passed_data"]["secondary_ring"] == [("masks", "segment_cell", "primary")]
    validate_pipeline(q)
    # steps_to_write still overrides the save list
    assert build_pipeline_steps(secondary={"ring": ("cell", 3)}, steps_to_write=["secondary_ring"])["save"] == ["secondary_ring"]
    # the volume keywords still work beside a secondary set that does not reach them
    v = build_pipeline_steps(secondary={"ring": ("cell", 3)}, volume_features=["intensity3d"], relate=[("nuclei", "cell")],
                             volume_relate=True)
    assert "secondary_ring" in v["steps"] and "volume_ring" not in v["steps"] and "volumerelate_cell" in v["steps"]


@pytest.mark.parametrize("kw", [
    dict(secondary={"cell": ("nuclei", 10)}),                                   # already a segmented object set
    dict(secondary={"ring": ("nuclei", 3)}, tertiary={"ring": ("cell", "nuclei")}),   # already a secondary object set
    dict(secondary={"ring": ("vacuole", 3)}),                                   # the primary is not an object set
    dict(secondary={"ring": ("ring", 3)}),
    dict(secondary={"ring": ("nuclei", 3), "halo": ("ring", 3)}),               # the primary is not a SEGMENTED object set
    dict(secondary={"ring": ("nuclei",)}),                                      # malformed entries
    dict(secondary={"ring": "nuclei"}),
    dict(secondary={"ring": ("nuclei", 3, 4)}),
    dict(secondary={"ring": ("nuclei", 0)}),
    dict(secondary={"ring": ("nuclei", 65)}),
    dict(secondary={"ring": ("nuclei", 2.5)}),
    dict(secondary={"ring": ("nuclei", True)}),
    dict(secondary={"ri_ng": ("nuclei", 3)}),
    dict(secondary=[("ring", "nuclei", 3)]),
    dict(secondary={"ring": ("nuclei", 3)}, volume_features=["intensity3d"], volume_relate=True, relate=[("ring", "nuclei")]),
    dict(secondary={"ring": ("nuclei", 3)}, volume_features=["intensity3d"], volume_relate=True, tertiary={"rest": ("ring", "nuclei")}),
])
def test_builder_refusals(kw):
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError):
        build_pipeline_steps(**kw)


def test_write_dispatch_knows_secondary():
    from aliby_amd.io.write import dispatch_write_fn, write_ndarray

    assert dispatch_write_fn("secondary_cell") is write_ndarray


def test_init_step_errors():
    from aliby_amd.pipe import init_step

    with pytest.raises(ValueError, match="unknown"):
        init_step("secondary_cell", {"distance": 5, "method": "propagation"})
    with pytest.raises(ValueError, match="distance"):
        init_step("secondary_cell", {})
    for bad in (0, 65, 2.5, True, "5"):
        with pytest.raises(ValueError, match="secondary_cell.*1..64"):
            init_step("secondary_cell", {"distance": bad})
    # a step whose aliased input never arrives says so (before it touches a device)
    step = init_step("secondary_cell", {"distance": 5})
    with pytest.raises(ValueError, match="primary"):
        step()
    with pytest.raises(ValueError, match="primary"):
        step(primary=None)


def test_validate_pipeline_checks_the_alias():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(secondary={"ring": ("nuclei", 3)})
    validate_pipeline(p)
    p["passed_data"]["secondary_ring"] = [("masks", "segment_nuclei")]  # alias lost
    with pytest.raises(ValueError, match="primary"):
        validate_pipeline(p)
    p = build_pipeline_steps(secondary={"ring": ("nuclei", 3)})
    del p["passed_data"]["secondary_ring"]
    with pytest.raises(ValueError, match="primary"):
        validate_pipeline(p)


def test_run_positions_refuses_a_secondary_step(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(NotImplementedError, match="no batched form of step 'secondary_ring'.*position by position"):
        parallel.run_positions([build_pipeline_steps(secondary={"ring": ("nuclei", 3)})], ["p0"], tmp_path)
