"""
The `propagate` definition without a device: the two restatements of tests/propagate_ref.py (a heap Dijkstra in Python integers,
the definition itself, and a NumPy Jacobi iteration on packed keys) agree bit for bit; the hand values of include/aliby_hip.h; what
the metric does on a ridge, a wall, a flat image; "Distance - B"; and the surface that needs no GPU (argument checks, exported
symbols, the builder's `propagate` keyword, the `propagate_` step's wiring).
"""
import ctypes

import numpy as np
import pytest

from tests import propagate_cases as pc
from tests import propagate_ref as ref
from tests import secondary_ref


# ------------------------------------------------------------------------------------------------ the two restatements
def _both(primary, image, **kw):
    out, D = ref.propagate_tile(primary, image, **kw)
    fast, fast_D, sweeps = ref.propagate_jacobi(primary, image, **kw)
    assert out.dtype == fast.dtype == np.uint16 and D.dtype == fast_D.dtype == np.uint64
    assert np.array_equal(out, fast) and np.array_equal(D, fast_D)
    assert np.array_equal(out[primary != 0], primary[primary != 0]) and not D[primary != 0].any()
    assert np.array_equal(out == 0, D == ref.NONE)
    return out, D, sweeps


@pytest.mark.parametrize("shape, seed", [((37, 53), 1), ((64, 96), 2), ((40, 70), 3)])
@pytest.mark.parametrize("kw", [{}, {"threshold": 3000}, {"threshold": 2000, "distance": 9}], ids=["plain", "threshold", "both"])
def test_the_restatements_agree_on_random_scenes(shape, seed, kw):
    primary, image = pc.scene((1, *shape), 6, seed, islands=2)
    out, _, sweeps = _both(primary[0], image[0], **kw)
    assert sweeps > 3 and (out != 0).sum() > (primary != 0).sum()
    if kw == {"threshold": 3000}:
        # the threshold leaves islands: passable pixels that no seed reaches (more than the odd noise pixel: a blob)
        assert ((out == 0) & ref.passable(primary[0], image[0], **kw)).sum() > 10


def test_the_restatements_agree_on_a_serpentine_corridor():
    primary, image = pc.serpentine(21, 41, 3)
    out, D, sweeps = _both(primary[0], image[0], threshold=1)
    assert sweeps > 200  # the one path runs the corridor's whole length
    assert out[19, 20] == 5 and not out[2, :38].any()  # the last corridor is reached, the walls are not
    assert D[19, 20] > D[0, 40] > 0


# ------------------------------------------------------------------------------------------------ hand values
def test_hand_values():
    assert ref.lambda2(0.05, 65535) == 10737091
    assert ref.lambda2(0.0) == 0 and ref.lambda2(16.0) == (16 * 65535) ** 2 and ref.lambda2(0.05, 255) == 163  # 12.75^2 = 162.5625
    flat = pc.flat((3, 5))
    assert ref.weight(flat, (1, 1), (1, 2), 10737091) == 52428 and ref.weight(flat, (1, 1), (2, 2), 10737091) == 74144
    assert 52428 ** 2 <= 256 * 10737091 < 52429 ** 2 and 74144 ** 2 <= 512 * 10737091 < 74145 ** 2
    row = np.array([[7, 0, 0, 0, 0, 0, 0, 0, 3]], np.uint16)
    out, D, _ = _both(row, pc.flat((1, 9)))
    assert out[0].tolist() == [7, 7, 7, 7, 3, 3, 3, 3, 3]  # the middle pixel is a tie and takes 3
    assert D[0].tolist() == [0, 52428, 104856, 157284, 209712, 157284, 104856, 52428, 0]
    # the vectorised weights are the scalar ones, sentinel included
    image = pc.scene((1, 9, 11), 2, 4)[1][0]
    ok = np.ones(image.shape, bool)
    ok[4, 5] = False
    w = ref.edge_weights(image, ok, 10737091)
    for k, (dy, dx) in enumerate(((0, 1), (1, -1), (1, 0), (1, 1))):
        for y in range(9):
            for x in range(11):
                qy, qx = y + dy, x + dx
                there = 0 <= qy < 9 and 0 <= qx < 11 and ok[y, x] and ok[qy, qx]
                assert int(w[k, y, x]) == (ref.weight(image, (y, x), (qy, qx), 10737091) if there else ref.NOEDGE)


def test_pair_difference_at_a_corner_clamps_each_coordinate():
    image = np.array([[10, 13, 19, 40], [100, 104, 111, 150], [7, 7, 7, 7]], np.uint16)
    # p = (0, 0), q = (0, 1): rows -1 and 0 both read row 0; p's columns are 0, 0, 1 and q's 0, 1, 2
    by_hand = 2 * (abs(10 - 10) + abs(10 - 13) + abs(13 - 19)) + (abs(100 - 100) + abs(100 - 104) + abs(104 - 111))
    assert ref.pair_difference(image, (0, 0), (0, 1)) == by_hand == 29
    assert ref.pair_difference(image, (0, 1), (0, 0)) == by_hand  # symmetric
    # the far corner, a diagonal step: q = (2, 3) from p = (1, 2); rows 0,1,2 against 1,2,2 and columns 1,2,3 against 2,3,3
    rows, cols = ((0, 1), (1, 2), (2, 2)), ((1, 2), (2, 3), (3, 3))
    want = sum(abs(int(image[a, c]) - int(image[b, d])) for a, b in rows for c, d in cols)
    assert ref.pair_difference(image, (1, 2), (2, 3)) == want
    assert ref.weight(image, (0, 0), (0, 1), 0) == 16 * 29  # lambda2 = 0: the weight is P in sixteenths


def test_a_ridge_moves_the_boundary_and_a_flat_image_splits_at_the_midline():
    primary, image = pc.ridge()
    on_ridge = _both(primary[0], image[0])[0]
    on_flat = _both(primary[0], pc.flat((21, 40), 2000))[0]
    assert (on_flat[:, :20] == 4).all() and (on_flat[:, 20:] == 9).all()  # 40 columns, seeds at 0 and 39: the tie column... has none
    assert (on_ridge[:, :12] == 4).all() and (on_ridge[:, 13:] == 9).all()  # the boundary sits on the ridge at column 12
    assert on_ridge.all()


def test_a_threshold_wall_leaves_the_far_side_empty():
    primary, image = pc.wall()
    out = _both(primary[0], image[0], threshold=1000)[0]
    assert (out[:, :30] == 3).all() and not out[:, 30:].any()
    assert ref.passable(primary[0], image[0], 1000)[10:20, 55:65].all()  # the island is passable, and nothing arrives
    assert _both(primary[0], image[0], threshold=0)[0].all()  # without the threshold the wall is only expensive


def test_lambda_zero_on_a_flat_image_floods_each_component_with_its_smallest_label():
    image = pc.flat((12, 30))
    primary = np.zeros((12, 30), np.uint16)
    primary[2, 2], primary[3, 5], primary[9, 25], primary[8, 27] = 9, 4, 65535, 8
    whole, D, _ = _both(primary, image, regularization=0.0)  # one component: the tile
    assert whole[2, 2] == 9 and whole[9, 25] == 65535 and whole[8, 27] == 8  # labelled pixels keep their label
    assert (whole[primary == 0] == 4).all() and not D.any()
    # two components: the reach of either pair of seeds, three pixels out
    out, D, _ = _both(primary, image, regularization=0.0, distance=3)
    left, right = out[:, :15], out[:, 15:]
    assert not out[:, 9:21].any() and (left != 0).sum() > 29 and (right != 0).sum() > 29  # (a lone pixel reaches 29)
    assert set(left[(left != 0) & (primary[:, :15] == 0)].tolist()) == {4} and set(right[(right != 0) & (primary[:, 15:] == 0)].tolist()) == {8}
    assert not D[out != 0].any()


@pytest.mark.parametrize("n", [1, 5, 16])
def test_distance_b_has_the_support_of_distance_n(n):
    primary, image = pc.scene((1, 50, 60), 5, 11)
    out = _both(primary[0], image[0], threshold=0, distance=n)[0]
    assert np.array_equal(out != 0, secondary_ref.secondary_labels(primary, n)[0] != 0)
    assert image.std() > 100  # not a flat image: the stain divides the set, it does not bound it


# ------------------------------------------------------------------------------------------------ the surface without a device
def test_propagate_args():
    from aliby_amd.extraction import features

    assert features.propagate_args() == (0, 0.05, None, 65535, 10737091)
    assert features.propagate_args(400.0, 0, np.int64(7), 4095.0) == (400, 0.0, 7, 4095, 0)
    assert features.propagate_args(65535, 16.0, 64, 65535)[4] == (16 * 65535) ** 2
    assert features.propagate_args(0, 0.05, None, 255)[4] == ref.lambda2(0.05, 255)
    for bad in (-1, 65536, True, 2.5, None, "5", float("nan")):
        with pytest.raises(ValueError, match="threshold must be an integer in 0..65535"):
            features.propagate_args(threshold=bad)
    for bad in (-0.1, float("nan"), float("inf"), True, None, "0.05"):
        with pytest.raises(ValueError, match="regularization must be a finite number >= 0"):
            features.propagate_args(regularization=bad)
    for bad in (0, 65, -3, True, 2.5, "5", float("nan")):
        with pytest.raises(ValueError, match="distance must be None or an integer in 1..64"):
            features.propagate_args(distance=bad)
    for bad in (0, 65536, True, 2.5, None):
        with pytest.raises(ValueError, match="image_max must be an integer in 1..65535"):
            features.propagate_args(image_max=bad)
    with pytest.raises(ValueError, match="at most 2\\^20"):
        features.propagate_args(regularization=16.1)


def test_library_binds_the_entries():
    from aliby_amd import _lib

    for name, arity in (("aliby_propagate_workspace_bytes", 3), ("aliby_propagate_labels", 15)):
        assert name in _lib.exported_symbols()
        assert len(_lib._SIGNATURES[name][1]) == arity
    assert _lib._SIGNATURES["aliby_propagate_labels"][1][7] is ctypes.c_uint64  # lambda2
    assert _lib._SIGNATURES["aliby_propagate_workspace_bytes"][0] is ctypes.c_size_t


EXAMPLE = dict(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1], propagate={"cell": ("nuclei", 0, {"threshold": 400})},
               tertiary={"cytoplasm": ("cell", "nuclei")}, relate=[("nuclei", "cell")])


def test_builder_unchanged_without_the_keyword():
    from aliby_amd.pipe_builder import build_pipeline_steps

    for kw in ({}, dict(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}),
               dict(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1], secondary={"cell": ("nuclei", 10)})):
        plain = build_pipeline_steps(**kw)
        assert build_pipeline_steps(propagate=None, **kw) == plain
        assert repr(build_pipeline_steps(propagate=None, **kw)) == repr(plain)  # order included
        assert not any(k.startswith("propagate") for k in (*plain["steps"], *plain["passed_data"], *plain["save"]))


def test_builder_with_the_keyword():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(**EXAMPLE)
    assert list(p["steps"]) == ["tile", "segment_nuclei", "propagate_cell", "tertiary_cytoplasm",
                                "extract_nuclei", "extract_cell", "extract_cytoplasm",
                                "extractmulti_nuclei", "extractmulti_cell", "extractmulti_cytoplasm",
                                "extractrelate_nuclei", "extractrelate_cell"]
    assert p["steps"]["propagate_cell"] == {"channel": 0, "threshold": 400}
    assert p["steps"]["extract_cell"] is p["steps"]["extract_nuclei"] and p["steps"]["extractmulti_cell"] is p["steps"]["extractmulti_nuclei"]
    pd = p["passed_data"]
    assert pd["propagate_cell"] == [("masks", "segment_nuclei", "primary"), ("pixels", "tile")]
    assert pd["tertiary_cytoplasm"] == [("masks", "propagate_cell", "outer"), ("masks", "segment_nuclei", "inner")]
    assert pd["extract_cell"] == pd["extractmulti_cell"] == [("masks", "propagate_cell"), ("pixels", "tile")]
    assert pd["extractrelate_nuclei"] == [("masks", "segment_nuclei"), ("masks", "propagate_cell", "masks_cell")]
    assert p["save"] == ["segment_nuclei", "propagate_cell", "tertiary_cytoplasm"]
    validate_pipeline(p)
    plain = build_pipeline_steps(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1])
    for key in plain["steps"]:
        assert p["steps"][key] == plain["steps"][key]
    for key in plain["passed_data"]:
        assert pd[key] == plain["passed_data"][key]
    # the two-entry form; after the secondary steps, before the tertiary ones; as an inner set; every option, checked
    q = build_pipeline_steps(secondary={"ring": ("nuclei", 3)}, propagate={"body": ("cell", 1), "b": ("nuclei", 0, {
        "distance": 12.0, "regularization": 0, "image_max": 4095, "threshold": 7})}, tertiary={"rest": ("cell", "body")})
    assert list(q["steps"])[:7] == ["tile", "segment_nuclei", "segment_cell", "secondary_ring", "propagate_body", "propagate_b", "tertiary_rest"]
    assert q["steps"]["propagate_body"] == {"channel": 1}
    assert q["steps"]["propagate_b"] == {"channel": 0, "distance": 12, "regularization": 0.0, "image_max": 4095, "threshold": 7}
    assert q["passed_data"]["tertiary_rest"] == [("masks", "segment_cell", "outer"), ("masks", "propagate_body", "inner")]
    assert q["save"] == ["segment_nuclei", "segment_cell", "secondary_ring", "propagate_body", "propagate_b", "tertiary_rest"]
    validate_pipeline(q)
    assert build_pipeline_steps(propagate={"body": ("cell", 1)}, steps_to_write=["propagate_body"])["save"] == ["propagate_body"]
    # the volume keywords still work beside a propagated set that does not reach them
    v = build_pipeline_steps(propagate={"body": ("cell", 1)}, volume_features=["intensity3d"], relate=[("nuclei", "cell")], volume_relate=True)
    assert "propagate_body" in v["steps"] and "volume_body" not in v["steps"] and "volumerelate_cell" in v["steps"]


@pytest.mark.parametrize("kw", [
    dict(propagate={"cell": ("nuclei", 0)}),                                          # already a segmented object set
    dict(propagate={"ring": ("nuclei", 0)}, secondary={"ring": ("nuclei", 3)}),       # already a secondary object set
    dict(propagate={"ring": ("nuclei", 0)}, tertiary={"ring": ("cell", "nuclei")}),   # clashes with a tertiary name
    dict(propagate={"ring": ("vacuole", 0)}),                                         # the primary is not an object set
    dict(propagate={"ring": ("ring", 0)}),
    dict(propagate={"ring": ("nuclei", 0), "halo": ("ring", 0)}),                     # the primary is not a SEGMENTED object set
    dict(propagate={"halo": ("ring", 0)}, secondary={"ring": ("nuclei", 3)}),
    dict(propagate={"ring": ("nuclei",)}),                                            # malformed entries
    dict(propagate={"ring": "nuclei"}),
    dict(propagate={"ring": ("nuclei", 0, {}, 4)}),
    dict(propagate={"ring": ("nuclei", -1)}),
    dict(propagate={"ring": ("nuclei", True)}),
    dict(propagate={"ring": ("nuclei", 0.0)}),
    dict(propagate={"ring": ("nuclei", 0, 400)}),
    dict(propagate={"ring": ("nuclei", 0, {"method": "propagation"})}),
    dict(propagate={"ring": ("nuclei", 0, {"threshold": -1})}),
    dict(propagate={"ring": ("nuclei", 0, {"distance": 65})}),
    dict(propagate={"ring": ("nuclei", 0, {"regularization": float("nan")})}),
    dict(propagate={"ring": ("nuclei", 0, {"image_max": 0})}),
    dict(propagate={"ri_ng": ("nuclei", 0)}),
    dict(propagate=[("ring", "nuclei", 0)]),
    dict(propagate={"ring": ("nuclei", 0)}, volume_features=["intensity3d"], volume_relate=True, relate=[("ring", "nuclei")]),
    dict(propagate={"ring": ("nuclei", 0)}, volume_features=["intensity3d"], volume_relate=True, tertiary={"rest": ("ring", "nuclei")}),
])
def test_builder_refusals(kw):
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError):
        build_pipeline_steps(**kw)


def test_write_dispatch_knows_propagate():
    from aliby_amd.io.write import dispatch_write_fn, write_ndarray

    assert dispatch_write_fn("propagate_cell") is write_ndarray


def test_init_step_errors():
    from aliby_amd.pipe import init_step

    with pytest.raises(ValueError, match="unknown"):
        init_step("propagate_cell", {"channel": 0, "method": "propagation"})
    with pytest.raises(ValueError, match="channel"):
        init_step("propagate_cell", {"threshold": 5})
    for bad in (-1, True, 0.5, "0", None):
        with pytest.raises(ValueError, match="propagate_cell.*channel"):
            init_step("propagate_cell", {"channel": bad})
    for key, bad, match in (("threshold", 65536, "0..65535"), ("regularization", -1, ">= 0"), ("distance", 0, "1..64"), ("image_max", 0, "1..65535")):
        with pytest.raises(ValueError, match=f"propagate_cell.*{match}"):
            init_step("propagate_cell", {"channel": 0, key: bad})
    # a step whose inputs never arrive says which (before it touches a device)
    step = init_step("propagate_cell", {"channel": 0, "threshold": 400, "distance": 20})
    with pytest.raises(ValueError, match="primary.*pixels"):
        step()
    with pytest.raises(ValueError, match=r"\['pixels'\]"):
        step(primary=np.zeros((4, 4), np.uint16))
    with pytest.raises(ValueError, match=r"\['primary'\]"):
        step(pixels=np.zeros((1, 1, 1, 4, 4), np.uint16))


def test_validate_pipeline_checks_the_alias_and_the_pixels():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(propagate={"body": ("nuclei", 0)})
    validate_pipeline(p)
    p["passed_data"]["propagate_body"] = [("masks", "segment_nuclei"), ("pixels", "tile")]  # alias lost
    with pytest.raises(ValueError, match="primary"):
        validate_pipeline(p)
    p["passed_data"]["propagate_body"] = [("masks", "segment_nuclei", "primary")]  # pixels lost
    with pytest.raises(ValueError, match="pixels"):
        validate_pipeline(p)
    del p["passed_data"]["propagate_body"]
    with pytest.raises(ValueError, match="primary.*pixels"):
        validate_pipeline(p)


def test_run_positions_refuses_a_propagate_step(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(NotImplementedError, match="no batched form of step 'propagate_body'.*position by position"):
        parallel.run_positions([build_pipeline_steps(propagate={"body": ("nuclei", 0)})], ["p0"], tmp_path)
