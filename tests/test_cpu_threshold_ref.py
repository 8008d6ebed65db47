"""
The automatic threshold without a device: the two statements of the definition in tests/threshold_ref.py (a Python loop, NumPy)
against each other bit for bit and against the worked examples of include/aliby_hip.h; the correction and the bounds; the argument
checks of features.auto_threshold_args; the bindings; the builder and the step.
"""

import ctypes

import numpy as np
import pytest

from tests import threshold_ref as ref


def _hist(pixels) -> np.ndarray:
    return ref.histogram(np.asarray(pixels, np.uint16))


def _both(h, **options) -> ref.Otsu:
    loop, vec = ref.otsu_loop(h, **options), ref.otsu_numpy(h, **options)
    assert loop == vec, (loop, vec, options)
    return loop


# ------------------------------------------------------------------------------------------------ the worked examples, as hand values
def test_two_levels():
    got = _both(_hist([100] * 10 + [200] * 10))
    assert got == ref.Otsu(101, 100, 200, 101, 101)


def test_three_spikes_tie():
    h = _hist([100] * 10 + [200] * 10 + [300] * 10)
    # the splits after 100 and after 200 tie: 1000^2/10 + 5000^2/20 == 3000^2/20 + 3000^2/10 == 1 350 000
    assert 1000.0 * 1000.0 / 10.0 + 5000.0 * 5000.0 / 20.0 == 3000.0 * 3000.0 / 20.0 + 3000.0 * 3000.0 / 10.0 == 1350000.0
    assert _both(h) == ref.Otsu(101, 100, 300, 101, 101)
    assert _both(h, classes=3) == ref.Otsu(101, 100, 300, 101, 201)
    assert _both(h, classes=3, middle="background") == ref.Otsu(201, 100, 300, 101, 201)


def test_ten_twenty_thirty():
    h = _hist([10, 20, 30])
    assert _both(h) == ref.Otsu(11, 10, 30, 11, 11)
    assert _both(h, classes=3) == ref.Otsu(11, 10, 30, 11, 21)


def test_the_ends_of_the_range():
    h = _hist([0, 65535])
    assert _both(h) == ref.Otsu(1, 0, 65535, 1, 1)
    assert _both(h, classes=3) == ref.Otsu(1, 0, 65535, 1, 1)  # two occupied bins: falls back
    assert _both(h, classes=3, middle="background") == ref.Otsu(1, 0, 65535, 1, 1)


def test_the_middle_of_the_range():
    assert _both(_hist([32767, 32768, 32768])) == ref.Otsu(32768, 32767, 32768, 32768, 32768)


@pytest.mark.parametrize("level", [0, 1, 32767, 32768, 65535])
def test_constant_tile(level):
    for options in ({}, {"classes": 3}, {"classes": 3, "middle": "background"}):
        assert _both(_hist([level] * 7), **options) == ref.Otsu(level, level, level, level, level)
    assert _both(_hist([level]), correction=0.5, bounds=(3, 40000)).threshold == min(max(int(np.rint(level * 0.5)), 3), 40000)


# ------------------------------------------------------------------------------------------------ correction and bounds
def test_correction_rounds_half_to_even():
    h = _hist([100] * 10 + [200] * 10)
    assert _both(h, correction=0.5).threshold == 50      # 50.5
    assert ref.finish(103, 0.5) == 52 and ref.finish(105, 0.5) == 52  # 51.5, 52.5
    assert _both(h, correction=1.5).threshold == 152     # 151.5
    assert _both(h, correction=0.7).threshold == 71      # 70.7
    assert _both(h, correction=0.5).details == (100, 200, 101, 101)  # the details stay raw


def test_bounds_clamp_on_both_sides():
    h = _hist([100] * 10 + [200] * 10)
    assert _both(h, bounds=(150, 65535)).threshold == 150
    assert _both(h, bounds=(0, 60)).threshold == 60
    assert _both(h, bounds=(101, 101)).threshold == 101
    assert _both(h, correction=1.5, bounds=(0, 151)).threshold == 151
    assert ref.finish(65535, 16.0) == 65535 and ref.finish(40000, 2.0, (0, 65535)) == 65535  # the product saturates first
    assert ref.finish(1, 0.25) == 0


# ------------------------------------------------------------------------------------------------ random histograms
def _random_hist(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    kind = seed % 6
    h = np.zeros(ref.LEVELS, np.int64)
    if kind == 0:    # sparse over the whole range
        h[rng.integers(0, ref.LEVELS, 40)] = rng.integers(1, 50, 40)
    elif kind == 1:  # dense, narrower than 256 levels
        lo = int(rng.integers(0, ref.LEVELS - 256))
        width = int(rng.integers(2, 256))
        h[lo:lo + width] = rng.integers(0, 1000, width)
    elif kind == 2:  # dense, straddling 32767 / 32768
        lo, hi = 32768 - int(rng.integers(1, 600)), 32768 + int(rng.integers(1, 600))
        h[lo:hi] = rng.integers(0, 30, hi - lo)
    elif kind == 3:  # three modes, large counts (sums near 2^40)
        for centre in rng.integers(1000, 64000, 3):
            v = np.clip(rng.normal(centre, 300, 3000).astype(np.int64), 0, ref.LEVELS - 1)
            np.add.at(h, v, int(rng.integers(1, 2000)))
    elif kind == 4:  # few levels, many ties
        lo = int(rng.integers(0, 60000))
        h[lo + rng.integers(0, 5000, 6)] = int(rng.integers(1, 9))
    else:            # narrow and sparse, straddling the middle
        h[32760 + rng.integers(0, 16, 5)] = rng.integers(1, 4, 5)
    if not h.any():
        h[int(rng.integers(0, ref.LEVELS))] = 1
    return h


@pytest.mark.parametrize("seed", range(24))
def test_loop_and_numpy_agree_on_random_histograms(seed):
    h = _random_hist(seed)
    two = _both(h)
    assert two.lo < two.t1 <= two.hi or two.lo == two.hi == two.t1
    for options in ({"classes": 3}, {"classes": 3, "middle": "background", "correction": 0.7, "bounds": (5, 60000)}):
        three = _both(h, **options)
        assert three.lo <= three.t1 <= three.t2 <= three.hi + 1
    assert _both(h, classes=3).t1 == _both(h, classes=3, middle="background").t1


def test_the_kinds_cover_what_they_say():
    narrow, straddle = _random_hist(1), _random_hist(2)
    assert np.flatnonzero(narrow)[-1] - np.flatnonzero(narrow)[0] < 256
    assert straddle[:32768].any() and straddle[32768:].any()
    assert np.count_nonzero(_random_hist(0)) <= 40 and np.count_nonzero(_random_hist(3)) > 1000


# ------------------------------------------------------------------------------------------------ the argument checks
def test_auto_threshold_args_good_values():
    from aliby_amd.extraction.features import AUTO_THRESHOLD_OPTIONS, auto_threshold_args

    assert tuple(auto_threshold_args()) == ("otsu", 2, None, 1.0, (0, 65535))  # two classes have no middle class
    assert auto_threshold_args().middle_code == 0 and auto_threshold_args(classes=3).middle_code == 0
    assert auto_threshold_args(classes=3, middle="background").middle_code == 1
    assert auto_threshold_args()._fields == AUTO_THRESHOLD_OPTIONS
    got = auto_threshold_args("otsu", 3, "background", 0.7, [10.0, 4095])
    assert tuple(got) == ("otsu", 3, "background", 0.7, (10, 4095)) and isinstance(got.bounds[0], int)
    assert auto_threshold_args(classes=np.int64(3)).middle == "foreground"
    assert auto_threshold_args(correction=16).correction == 16.0 and auto_threshold_args(correction=1e-3).correction == 1e-3
    assert auto_threshold_args(bounds=(7, 7)).bounds == (7, 7)
    assert got.options() == {"method": "otsu", "classes": 3, "middle": "background", "correction": 0.7, "bounds": [10, 4095]}
    assert got.options({"classes": 0, "bounds": 0}) == {"classes": 3, "bounds": [10, 4095]}


@pytest.mark.parametrize("kw, match", [
    (dict(method="mce"), "not built"),
    (dict(method="minimum_cross_entropy"), "not built"),
    (dict(method="li"), "not built"),
    (dict(method="triangle"), "must be 'otsu'"),
    (dict(method=2), "must be 'otsu'"),
    (dict(classes=4), "2 or 3"),
    (dict(classes=True), "2 or 3"),
    (dict(classes=2.0), "2 or 3"),
    (dict(classes="3"), "2 or 3"),
    (dict(classes=2, middle="foreground"), "three classes only"),
    (dict(middle="background"), "three classes only"),
    (dict(classes=3, middle="middle"), "'foreground' or 'background'"),
    (dict(classes=3, middle=1), "'foreground' or 'background'"),
    (dict(correction=0), r"\(0, 16\]"),
    (dict(correction=-1.0), r"\(0, 16\]"),
    (dict(correction=16.5), r"\(0, 16\]"),
    (dict(correction=float("nan")), r"\(0, 16\]"),
    (dict(correction=float("inf")), r"\(0, 16\]"),
    (dict(correction=True), r"\(0, 16\]"),
    (dict(correction="0.7"), r"\(0, 16\]"),
    (dict(bounds=(5, 4)), "0 <= lo <= hi <= 65535"),
    (dict(bounds=(-1, 4)), "0 <= lo <= hi <= 65535"),
    (dict(bounds=(0, 65536)), "0 <= lo <= hi <= 65535"),
    (dict(bounds=(0.5, 10)), "0 <= lo <= hi <= 65535"),
    (dict(bounds=(0, True)), "0 <= lo <= hi <= 65535"),
    (dict(bounds=("0", "10")), "0 <= lo <= hi <= 65535"),
    (dict(bounds=(0, 10, 20)), "0 <= lo <= hi <= 65535"),
    (dict(bounds=10), "0 <= lo <= hi <= 65535"),
])
def test_auto_threshold_args_bad_values(kw, match):
    from aliby_amd.extraction.features import auto_threshold_args

    with pytest.raises(ValueError, match=match):
        auto_threshold_args(**kw)


@pytest.mark.parametrize("given", [{}, {"correction": 0.7}, {"classes": 2, "bounds": (3, 4095)}, {"classes": 3},
                                   {"classes": 3, "middle": "background", "correction": 1.5}, {"method": "otsu"}])
def test_checked_options_pass_the_checks_again(given):
    """What a step stores and hands down on every call is a checked dict: it must be accepted as it is, two classes included."""
    from aliby_amd.extraction.features import auto_threshold_args, auto_threshold_options

    first = auto_threshold_options(given)
    assert auto_threshold_options(first.options()) == first
    assert auto_threshold_options(first.options(given)) == first and set(first.options(given)) == set(given)
    assert auto_threshold_args(*first) == first and auto_threshold_args(**first._asdict()) == first
    assert ("middle" in first.options()) == (first.classes == 3)


def test_auto_threshold_options_names_the_keys():
    from aliby_amd.extraction.features import auto_threshold_options

    assert auto_threshold_options({}) == auto_threshold_options({"method": "otsu", "classes": 2})
    for bad in ({"klasses": 3}, {"threshold": 5}, "otsu", None, [("classes", 3)]):
        with pytest.raises(ValueError, match="'method', 'classes', 'middle', 'correction', 'bounds'"):
            auto_threshold_options(bad)


def test_propagate_args_is_what_it_was():
    from aliby_amd.extraction.features import PROPAGATE_OPTIONS, propagate_args

    assert PROPAGATE_OPTIONS == ("threshold", "regularization", "distance", "image_max")
    assert propagate_args()._fields == (*PROPAGATE_OPTIONS, "lambda2")


def test_symbols_are_bound():
    from aliby_amd import _lib

    for name, arity in (("aliby_auto_threshold_workspace_bytes", 1), ("aliby_auto_threshold", 15), ("aliby_propagate_labels_per_tile", 15)):
        assert name in _lib.exported_symbols()
        assert len(_lib._SIGNATURES[name][1]) == arity
    assert _lib._SIGNATURES["aliby_auto_threshold_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib._SIGNATURES["aliby_auto_threshold"][1][7] is ctypes.c_double  # correction
    per_tile, scalar = _lib._SIGNATURES["aliby_propagate_labels_per_tile"][1], _lib._SIGNATURES["aliby_propagate_labels"][1]
    assert per_tile[6] is ctypes.c_void_p and scalar[6] is ctypes.c_int and per_tile[:6] == scalar[:6] and per_tile[7:] == scalar[7:]
    assert len(scalar) == 15  # the old entry keeps its signature


# ------------------------------------------------------------------------------------------------ builder and step
AUTO = {"classes": 3, "middle": "foreground", "correction": 0.7}


def test_builder_writes_the_checked_dict():
    from aliby_amd.pipe_builder import build_pipeline_steps
    from aliby_amd.pipe_core import validate_pipeline

    p = build_pipeline_steps(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1], propagate={"cell": ("nuclei", 0, {"auto_threshold": AUTO})},
                             tertiary={"cytoplasm": ("cell", "nuclei")})
    assert p["steps"]["propagate_cell"] == {"channel": 0, "auto_threshold": {"classes": 3, "middle": "foreground", "correction": 0.7}}
    assert p["steps"]["propagate_cell"]["auto_threshold"] is not AUTO
    assert p["passed_data"]["propagate_cell"] == [("masks", "segment_nuclei", "primary"), ("pixels", "tile")]
    validate_pipeline(p)
    q = build_pipeline_steps(propagate={"body": ("nuclei", 0, {"distance": 12.0, "auto_threshold": {"bounds": (10.0, 4095), "classes": np.int64(2)}})})
    assert q["steps"]["propagate_body"] == {"channel": 0, "distance": 12, "auto_threshold": {"classes": 2, "bounds": [10, 4095]}}
    assert type(q["steps"]["propagate_body"]["auto_threshold"]["classes"]) is int
    validate_pipeline(q)
    assert build_pipeline_steps(propagate={"body": ("nuclei", 0, {"auto_threshold": {}})})["steps"]["propagate_body"] == {"channel": 0, "auto_threshold": {}}
    # an explicit threshold of 0 beside it is no conflict
    r = build_pipeline_steps(propagate={"body": ("nuclei", 0, {"threshold": 0, "auto_threshold": {}})})
    assert r["steps"]["propagate_body"] == {"channel": 0, "threshold": 0, "auto_threshold": {}}


def test_builder_unchanged_without_the_option():
    from aliby_amd.pipe_builder import build_pipeline_steps

    kw = dict(channels_to_segment={"nuclei": 1}, channels_to_extract=[0, 1], propagate={"cell": ("nuclei", 0, {"threshold": 400, "distance": 9})},
              tertiary={"cytoplasm": ("cell", "nuclei")}, relate=[("nuclei", "cell")])
    p = build_pipeline_steps(**kw)
    assert p["steps"]["propagate_cell"] == {"channel": 0, "threshold": 400, "distance": 9}
    assert list(p["steps"]["propagate_cell"]) == ["channel", "threshold", "distance"]
    assert not any("auto_threshold" in repr(step) for step in p["steps"].values())
    assert build_pipeline_steps(propagate={"body": ("cell", 1)})["steps"]["propagate_body"] == {"channel": 1}


@pytest.mark.parametrize("options", [
    {"threshold": 400, "auto_threshold": {}},                       # both
    {"auto_threshold": {"classes": 2, "middle": "foreground"}},     # middle with two classes
    {"auto_threshold": {"method": "mce"}},
    {"auto_threshold": {"klasses": 3}},                             # unknown nested key
    {"auto_threshold": {"classes": 3, "threshold": 5}},
    {"auto_threshold": "otsu"},
    {"auto_threshold": None},
    {"auto_threshold": {"correction": 0}},
    {"auto_threshold": {"bounds": (5, 4)}},
    {"method": "otsu"},                                             # only the nested dict knows `method`
    {"classes": 3},
])
def test_builder_refusals(options):
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError, match=r"propagate\['ring'\]"):
        build_pipeline_steps(propagate={"ring": ("nuclei", 0, options)})


def test_builder_says_which_options_conflict():
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(ValueError, match="threshold or auto_threshold, not both"):
        build_pipeline_steps(propagate={"ring": ("nuclei", 0, {"threshold": 400, "auto_threshold": {}})})


def test_init_step_errors_name_the_step():
    from aliby_amd.pipe import init_step

    for parameters, match in (
        ({"auto_threshold": {"method": "mce"}}, "not built"),
        ({"auto_threshold": {"classes": 2, "middle": "background"}}, "three classes only"),
        ({"auto_threshold": {"klasses": 3}}, "keys of"),
        ({"auto_threshold": 3}, "keys of"),
        ({"auto_threshold": {"correction": 17}}, r"\(0, 16\]"),
        ({"auto_threshold": {"bounds": [9, 3]}}, "0 <= lo <= hi"),
        ({"auto_threshold": {}, "threshold": 5}, "not both"),
        ({"method": "otsu"}, "unknown"),
        ({"classes": 3}, "unknown"),
    ):
        with pytest.raises(ValueError, match=f"propagate_cell.*{match}"):
            init_step("propagate_cell", {"channel": 0, **parameters})
    step = init_step("propagate_cell", {"channel": 0, "auto_threshold": {"classes": 3, "bounds": [0, 4095]}, "distance": 20})
    assert step.thresholds == []
    with pytest.raises(ValueError, match="primary.*pixels"):  # says which inputs are missing before it touches a device
        step()
    # two classes, the default: the stored options pass the checks of every call (the step re-checks what it hands down)
    for auto in ({}, {"correction": 0.7}, {"classes": 2}):
        step = init_step("propagate_cell", {"channel": 0, "auto_threshold": auto})
        with pytest.raises(ValueError, match="propagate_cell.*no tiles"):  # past the option checks, before it touches a device
            step(primary=[], pixels=np.zeros((1, 1, 1, 4, 4), np.uint16))
    # the scalar step keeps the attribute too
    assert init_step("propagate_cell", {"channel": 0, "threshold": 400}).thresholds == []


def test_host_forms_refuse_both_before_a_device_is_touched():
    from aliby_amd.extraction import extract, functions

    labels, stain = np.zeros((4, 4), np.uint16), np.zeros((4, 4), np.uint16)
    with pytest.raises(ValueError, match="not both"):
        extract.propagate_masks(labels, stain[None, None, None], 0, threshold=5, auto_threshold={})
    with pytest.raises(ValueError, match="keys of"):
        extract.propagate_masks(labels, stain[None, None, None], 0, auto_threshold={"klasses": 2})
    with pytest.raises(ValueError, match="not both"):
        functions.propagate_objects(labels, stain, threshold=5, auto_threshold={})
    with pytest.raises(ValueError, match="not built"):
        functions.propagate_objects(labels, stain, auto_threshold={"method": "li"})
    with pytest.raises(ValueError, match="threshold must be an integer in 0..65535"):  # a bad threshold is reported as that
        functions.propagate_objects(labels, stain, threshold="5", auto_threshold={})
    with pytest.raises(ValueError, match="uint16"):
        functions.auto_threshold(stain.astype(np.float32))


def test_run_positions_still_refuses_the_step(tmp_path):
    from aliby_amd import parallel
    from aliby_amd.pipe_builder import build_pipeline_steps

    with pytest.raises(NotImplementedError, match="no batched form of step 'propagate_body'"):
        parallel.run_positions([build_pipeline_steps(propagate={"body": ("nuclei", 0, {"auto_threshold": AUTO})})], ["p0"], tmp_path)
