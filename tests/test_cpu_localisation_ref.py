"""
tests/localisation_ref.py (the float64 restatement of nuc_est_conv the GPU tests compare with) against what the reference's own
function returned on the same seeded inputs (tests/golden/reference_nuc_est_conv.json, written by
tests/golden/make_localisation_golden.py), and the registration of the new family: registry name, C symbol, binding.

Measured largest relative difference, restatement to reference (SciPy 1.15.3, NumPy 2.2.6):

    uint16 pixels (ten scenes, 36 defined rows)   8.64e-16     asserted: 8.64e-15
    float32 pixels (mixed_f32, 8 rows)            4.82e-08     asserted: 4.82e-07

The uint16 figure is the rounding of two float64 summation orders plus the reference's zeroing of filter entries below eps * max.
The float32 figure is NOT the restatement's: the reference hands its float32 image to scipy.signal.convolve, which picks the FFT
method for these sizes and transforms a float32 array in single precision, so the reference's own value carries about 1e-7 of
noise.  test_float32_difference_is_scipys_single_precision_fft shows it: the same 2-D convolution called with the float32 array
lands on the golden value, called with the same numbers held in float64 it lands on the restatement, to 1e-13 both.
"""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import localisation_ref as lr

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "reference_nuc_est_conv.json").read_text())
BOUND_U16 = 10 * 8.64e-16
BOUND_F32 = 10 * 4.82e-08


def _golden(name):
    return np.array([float(v) for v in GOLDEN[name]], np.float64)


def _max_rel(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    keep = ~np.isnan(want) & (got != want)
    return float(np.max(np.abs(got[keep] - want[keep]) / np.abs(want[keep]))) if keep.any() else 0.0


def test_golden_holds_every_scene():
    assert set(GOLDEN) == set(lr.scenes()) | {"border_filter_shape_3x3"}
    for name, s in lr.scenes().items():
        assert len(GOLDEN[name]) == len(lr.rows(s)), name


@pytest.mark.parametrize("name", list(lr.scenes()))
def test_restatement_equals_the_reference(name):
    rel = _max_rel(lr.expected(name), _golden(name))
    print(f"{name}: largest relative difference {rel:.3g}")
    assert rel <= (BOUND_F32 if name == "mixed_f32" else BOUND_U16), (name, rel)


def test_float32_difference_is_scipys_single_precision_fft():
    from scipy import signal

    s = lr.scenes()["mixed_f32"]
    for i, (f, l) in enumerate(lr.rows(s)):
        J, g, denominator = lr.parts(s["labels"][f] == l, s["planes"][f, s["channel"]])
        h = np.outer(g, g)
        assert np.array_equal(J, J.astype(np.float32))  # float32 values held in float64
        assert signal.choose_conv_method(J.astype(np.float32), h, "same") == "fft"
        single = np.max(signal.convolve(J.astype(np.float32), h, "same")) / denominator
        double = np.max(signal.convolve(J, h, "same")) / denominator
        assert abs(single - _golden("mixed_f32")[i]) <= 1e-13 * abs(single), (i, single, _golden("mixed_f32")[i])
        assert abs(double - lr.expected("mixed_f32")[i]) <= 1e-13 * abs(double), (i, double, lr.expected("mixed_f32")[i])


def test_special_values_of_the_reference():
    assert _golden("tiny")[0] == 0.0 and lr.expected("tiny")[0] == 0.0  # one pixel
    d = _golden("degenerate")
    assert np.isnan(d[0]) and np.isnan(d[1]) and d[2] == 0.0 and np.isfinite(d[3])  # all-zero, absent, uniform, a blob
    assert np.array_equal(_golden("border"), _golden("border_filter_shape_3x3"))  # gaussian_filter_shape is overwritten
    s = lr.scenes()["border"]
    assert lr.nuc_est_conv(s["labels"][0] == 1, s["planes"][0, 0], gaussian_filter_shape=(3, 3)) == lr.expected("border")[0]
    # the dim object of the touching pair does not see its neighbour
    assert _golden("neighbours")[0] == _golden("neighbours_zeroed")[0]


def test_family_is_registered():
    from aliby_amd.extraction import families
    from aliby_amd.extraction.engine import FeatureEngine
    from aliby_amd.extraction import functions

    reg = families.MONO["nuc_est_conv"]
    assert reg.names({}) is None and reg.needs_pixels and reg.after_join
    assert callable(FeatureEngine.nuc_est_conv) and callable(functions.nuc_est_conv)


def test_library_exports_nuc_est_conv():
    lib_path = ROOT / "aliby_amd" / "libaliby_hip.so"
    if not lib_path.exists():
        import __graft_entry__ as g

        g.build()
    header = (ROOT / "include" / "aliby_hip.h").read_text()
    assert re.search(r"\baliby_features_nuc_est_conv\s*\(", header)
    from aliby_amd import _lib

    assert "aliby_features_nuc_est_conv" in _lib.exported_symbols()
    restype, argtypes = _lib._SIGNATURES["aliby_features_nuc_est_conv"]
    assert restype is ctypes.c_int and len(argtypes) == 22 and argtypes.count(ctypes.c_double) == 3
    assert getattr(ctypes.CDLL(str(lib_path)), "aliby_features_nuc_est_conv") is not None
