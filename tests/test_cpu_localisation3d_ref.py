"""
tests/localisation3d_ref.py (the float64 restatement of nuc_conv_3d the GPU tests compare with) against what the reference's own
function returned on the same seeded inputs (tests/golden/reference_nuc_conv_3d.json, written by
tests/golden/make_localisation3d_golden.py), and the registration of the new metric: registry entry, C symbol, binding.

Measured largest relative difference, restatement to reference (SciPy 1.15.3, NumPy 2.2.6):

    uint16 voxels (thirteen scenes, 41 defined rows)   2.29e-15     asserted: 2.29e-14
    float32 voxels (three scenes, 11 rows)             3.72e-08     asserted: 3.72e-07

The uint16 figure is the rounding of different float64 summation orders (the reference transforms, the restatement sums directly)
plus the reference's zeroing of filter entries below eps * max.  The float32 figure is not the restatement's, as in 2-D
(tests/test_cpu_localisation_ref.py): the reference hands its float32 stack to scipy.signal.convolve, which transforms a float32
array in single precision.  test_float32_difference_is_scipys_single_precision shows it on the first row.
"""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import localisation3d_ref as lr

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "reference_nuc_conv_3d.json").read_text())
BOUND_U16 = 10 * 2.29e-15
BOUND_F32 = 10 * 3.72e-08


def _golden(name):
    return np.array([float(v) for v in GOLDEN[name]], np.float64)


def _max_rel(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    keep = ~np.isnan(want) & (got != want)
    return float(np.max(np.abs(got[keep] - want[keep]) / np.abs(want[keep]))) if keep.any() else 0.0


def test_golden_holds_every_scene():
    assert set(GOLDEN) == set(lr.scenes())
    for name, s in lr.scenes().items():
        assert len(GOLDEN[name]) == len(lr.rows(s)), name


@pytest.mark.parametrize("name", list(lr.scenes()))
def test_restatement_equals_the_reference(name):
    rel = _max_rel(lr.expected(name), _golden(name))
    print(f"{name}: largest relative difference {rel:.3g}")
    assert rel <= (BOUND_F32 if name.endswith("_f32") else BOUND_U16), (name, rel)


def test_float32_difference_is_scipys_single_precision():
    """The reference's 3-D convolution of the float32 J lands on the golden value; of the same numbers held in float64, on the
    restatement (to the uint16 bound: the method differs, the precision does not)."""
    from scipy import signal

    s = lr.scenes()["mixed_f32"]
    f, l = lr.rows(s)[0]
    J, gx, gz, denominator, _ = lr.parts(s["labels"][f] == l, s["stack"][f, s["channel"]])
    h = gz[:, None, None] * gx[None, :, None] * gx[None, None, :]
    assert np.array_equal(J, J.astype(np.float32))  # float32 values held in float64
    single = np.max(signal.convolve(J.astype(np.float32), h, "same")) / denominator
    double = np.max(signal.convolve(J, h, "same")) / denominator
    assert abs(single - _golden("mixed_f32")[0]) <= 1e-6 * abs(single) and single != double
    assert abs(double - lr.expected("mixed_f32")[0]) <= BOUND_U16 * abs(double), (double, lr.expected("mixed_f32")[0])
    assert abs(single - double) > 10 * abs(double - lr.expected("mixed_f32")[0])


def test_special_values_of_the_reference():
    assert _golden("tiny_z1")[0] == 0.0 and lr.expected("tiny_z1")[0] == 0.0  # one voxel
    assert _golden("tiny_z9")[0] > 0.0  # one pixel on nine planes is nine voxels
    d = _golden("degenerate")
    assert np.isnan(d[0]) and np.isnan(d[1]) and d[2] == 0.0 and np.isfinite(d[3])  # all-zero, absent, uniform, a blob
    # the dim object of the touching pair does not see its neighbour
    assert _golden("neighbours")[0] == _golden("neighbours_zeroed")[0] == _golden("neighbours_alone")[0]
    # the two keyword pairs change the value, each in its own way
    assert len({_golden(n)[0] for n in ("mixed_u16", "kw_flat", "kw_cubic")}) == 3


def test_scenes_are_what_the_gpu_tests_take_them_for():
    s = lr.scenes()
    z = s["zeros_inside"]
    area, n = int(z["labels"][0].sum()), int(np.count_nonzero(z["stack"][0, 0][:, z["labels"][0] > 0]))
    assert n < 5 * area and n % area != 0
    for name, hw_want, planes in (("tiny_z9", (1, 2), 9), ("disc40", (53,), 5)):
        sc = s[name]
        assert sc["stack"].shape[2] == planes
        hws = {lr.parts(sc["labels"][f] == l, sc["stack"][f, 0])[4] for f, l in lr.rows(sc)}
        assert hws <= set(hw_want), (name, hws)
    # the object of `fill`: its box dilated by hw is the whole tile
    f = s["fill"]
    hw = lr.parts(f["labels"][0] == 1, f["stack"][0, 0])[4]
    ys, xs = np.nonzero(f["labels"][0])
    assert ys.min() - hw <= 0 and xs.min() - hw <= 0 and ys.max() + hw >= 11 and xs.max() + hw >= 11


def test_metric_is_registered():
    from aliby_amd.extraction import families
    from aliby_amd.extraction.engine import FeatureEngine
    from aliby_amd.extraction import functions

    reg = families.MONO["nuc_conv_3d"]
    assert reg.names({}) is None and reg.needs_pixels and reg.after_join and reg.stack
    assert [m for m, r in families.MONO.items() if r.stack] == ["nuc_conv_3d"]
    assert callable(FeatureEngine.nuc_conv_3d) and callable(functions.nuc_conv_3d)


def test_library_exports_nuc_conv_3d():
    lib_path = ROOT / "aliby_amd" / "libaliby_hip.so"
    if not lib_path.exists():
        import __graft_entry__ as g

        g.build()
    header = (ROOT / "include" / "aliby_hip.h").read_text()
    assert re.search(r"\baliby_features_nuc_conv_3d\s*\(", header)
    from aliby_amd import _lib

    assert "aliby_features_nuc_conv_3d" in _lib.exported_symbols()
    restype, argtypes = _lib._SIGNATURES["aliby_features_nuc_conv_3d"]
    assert restype is ctypes.c_int and len(argtypes) == 21 and argtypes.count(ctypes.c_double) == 2
    assert getattr(ctypes.CDLL(str(lib_path)), "aliby_features_nuc_conv_3d") is not None
