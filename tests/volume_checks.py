"""
What the GPU tests of the per-object volume families (tests/test_gpu_coloc3d.py, tests/test_gpu_texture3d.py) share: the parity rule
(README "Parity", tests/test_gpu_features.py::_compare: float columns within rtol = 1e-4, atol = 1e-9, NaN where the reference has
NaN), the view that makes bitwise comparisons, the two pixel modes and the silencing of the references' NumPy warnings.
"""
import warnings

import numpy as np
import pytest

from tests import coloc3d_ref

RTOL, ATOL = 1e-4, 1e-9


@pytest.fixture(autouse=True)
def quiet_numpy():
    """Autouse in a module that imports it.  (The oracle's one-voxel variance: numpy warns, the value is the NaN that is wanted.)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def pixel_mode(px, mode):
    """mode "u16": the uint16 pixels as they are; "f32_unit": float32 in [0, 1]."""
    return px if mode == "u16" else coloc3d_ref.unit_float(px)


def check(family, got, want, tag):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape, tag
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    ok = np.isclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    rel = rel[np.isfinite(rel)]
    print(f"{family} {tag}: {want.shape[0]} objects x {want.shape[1]} columns, {int(np.isfinite(want).sum())} finite, "
          f"worst relative error {float(rel.max()) if rel.size else 0.0:.2e}")
    assert ok.all(), (tag, [(int(r), int(c), got[r, c], want[r, c]) for r, c in np.argwhere(~ok)[:6]])
