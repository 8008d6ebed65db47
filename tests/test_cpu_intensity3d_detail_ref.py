"""
Pins tests/intensity3d_detail_ref.py (the reference the GPU family `intensity3d_detail` is compared with) without a GPU: to the
oracle's get_intensity on one-plane stacks for every shared column, to the oracle's find_boundaries_inner on 3-D label arrays, and to
hand values for the branches of the quartile rule, the edge test and the tie rule.  It also checks the column names, and that the new
C entries are declared, bound and exported.  cp_measure / CellProfiler are not vendored: parity on volumes stays unpinned.
"""
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

from oracle import cp_measure_restated as cpm
from tests import intensity3d_detail_ref as ref

ROOT = Path(__file__).resolve().parents[1]
C13 = ref.cols(True)


@pytest.fixture(autouse=True)
def _quiet_numpy():
    with warnings.catch_warnings():  # (the oracle divides by the area of absent labels: numpy warns, the NaN is wanted)
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def _one(values, edge=True):
    """The row of one object whose voxels, in raster order, hold `values`: a line along x inside a larger stack."""
    values = np.asarray(values)
    n = len(values)
    vol = np.zeros((3, 3, n + 2), np.uint16)
    vol[1, 1, 1:1 + n] = 1
    px = np.zeros(vol.shape, values.dtype)
    px[1, 1, 1:1 + n] = values
    return ref.detail(vol, px, 1, edge)[0]


# ------------------------------------------------------------------------------------------------ names and the C ABI
def test_names_in_both_flag_states():
    from aliby_amd.extraction import features

    with_edge = features.intensity3d_detail_names()
    assert with_edge == features.intensity3d_detail_names(True) == ref.names(True) and len(with_edge) == 13
    assert with_edge[:5] == features.INTENSITY_EDGE and with_edge[5] == "Intensity_MassDisplacement"
    assert with_edge[6:10] == ["Intensity_LowerQuartileIntensity", "Intensity_MedianIntensity", "Intensity_MADIntensity", "Intensity_UpperQuartileIntensity"]
    assert with_edge[10:] == ["Location_MaxIntensity_X", "Location_MaxIntensity_Y", "Location_MaxIntensity_Z"]
    without = features.intensity3d_detail_names(False)
    assert without == with_edge[5:] == ref.names(False) and len(without) == 8
    for flag in (True, False):  # intensity3d and the detail block together: the 2-D family's columns, plus Volume and Location_Center_*
        both = features.intensity3d_names() + features.intensity3d_detail_names(flag)
        assert len(set(both)) == len(both)
        assert set(both) == set(features.intensity_names(flag)) | {"Volume", "Location_Center_X", "Location_Center_Y", "Location_Center_Z"}
        kept = [k for k in features.intensity_names(flag) if k in features.intensity3d_detail_names(flag)]
        assert kept == features.intensity3d_detail_names(flag)  # in the 2-D family's order
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(TypeError):
            features.intensity3d_detail_names(bad)


def test_the_c_entries_are_declared_bound_and_exported():
    header = (ROOT / "include" / "aliby_hip.h").read_text()
    assert re.search(r"\bint aliby_intensity3d_detail_lds_voxels\s*\(\s*void\s*\)", header)
    m = re.search(r"\bint aliby_features_intensity3d_detail\s*\(([^)]*)\)", header)
    assert m
    from aliby_amd import _lib

    assert {"aliby_features_intensity3d_detail", "aliby_intensity3d_detail_lds_voxels"} <= set(_lib.exported_symbols())
    assert len(_lib._SIGNATURES["aliby_features_intensity3d_detail"][1]) == len(m.group(1).split(",")) == 16
    assert _lib._SIGNATURES["aliby_intensity3d_detail_lds_voxels"] == (_lib._i, [])
    import ctypes

    lib_path = ROOT / "aliby_amd" / "libaliby_hip.so"
    if not lib_path.exists():
        import __graft_entry__ as g

        g.build()
    handle = ctypes.CDLL(str(lib_path))
    handle.aliby_intensity3d_detail_lds_voxels.restype = ctypes.c_int
    budget = handle.aliby_intensity3d_detail_lds_voxels()
    assert budget >= 1024 and budget & (budget - 1) == 0  # a power of two: the sort pads to one
    assert handle.aliby_features_intensity3d_detail is not None


# ------------------------------------------------------------------------------------------------ hand values
def test_the_quartile_rule_branch_by_branch():
    q = lambda row: [row[C13[k]] for k in ("Intensity_LowerQuartileIntensity", "Intensity_MedianIntensity", "Intensity_UpperQuartileIntensity")]  # noqa: E731
    u = lambda *v: np.asarray(v, np.uint16)  # noqa: E731
    assert q(_one(u(7))) == [7.0, 7.0, 7.0]                               # n = 1: i = 0 = n - 1 throughout
    assert q(_one(u(30, 10))) == [20.0, 30.0, 30.0]                       # n = 2: 1/4 -> i 0, f 1/2; 1/2 -> v[1]; 3/4 -> i 1 = n - 1: v[1]
    assert q(_one(u(30, 10, 20))) == [17.5, 25.0, 30.0]                   # n = 3: q = 3/4, 3/2, 9/4: the last has no upper neighbour
    assert q(_one(u(40, 10, 30, 20))) == [20.0, 30.0, 40.0]               # n = 4: f = 0 throughout
    assert q(_one(u(50, 10, 40, 20, 30))) == [22.5, 35.0, 47.5]           # n = 5: q = 5/4, 5/2, 15/4
    mad = C13["Intensity_MADIntensity"]
    assert _one(u(7))[mad] == 0.0
    assert _one(u(30, 10))[mad] == 20.0                                   # |v - 30| = 0, 20 -> v[1]
    assert _one(u(30, 10, 20))[mad] == 10.0                               # |v - 25| = 5, 5, 15 -> q = 3/2: (5 + 15) / 2
    assert _one(u(50, 10, 40, 20, 30))[mad] == 15.0                       # |v - 35| = 5, 5, 15, 15, 25 -> q = 5/2: (15 + 15) / 2
    f = np.asarray([0.1, 0.7, 0.2], np.float32)                           # float32 pixels: float64 arithmetic on the exact values
    s = np.sort(f.astype(np.float64))
    assert q(_one(f)) == [s[0] * 0.25 + s[1] * 0.75, s[1] * 0.5 + s[2] * 0.5, s[2]]
    med = s[1] * 0.5 + s[2] * 0.5
    d = np.sort(np.abs(f.astype(np.float64) - med))
    assert _one(f)[mad] == d[1] * 0.5 + d[2] * 0.5 and np.float64(np.float32(_one(f)[mad])) != _one(f)[mad]  # (it does not fit a float32)


def test_a_cube_has_26_edge_voxels_and_a_centre_that_is_none():
    vol = np.zeros((5, 5, 5), np.uint16)
    vol[1:4, 1:4, 1:4] = 1
    e = ref.edge_mask(vol)
    assert int(e.sum()) == 26 and not e[2, 2, 2]
    px = np.full(vol.shape, 5, np.uint16)
    px[2, 2, 2] = 60000  # the centre: not an edge voxel
    row = ref.detail(vol, px, 1)[0]
    assert list(row[:5]) == [130.0, 5.0, 0.0, 5.0, 5.0]
    # a face of the stack is no edge: a block that fills its stack has none
    full = np.ones((3, 3, 3), np.uint16)
    assert not ref.edge_mask(full).any()


def test_a_stack_filled_by_one_label_has_five_zeros():
    vol = np.ones((2, 3, 4), np.uint16)
    px = np.arange(24, dtype=np.uint16).reshape(vol.shape) + 1
    row = ref.detail(vol, px, 1)[0]
    assert list(row[:5]) == [0.0] * 5 and np.isfinite(row[5:]).all()
    assert ref.detail(vol, px, 1, edge=False).shape == (1, 8) and np.array_equal(ref.detail(vol, px, 1, edge=False)[0], row[5:])


def test_a_maximum_repeated_on_two_planes_takes_the_last():
    vol = np.zeros((4, 5, 6), np.uint16)
    vol[0:3, 1:4, 1:5] = 1
    px = np.full(vol.shape, 9, np.uint16)
    px[0, 2, 3] = px[2, 1, 2] = px[1, 3, 4] = 500  # raster order: plane 0, plane 1, plane 2: the last is (z 2, y 1, x 2)
    row = ref.detail(vol, px, 1)[0]
    assert [row[C13[f"Location_MaxIntensity_{a}"]] for a in "XYZ"] == [2.0, 1.0, 2.0]
    px[:] = 9  # all equal: the very last voxel of the object
    row = ref.detail(vol, px, 1)[0]
    assert [row[C13[f"Location_MaxIntensity_{a}"]] for a in "XYZ"] == [4.0, 3.0, 2.0]


def test_mass_displacement_of_a_two_voxel_object_and_of_a_dark_one():
    md = C13["Intensity_MassDisplacement"]
    assert _one(np.asarray([1, 3], np.uint16))[md] == 0.25  # centre 1.5, centre of mass (1 + 2 * 3) / 4 = 1.75
    assert np.isnan(_one(np.asarray([0, 0, 0], np.uint16))[md])
    vol = np.zeros((3, 3, 3), np.uint16)
    vol[0, 0, 0] = vol[2, 2, 2] = 1
    px = np.zeros(vol.shape, np.uint16)
    px[2, 2, 2] = 77  # all the mass in one corner: the displacement is half the diagonal
    assert np.isclose(ref.detail(vol, px, 1)[0][md], np.sqrt(3.0), rtol=1e-15, atol=0)


def test_absent_labels_labels_above_the_count_and_the_flag():
    vol, n, px = ref.faces_volume()
    got = ref.detail(vol, px, n)
    assert got.shape == (8, 13) and np.isnan(got[7]).all() and np.isfinite(got[:7]).all()  # label 8 has no voxels; 9 is not measured
    assert np.array_equal(ref.detail(vol, px, n, edge=False), got[:, 5:], equal_nan=True)
    assert ref.detail(np.zeros((2, 2, 2), np.uint16), np.zeros((2, 2, 2), np.uint16), 0).shape == (0, 13)
    # the voxel of label 9 makes (3, 3, 4) of label 7 an edge voxel — it is one anyway; erase the background next to another to see 9 count
    solid = np.zeros((5, 5, 5), np.uint16)
    solid[:] = 1
    solid[2, 2, 2] = 9
    assert int(ref.edge_mask(solid).sum()) == 7 and ref.detail(solid, np.ones_like(solid), 1)[0][0] == 6.0


def test_the_closed_form_for_one_voxel_objects_equals_the_general_reference():
    vol, px = ref.single_voxels((5, 6, 7), 200, seed=3)
    px[vol == 17] = 0
    assert np.array_equal(ref.one_voxel_rows(vol, px), ref.detail(vol, px, 200), equal_nan=True)


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle_rows(labels2d, pixels2d, n):
    res = cpm.get_intensity(labels2d, pixels2d, edge_measurements=True)
    return np.stack([np.asarray(res[k], float)[:n] for k in ref.names(True)], axis=1)


def _planes():
    from tests.sizeshape3d_ref import random_labels

    out = []
    vol, n = random_labels(31, (1, 64, 72), n_seeds=8)  # irregular touching labels
    out.append(("irregular", vol, n))
    small = np.zeros((1, 24, 40), np.uint16)  # objects of 1 to 9 pixels, some touching
    at = 0
    for k in range(1, 10):
        small.reshape(-1)[at * 41 + 1:at * 41 + 1 + k] = k
        at += 2
    small[0, 20, 5:8] = 10
    small[0, 21, 5:7] = 11  # touches 10
    out.append(("small", small, 11))
    return out


@pytest.mark.parametrize("mode", ["u16", "f32", "f32_signed"])
def test_one_plane_stacks_equal_the_oracles_get_intensity(mode):
    from tests.coloc3d_ref import noise_pixels

    for name, vol, n in _planes():
        for px in (ref.as_mode(noise_pixels(31, vol.shape)[0], mode), ref.as_mode(ref.tied_pixels(1, vol), mode)):
            got = ref.detail(vol, px, n)
            want = _oracle_rows(vol[0], px[0], n)
            assert got.shape == want.shape == (n, 13)
            for k, j in C13.items():
                if k in ref.BITWISE:
                    assert np.array_equal(got[:, j], want[:, j]), (name, mode, k)
                elif k == "Intensity_MassDisplacement":  # the oracle divides float64 sums; NaN on a dark object on both sides
                    assert np.allclose(got[:, j], want[:, j], rtol=0, atol=1e-9, equal_nan=True), (name, mode, k)
                else:
                    assert np.allclose(got[:, j], want[:, j], rtol=1e-9, atol=1e-12), (name, mode, k)


def _label_cases():
    from tests.sizeshape3d_ref import random_labels

    touching, _ = random_labels(7, (9, 20, 22), n_seeds=7)
    hole = np.zeros((5, 6, 7), np.uint16)
    hole[1:4, 1:5, 1:6] = 1
    hole[2, 2, 3] = 0
    return [("touching", touching), ("hole", hole), ("faces", ref.faces_volume()[0]), ("full", np.full((3, 4, 5), 2, np.uint16)),
            ("one plane", touching[:1]), ("one column", touching[:, :, :1])]


@pytest.mark.parametrize("case", _label_cases(), ids=[c[0] for c in _label_cases()])
def test_the_edge_voxels_are_find_boundaries_inner_on_the_3d_labels(case):
    vol = case[1]
    assert np.array_equal(ref.edge_mask(vol), cpm.find_boundaries_inner(vol))


def test_exact_ints_are_exact():
    rng = np.random.default_rng(0)
    f = np.concatenate([rng.standard_normal(500).astype(np.float32), np.asarray([0.0, 1e-30, -3e20, 1.0], np.float32)])
    m, k = ref.exact_ints(f)
    from fractions import Fraction

    assert all(Fraction(int(a)) * Fraction(2) ** k == Fraction(float(b)) for a, b in zip(m, f))
    m, k = ref.exact_ints(np.asarray([0, 65535], np.uint16))
    assert k == 0 and list(m) == [0, 65535]


def test_the_gpu_tests_inputs_have_the_stated_sizes():
    vol, n, _ = ref.power_of_two_volume()
    assert list(np.bincount(vol.ravel())[1:]) == ref.pow2_sizes() and n == 30
    vol, n, _ = ref.budget_volume(16384)
    assert list(np.bincount(vol.ravel())[1:]) == [16383, 16384, 16385, 37]
    vols, px = ref.form_pair(16384)
    assert int((vols[0] == 1).sum()) == 16384 and int((vols[1] == 1).sum()) == 16385 and px.shape == (2, 1, 6, 64, 64)
    a, b = ref.detail(vols[0], px[0, 0], 1)[0], ref.detail(vols[1], px[1, 0], 1)[0]
    same = [C13[k] for k in ref.BITWISE if "Edge" not in k]
    assert np.array_equal(a[same], b[same]) and not np.array_equal(a[:3], b[:3])
    vol, _ = ref.single_voxels()
    assert vol.shape == (40, 40, 41) and int(vol.max()) == 65535 and (np.bincount(vol.ravel())[1:] == 1).all()
    vol, n, _ = ref.faces_volume()
    kept = ref.keep_touching(vol, 7)
    assert (kept == 7).sum() == (vol == 7).sum() and kept[4, 3, 4] == 9 and not (kept == 1).any()
