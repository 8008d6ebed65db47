"""
`projection3d` without a device: the NumPy restatement (tests/projection3d_ref.py) against hand-written rows on stacks of at most
4 x 5 x 6, its labels against the collapse itself (max over z, sequential relabel), the column names, and the C symbol.  The same
hand cases run on the device in tests/test_gpu_projection3d.py.
"""
import numpy as np
import pytest

from tests import projection3d_ref as ref

CASES = ref.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    volume, counts, want = CASES[name]
    assert volume.shape[1] <= 4 and volume.shape[2] <= 5 and volume.shape[3] <= 6
    got = ref.projection3d(volume, counts)
    assert ref.same_rows(got, want), (got, want)


def test_hand_cases_cover_the_edges():
    assert {"single_voxel", "lower_value_fully_hidden", "partly_hidden", "reentry_counts_once", "label_without_voxels",
            "value_above_counts", "one_plane", "two_stacks"} <= set(CASES)
    hidden = CASES["lower_value_fully_hidden"][2]
    assert hidden[0].tolist() == [6.0, 0.0, 0.0, 0.0]  # label 0, visible 0, fraction 0
    one = CASES["one_plane"][2]
    seen = one[one[:, 0] > 0]
    assert (seen[:, 2] == 1.0).all() and seen[:, 3].tolist() == [1.0, 2.0, 3.0]  # Z = 1: the label is the rank
    vol, counts, rows = CASES["value_above_counts"]
    assert vol.max() > counts[0] and rows.shape == (3, 4)  # it occludes (VisibleArea below Area) and gets no row
    assert (rows[:, 1] < rows[:, 0]).any()


def test_label_is_the_value_in_the_collapsed_image():
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 7, size=(4, 5, 6)).astype(np.uint16)
    vol[rng.random(vol.shape) < 0.5] = 0
    rows = ref.projection3d(vol[None], [4])  # 5 and 6 are above the count
    flat = ref.collapse(vol)
    top = vol.max(axis=0)
    for L in range(1, 5):
        label = int(rows[L - 1, 3])
        assert rows[L - 1, 1] == (top == L).sum()
        if label:
            assert np.array_equal(flat == label, top == L)
        else:
            assert not (top == L).any()
    assert sorted(set(rows[:, 3]) - {0.0}) == sorted({float(flat[top == L][0]) for L in range(1, 5) if (top == L).any()})


def test_names_and_family():
    from aliby_amd.extraction import families
    from aliby_amd.extraction import features as feat

    names = ["Projection_Area", "Projection_VisibleArea", "Projection_VisibleFraction", "Projection_Label"]
    assert feat.projection3d_names() == names
    assert feat.family_names("projection3d") == names
    assert families.VOLUME["projection3d"].names({}) == names and not families.VOLUME["projection3d"].needs_pixels


def test_symbol_is_exported():
    from aliby_amd import _lib

    assert "aliby_features_projection3d" in _lib.exported_symbols()
    assert _lib.load().aliby_features_projection3d is not None
