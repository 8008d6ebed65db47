"""
Pins tests/neighbors3d_ref.py (the restatement `FeatureEngine.neighbors3d` is compared with) without a GPU: the hand values of the
worked case in include/aliby_hip.h's definition, an independent formulation with scipy.ndimage (binary_dilation with explicitly built
3-D structures on the whole volume), the collapse to the 2-D restatement on one plane, the names and distances, and the C symbol.
Parity with cp_measure / CellProfiler stays unpinned: neither can be run here.
"""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import neighbors3d_ref as ref
from tests import neighbors_ref as ref2d
from tests.volume_checks import ATOL, RTOL

ROOT = Path(__file__).resolve().parents[1]


def test_worked_case():
    """A and B share a face; B and C meet along one edge across planes, offset (1, 1, 0): in T (the 18-neighbourhood), not in S."""
    assert sorted(ref.ball(1)) == sorted([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    assert len(ref.ball(1, half=True)) == 19 and (1, 1, 0) in ref.ball(1, half=True) and (1, 1, 1) not in ref.ball(1, half=True)
    lab = ref.worked()
    assert lab.shape == (4, 6, 8)
    got = ref.neighbors3d(lab)
    assert got.shape == (3, 7)
    assert got[:, 0].tolist() == [1, 1, 0]  # the cross does not reach C from B
    assert got[:, 1].tolist() == [50.0, 62.5, 25.0]  # the 18-neighbourhood does: 4 / 8, 5 / 8, 2 / 8
    assert int(ref.outline(lab).sum()) == 24  # every voxel of a 2 x 2 plane section is an outline voxel
    # centres (z, y, x): A (0.5, 1.5, 1.5), B (0.5, 1.5, 3.5), C (2.5, 3.5, 3.5)
    assert ref.centres(lab, 3).tolist() == [[0.5, 1.5, 1.5], [0.5, 1.5, 3.5], [2.5, 3.5, 3.5]]
    assert got[0, 2:6].tolist() == [2, 2.0, 3, np.sqrt(12.0)]
    assert got[1, 2:6].tolist() == [1, 2.0, 3, np.sqrt(8.0)]
    assert got[2, 2:6].tolist() == [2, np.sqrt(8.0), 1, np.sqrt(12.0)]
    # A: B along +x, C at (2, 2, 2); B: A along -x, C at (2, 2, 0): a right angle; C: B at (-2, -2, 0), A at (-2, -2, -2)
    want = [np.degrees(np.arctan2(np.sqrt(32.0), 4.0)), 90.0, np.degrees(np.arctan2(np.sqrt(32.0), 8.0))]
    assert np.allclose(got[:, 6], want, rtol=1e-14)
    # planes above and below make no outline voxel: a 3 x 3 x 3 block's centre voxel of every plane stays inside
    block = np.zeros((5, 7, 7), np.uint16)
    block[1:4, 2:5, 2:5] = 1
    assert int(ref.outline(block).sum()) == 3 * 8
    assert ref.neighbors3d(ref.small_scenes()["full"][0])[0].tolist() == [0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_against_scipy(distance):
    from scipy import ndimage as ndi

    d = 1 if distance is None else distance
    zz, yy, xx = np.mgrid[-d : d + 1, -d : d + 1, -d : d + 1]
    r2 = zz * zz + yy * yy + xx * xx
    S, T = r2 <= d * d, r2 <= (d + 0.5) ** 2
    assert int(S.sum()) == len(ref.ball(d)) and int(T.sum()) == len(ref.ball(d, half=True))
    square = np.ones((1, 3, 3), bool)
    scenes = {"worked": (ref.worked(), 3), "cap": (ref.cap_scene(), 4), **ref.small_scenes()}
    for name, (lab, n) in scenes.items():
        got = ref.expected(name, lab, n=n, distance=distance)
        assert got.shape == (n, 7), name
        edge = ref.outline(lab)
        present = [L for L in range(1, n + 1) if (lab == L).any()]
        assert np.array_equal(~np.isnan(got).all(axis=1), np.isin(np.arange(1, n + 1), present)), name
        for L in present[:12]:  # (the crowd's one-voxel objects are all alike)
            mine = lab == L
            # a voxel q reaches v through an offset of the (symmetric) ball exactly when q lies in v's dilation by it
            other = (lab != 0) & ~mine
            reach = np.unique(lab[ndi.binary_dilation(mine, S, border_value=0) & other])
            assert got[L - 1, 0] == int((reach <= n).sum()), (name, L)
            t = int((ndi.binary_dilation(other, T, border_value=0) & mine & edge).sum())
            assert got[L - 1, 1] == t / int((mine & edge).sum()) * 100.0, (name, L)
            # the outline: what erosion by the in-plane 3 x 3 square with a background border removes
            assert np.array_equal(edge & mine, mine & ~ndi.binary_erosion(mine, square, border_value=0)), (name, L)
        if present:
            com = np.asarray(ndi.center_of_mass(np.ones(lab.shape), lab, present), np.float64).reshape(-1, 3)
            assert np.allclose(com, ref.centres(lab, n)[[L - 1 for L in present]], rtol=1e-13, atol=0), name
            com = ref.centres(lab, n)[[L - 1 for L in present]]
            for i, L in enumerate(present[:12]):
                dz, dy, dx = (com - com[i]).T
                key = (dz * dz + dy * dy) + dx * dx
                order = [present[j] for j in np.lexsort((present, key)) if j != i]
                assert got[L - 1, [2, 4]].tolist() == (order + [0, 0])[:2], (name, L)
                assert got[L - 1, [3, 5]].tolist() == (np.sqrt(np.sort(np.delete(key, i))).tolist() + [0, 0])[:2], (name, L)
    if distance is None:  # what the scenes are there for
        sc = {k: ref.expected(k, *v, distance=None) for k, v in ref.small_scenes().items()}
        assert sc["one"].tolist() == [[0.0] * 7] and (sc["two"][:, 4:] == 0).all() and sc["two"][:, 2].tolist() == [2, 1]
        assert sc["shell"][1, 2] == 1 and sc["shell"][1, 3] == 0.0 and np.isnan(sc["shell"][[0, 1], 6]).all() and sc["shell"][2, 6] == 0.0
        assert sc["cross"][3, [2, 4]].tolist() == [1, 2] and sc["cross"][0, [2, 4]].tolist() == [4, 2] and sc["cross"][6, [2, 4]].tolist() == [4, 2]
        assert np.isnan(sc["gaps"][[0, 2, 3, 6, 7]]).all() and not np.isnan(sc["gaps"][[1, 4, 5, 8]]).any()
        above = ref.small_scenes()["above"][0]
        without = ref.neighbors3d(np.where(above > 2, 0, above), n=2)
        assert sc["above"].shape == (2, 7) and sc["above"][:, 0].tolist() == without[:, 0].tolist() == [1, 1]  # 7 and 9 are not counted
        assert (sc["above"][:, 1] > without[:, 1]).all()  # but touched
        assert sc["sparse"][0, 0] == 1 and sc["sparse"][0, 1] == 100.0 and sc["sparse"][2, :2].tolist() == [0, 0]
    if distance == 5:
        assert ref.expected("crowd", *ref.small_scenes()["crowd"], distance=5)[0, 0] > 64


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_one_plane_is_the_2d_family(distance):
    """On [1, 64, 64] the definition collapses to the 2-D one: columns 0-5 exactly, the angle within the project's parity rule."""
    for name, lab in ref2d.small_scenes().items():
        want = ref2d.expected(name, lab, distance=distance)
        got = ref.neighbors3d(lab[None], distance=distance)
        assert got.shape == want.shape, name
        assert np.array_equal(got[:, :6].view(np.int64), np.ascontiguousarray(want[:, :6]).view(np.int64)), name
        assert np.array_equal(np.isnan(got[:, 6]), np.isnan(want[:, 6])), name
        assert np.allclose(got[:, 6], want[:, 6], rtol=RTOL, atol=ATOL, equal_nan=True), name


def test_names_and_distances():
    from aliby_amd.extraction import features as feat

    assert feat.neighbors3d_names() == feat.neighbors3d_names(None) == ref.names(None) == feat.neighbors_names()
    assert feat.neighbors3d_names()[0] == "Neighbors_NumberOfNeighbors_Adjacent" and feat.neighbors3d_names()[6] == "Neighbors_AngleBetweenNeighbors_Adjacent"
    assert feat.neighbors3d_names(1) == ref.names(1) and feat.neighbors3d_names(1)[1] == "Neighbors_PercentTouching_1"
    assert feat.neighbors3d_names(5) == ref.names(5) == feat.neighbors_names(5) and len(feat.neighbors3d_names(16)) == 7
    assert feat.NEIGHBORS3D_MAX_DISTANCE == 16
    assert feat.neighbors3d_distance(None) == 1 and feat.neighbors3d_distance(1) == 1 and feat.neighbors3d_distance(np.int64(16)) == 16
    for bad in (0, 17, 2.5, True, "3", -1, 5.0):
        with pytest.raises(ValueError):
            feat.neighbors3d_distance(bad)
        with pytest.raises(ValueError):
            feat.neighbors3d_names(bad)


def test_c_symbol_is_declared_and_bound():
    from aliby_amd import _lib

    header = (ROOT / "include" / "aliby_hip.h").read_text()
    m = re.search(r"\bint aliby_features_neighbors3d\s*\(([^;]*)\)\s*;", header)
    assert m
    assert "aliby_features_neighbors3d" in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["aliby_features_neighbors3d"][1]) == len(m.group(1).split(",")) == 13
    comment = header[header.index('"neighbors3d"'):m.start()]
    assert "PARITY UNPINNED" in comment and "Expand until adjacent" in comment and "[4, 6, 8]" in comment
    assert hasattr(_lib.load(), "aliby_features_neighbors3d")
