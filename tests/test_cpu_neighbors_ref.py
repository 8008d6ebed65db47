"""
Pins tests/neighbors_ref.py (the restatement the GPU family `neighbors` is compared with) three ways, without a GPU: the hand values
of the worked case in include/aliby_hip.h's definition, an independent formulation with scipy.ndimage (binary_dilation with
explicitly built discs on the whole frame, center_of_mass), and the family's registration (names, registry entry, plan, C symbol).
Parity with cp_measure / CellProfiler stays unpinned: neither can be run here.
"""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import neighbors_ref as ref

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------------------------ hand values
def test_worked_case():
    got = ref.neighbors(ref.worked())
    assert got.shape == (3, 7)
    assert got[:, 0].tolist() == [1, 1, 0]  # the cross does not reach C from B
    assert got[:, 1].tolist() == [50.0, 75.0, 25.0]  # the 3 x 3 square does
    # centres: A (1.5, 1.5), B (1.5, 3.5), C (3.5, 5.5)
    assert got[0, 2:6].tolist() == [2, 2.0, 3, np.sqrt(4.0 + 16.0)]
    assert got[1, 2:6].tolist() == [1, 2.0, 3, np.sqrt(4.0 + 4.0)]
    assert got[2, 2:6].tolist() == [2, np.sqrt(8.0), 1, np.sqrt(20.0)]
    # A: B lies along +x, C at (2, 4) from A: atan2(2, 4); B: A along -x, C at (2, 2): 135 degrees
    assert np.allclose(got[:, 6], [np.degrees(np.arctan2(2.0, 4.0)), 135.0, np.degrees(np.arctan2(4.0, 12.0))], rtol=1e-14)


def test_discs_are_the_two_structuring_elements():
    assert sorted(ref.disc(1)) == [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]  # strel_disk(1): the cross
    assert len(ref.disc(1, half=True)) == 9  # strel_disk(1.5): the 3 x 3 square
    for d in (2, 5, 9, 64):
        S, T = set(ref.disc(d)), set(ref.disc(d, half=True))
        assert S < T and (d, 0) in S and (d + 1, 0) not in T
        assert all((dy * dy + dx * dx <= (d + 0.5) ** 2) == ((dy, dx) in T) for dy in range(-d - 1, d + 2) for dx in range(-d - 1, d + 2))


def test_degenerate_rows():
    sc = ref.small_scenes()
    assert ref.neighbors(sc["empty"]).shape == (0, 7)
    assert ref.neighbors(sc["one"]).tolist() == [[0, 0, 0, 0, 0, 0, 0]]
    two = ref.neighbors(sc["two"], distance=5)
    assert two[:, 0].tolist() == [1, 1] and two[:, 2].tolist() == [2, 1] and (two[:, 4:] == 0).all()
    gaps = ref.neighbors(sc["gaps"])
    assert np.isnan(gaps[[0, 2, 3, 6, 7]]).all() and not np.isnan(gaps[[1, 4, 5, 8]]).any()
    assert gaps[1, 2] == 5 and gaps[8, 0] == 0
    ring = ref.neighbors(sc["ring"], distance=2)
    assert ring[1, 2] == 1 and ring[1, 3] == 0.0 and np.isnan(ring[1, 6]) and ring[0, 2] == 2 and np.isnan(ring[0, 6])
    assert ring[2, 6] == 0.0  # both of its vectors are the same one: 0 degrees, not NaN
    cross = ref.neighbors(sc["cross"], distance=9)
    assert cross[2, [2, 4]].tolist() == [1, 2] and cross[0, [2, 4]].tolist() == [3, 2] and cross[4, [2, 4]].tolist() == [3, 2]
    assert cross[:, 0].tolist() == [0, 0, 0, 0, 0]  # 17 pixels of background between them
    far = ref.neighbors(sc["sparse"], distance=9)
    assert far[2, 0] == 0 and far[2, 1] == 0.0 and far[0, 0] == 1 and far[0, 1] == 100.0
    crowd = ref.neighbors(sc["crowd"], distance=5)
    assert crowd[0, 0] > 64


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_every_gpu_scene_has_a_restatement(distance):
    """The scenes of tests/test_gpu_neighbors.py: a row is NaN exactly where its label has no pixel, counts are whole numbers."""
    scenes = {"worked": ref.worked(), "high": ref.high_labels(), **ref.small_scenes(), **ref.big_scenes()}
    for name, lab in scenes.items():
        got = ref.expected(name, lab, distance=distance)
        present = np.isin(np.arange(1, int(lab.max()) + 1), lab)
        assert got.shape == (int(lab.max()), 7) and np.array_equal(~np.isnan(got[:, :6]).any(axis=1), present), name
        whole = got[present][:, [0, 2, 4]]
        assert (whole == np.floor(whole)).all() and ((got[present, 1] >= 0) & (got[present, 1] <= 100)).all(), name
    if distance == 9:  # the discs cover the whole 6 x 8 frame of the worked case
        assert ref.expected("worked", ref.worked(), distance=9)[:, :2].tolist() == [[2, 100], [2, 100], [2, 100]]


# --------------------------------------------------------------------------------------------------------- independent formulation
def _random_scene(seed):
    rng = np.random.default_rng(seed)
    Y, X = int(rng.integers(9, 30)), int(rng.integers(9, 30))
    lab = np.zeros((Y, X), np.uint16)
    for L in range(1, int(rng.integers(2, 9)) + 1):
        if rng.random() < 0.2:
            continue  # a gap in the numbering
        y, x = int(rng.integers(0, Y - 1)), int(rng.integers(0, X - 1))
        lab[y : y + int(rng.integers(1, 8)), x : x + int(rng.integers(1, 8))] = L  # later objects cut into earlier ones
    return lab


@pytest.mark.parametrize("seed", range(12))
def test_against_scipy(seed):
    from scipy import ndimage as ndi

    lab = _random_scene(seed)
    n = int(lab.max())
    for distance in (None, 2, 3, 7, 30):  # (30: every disc leaves the frame on every side)
        d = 1 if distance is None else distance
        got = ref.neighbors(lab, distance=distance)
        yy, xx = np.mgrid[-d : d + 1, -d : d + 1]
        S, T = yy * yy + xx * xx <= d * d, yy * yy + xx * xx <= (d + 0.5) ** 2
        edge = ref.outline(lab)
        for L in range(1, n + 1):
            mine = lab == L
            if not mine.any():
                assert np.isnan(got[L - 1]).all()
                continue
            # a pixel q reaches v through an offset of the (symmetric) disc exactly when q lies in v's dilation by it
            other = (lab != 0) & ~mine
            assert got[L - 1, 0] == len(np.unique(lab[ndi.binary_dilation(mine, S) & other]))
            t = int((ndi.binary_dilation(other, T) & mine & edge).sum())
            assert got[L - 1, 1] == t / int((mine & edge).sum()) * 100.0
            # the outline: what binary erosion by the 3 x 3 square with a background border removes
            assert np.array_equal(edge & mine, mine & ~ndi.binary_erosion(mine, np.ones((3, 3), bool), border_value=0))
        present = [L for L in range(1, n + 1) if (lab == L).any()]
        com = np.asarray(ndi.center_of_mass(np.ones(lab.shape), lab, present), np.float64).reshape(-1, 2)
        mine = ref.centres(lab, n)[[L - 1 for L in present]]
        assert np.array_equal(com.view(np.int64), mine.view(np.int64))
        for i, L in enumerate(present):
            key = ((com - com[i]) ** 2).sum(axis=1)
            order = [present[j] for j in np.lexsort((present, key)) if j != i]
            want = (order + [0, 0])[:2]
            assert got[L - 1, [2, 4]].tolist() == want


# ------------------------------------------------------------------------------------------------------------------ registration
def test_names():
    from aliby_amd.extraction import features as feat

    assert feat.neighbors_names() == feat.neighbors_names(None) == ref.names(None) == feat.family_names("neighbors")
    assert feat.neighbors_names()[0] == "Neighbors_NumberOfNeighbors_Adjacent" and feat.neighbors_names()[6] == "Neighbors_AngleBetweenNeighbors_Adjacent"
    assert feat.neighbors_names(1) == ref.names(1) and feat.neighbors_names(1)[1] == "Neighbors_PercentTouching_1"
    assert feat.neighbors_names(5) == ref.names(5) == feat.family_names("neighbors", distance=5)
    assert feat.neighbors_names(5)[2:6] == ["Neighbors_FirstClosestObjectNumber_5", "Neighbors_FirstClosestDistance_5",
                                            "Neighbors_SecondClosestObjectNumber_5", "Neighbors_SecondClosestDistance_5"]
    assert len(feat.neighbors_names(64)) == 7


def test_distance_validation_needs_no_device():
    from aliby_amd.extraction import families
    from aliby_amd.extraction import features as feat

    assert feat.neighbors_distance(None) == 1 and feat.neighbors_distance(1) == 1 and feat.neighbors_distance(np.int64(64)) == 64
    for bad in (0, 65, 2.5, -1, "3", True, 5.0):
        with pytest.raises(ValueError):
            feat.neighbors_distance(bad)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            families.plan([("None", "None", "neighbors")], {"neighbors": {"distance": bad}})


def test_registry_entry_and_plan():
    from aliby_amd.extraction import families

    fam = families.MONO["neighbors"]
    assert isinstance(fam, families.Family) and fam.needs_pixels is False and fam.after_join is False and fam.stack is False
    assert fam.names({}) == ref.names(None) and fam.names({"distance": 5}) == ref.names(5)
    assert "neighbors" in families.CP_MEASURE_NAMES and families.BUILT_KWARGS["neighbors"] == ("distance",)
    assert "neighbors" not in families.MULTI
    p = families.plan([("None", "None", "sizeshape"), ("None", "None", "neighbors")], {})
    assert p.n_cols == 78 + 7 and p.blocks[1] == (78, ref.names(None)) and p.steps[1].role == families.LAUNCH
    p = families.plan([("None", "None", "neighbors")], {"neighbors": {"distance": 5}})
    assert p.n_cols == 7 and p.blocks == [(0, ref.names(5))] and p.steps[0].kw == {"distance": 5}
    # pixel-independent: listed again under a channel, it is a copy of the first block
    p = families.plan([("None", "None", "neighbors"), (0, "max", "neighbors"), (1, "max", "intensity")], {})
    assert [s.role for s in p.steps] == [families.LAUNCH, families.COPY, families.LAUNCH] and p.copies == [(7, 0, 7)]
    with pytest.raises(NotImplementedError, match="distance_method"):
        families.plan([("None", "None", "neighbors")], {"neighbors": {"distance_method": "E"}})
    with pytest.raises(NotImplementedError, match="neighbors_labels"):
        families.plan([("None", "None", "neighbors")], {"neighbors": {"neighbors_labels": "nuclei"}})


def test_c_symbol_is_declared_and_bound():
    from aliby_amd import _lib

    header = (ROOT / "include" / "aliby_hip.h").read_text()
    assert re.search(r"\bint aliby_features_neighbors\s*\(", header)
    assert "aliby_features_neighbors" in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["aliby_features_neighbors"][1]) == 17
    assert "PARITY UNPINNED" in header[header.index("MeasureObjectNeighbors"):header.index("int aliby_features_neighbors")]
    assert hasattr(_lib.load(), "aliby_features_neighbors")
