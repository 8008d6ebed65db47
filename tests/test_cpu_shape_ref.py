"""
tests/shape_ref.py, the exact reference of the 2-D size/shape kernels, pinned without a GPU: to closed forms (a rectangle, a line,
a diagonal, a ring), to oracle/cp_measure_restated.py on the whole catalogue column by column, and to the stated precondition of
every input of tests/test_gpu_shape.py (areas, Euler numbers, isotropy class, launch form of each of the three kernels, raw
moments below 2^53).

Orientation is not compared by a rule that folds perpendicular axes into one: ORIENTATION lists, for each catalogue shape, the
branch of the exact rule in tile 0 and whether the float oracle lands on the exact answer in tile 0 and in the mirrored tile 1.
Where it does not, the object is isotropic in integers (I20 == I02, I11 != 0) and the oracle's float moments differ by an ulp, so
it takes the atan2 branch and returns the perpendicular axis: a documented disagreement of the oracle with the exact rule.
"""
import math

import numpy as np
import pytest

from tests import shape_ref as ref
from tests.test_gpu_object_forms import forms

C = ref.COL
NO_ORIENTATION = [n for n in ref.ALL_NAMES if n != "Orientation"]


def _one(mask, y0=3, x0=5):
    lab = np.zeros((mask.shape[0] + y0 + 2, mask.shape[1] + x0 + 4), np.uint16)
    lab[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]][mask] = 1
    r = ref.reference(lab)
    return r["values"][0], r["objects"][0]


def _val(v, name):
    return v[C[name]]


# ------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("a,b", [(1, 1), (2, 2), (3, 4), (5, 5), (6, 3), (2, 7)])
def test_rectangle(a, b):
    v, o = _one(np.ones((a, b), bool))
    assert _val(v, "Area") == a * b == _val(v, "ConvexArea") == _val(v, "BoundingBoxArea") and _val(v, "EulerNumber") == 1
    assert (_val(v, "BoundingBoxMinimum_Y"), _val(v, "BoundingBoxMaximum_Y"), _val(v, "BoundingBoxMinimum_X"), _val(v, "BoundingBoxMaximum_X")) == (3, 3 + a, 5, 5 + b)
    assert _val(v, "Center_X") == 5 + (b - 1) / 2 and _val(v, "Center_Y") == 3 + (a - 1) / 2
    assert _val(v, "Extent") == 1 and _val(v, "Solidity") == 1
    if min(a, b) >= 3:  # the border ring: every pixel of it has two or three ring neighbours on its axes (code 5, 7 ... weight 1)
        assert o["perimeter_counts"] == (2 * (a + b) - 4, 0, 0)
    assert _val(v, "MaxFeretDiameter") == math.hypot(a - 1, b - 1) and _val(v, "MinFeretDiameter") == min(a, b) - 1
    d2 = sorted(min(i + 1, a - i, j + 1, b - j) ** 2 for i in range(a) for j in range(b))
    assert o["d2"] == d2 and _val(v, "MaximumRadius") == (min(a, b) + 1) // 2
    assert _val(v, "MeanRadius") == math.fsum(math.sqrt(x) for x in d2) / (a * b)
    assert _val(v, "CentralMoment_2_0") == b * a * (a * a - 1) / 12 and _val(v, "CentralMoment_0_2") == a * b * (b * b - 1) / 12
    for name in ("CentralMoment_0_1", "CentralMoment_1_0", "CentralMoment_1_1", "CentralMoment_1_2", "CentralMoment_2_1", "CentralMoment_0_3"):
        assert _val(v, name) == 0
    l1, l2 = max(a * a - 1, b * b - 1) / 12, min(a * a - 1, b * b - 1) / 12
    assert _val(v, "InertiaTensorEigenvalues_0") == l1 and _val(v, "InertiaTensorEigenvalues_1") == l2
    assert _val(v, "InertiaTensor_0_0") == (b * b - 1) / 12 and _val(v, "InertiaTensor_1_1") == (a * a - 1) / 12 and _val(v, "InertiaTensor_0_1") == 0
    assert math.isclose(_val(v, "MajorAxisLength"), 4 * math.sqrt(l1), rel_tol=4e-16)
    assert o["branch"] == ("iso+45" if a == b else "atan2") and _val(v, "Orientation") == (45 if a == b else 0 if a > b else 90)
    assert math.isclose(_val(v, "EquivalentDiameter"), math.sqrt(4 * a * b / math.pi), rel_tol=4e-16)
    if a * b > 1:
        assert math.isclose(_val(v, "HuMoment_0"), (a * a - 1 + b * b - 1) / (12 * a * b), rel_tol=4e-16)


@pytest.mark.parametrize("n", [2, 3, 9, 40])
@pytest.mark.parametrize("vertical", [False, True])
def test_line(n, vertical):
    v, o = _one(np.ones((n, 1) if vertical else (1, n), bool))
    assert _val(v, "Area") == n == _val(v, "ConvexArea") and _val(v, "EulerNumber") == 1
    assert o["perimeter_counts"] == (n - 2, 0, 0) and _val(v, "Perimeter") == n - 2  # the two ends have one neighbour: code 3, weight 0
    if n == 2:
        assert _val(v, "FormFactor") == math.inf and _val(v, "Compactness") == 0
    else:
        assert math.isclose(_val(v, "FormFactor"), 4 * math.pi * n / (n - 2) ** 2, rel_tol=4e-16)
    assert _val(v, "MaxFeretDiameter") == n - 1 and _val(v, "MinFeretDiameter") == 0 and _val(v, "MinFeret") == 0
    assert o["d2"] == [1] * n and _val(v, "MaximumRadius") == _val(v, "MeanRadius") == _val(v, "MedianRadius") == 1
    assert _val(v, "InertiaTensorEigenvalues_0") == (n * n - 1) / 12 and _val(v, "InertiaTensorEigenvalues_1") == 0
    assert _val(v, "MinorAxisLength") == 0 and _val(v, "Eccentricity") == 1
    assert o["branch"] == "atan2" and _val(v, "Orientation") == (0 if vertical else 90)


@pytest.mark.parametrize("n", [2, 7, 33])
@pytest.mark.parametrize("down_right", [True, False])
def test_diagonal(n, down_right):
    m = np.eye(n, dtype=bool)
    v, o = _one(m if down_right else m[:, ::-1])
    assert _val(v, "Area") == n == _val(v, "ConvexArea") and _val(v, "BoundingBoxArea") == n * n and _val(v, "EulerNumber") == 1
    assert o["perimeter_counts"] == (0, n - 2, 0)  # inner pixels: two diagonal neighbours, code 21
    assert _val(v, "MaxFeretDiameter") == math.sqrt(2 * (n - 1) ** 2) and _val(v, "MinFeretDiameter") == 0
    assert o["d2"] == [1] * n
    assert _val(v, "InertiaTensorEigenvalues_0") == (n * n - 1) / 6 and _val(v, "InertiaTensorEigenvalues_1") == 0
    assert _val(v, "MinorAxisLength") == 0 and _val(v, "Eccentricity") == 1
    assert o["iso"][0] == o["iso"][1] and o["branch"] == ("iso-45" if down_right else "iso+45")
    assert _val(v, "Orientation") == (-45 if down_right else 45)


@pytest.mark.parametrize("k,t", [(5, 1), (7, 2), (9, 1)])
def test_ring(k, t):
    m = np.ones((k, k), bool)
    m[t:k - t, t:k - t] = False
    v, o = _one(m)
    assert _val(v, "Area") == k * k - (k - 2 * t) ** 2 and _val(v, "ConvexArea") == k * k and _val(v, "EulerNumber") == 0
    assert _val(v, "MaxFeretDiameter") == math.sqrt(2 * (k - 1) ** 2) and _val(v, "MinFeretDiameter") == k - 1
    assert _val(v, "MaximumRadius") == (1 if t == 1 else math.sqrt(2)) and o["branch"] == "iso+45"  # (t = 2: the pixel diagonal to the hole's corner)
    if t == 1:
        assert o["perimeter_counts"] == (4 * k - 4, 0, 0) and o["d2"] == [1] * (4 * k - 4)
    for name in ("HuMoment_2", "HuMoment_3", "HuMoment_4", "HuMoment_5", "HuMoment_6", "CentralMoment_1_1"):
        assert _val(v, name) == 0  # four-fold symmetry


def test_euler_number_counts_holes_and_components():
    v, _ = _one(np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]], bool))  # an X: one 8-connected component, no enclosed background
    assert _val(v, "EulerNumber") == 1
    v, _ = _one(np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], bool))  # a diamond: the centre is enclosed for 4-connected background
    assert _val(v, "EulerNumber") == 0


def test_names_are_the_engines_and_the_oracles():
    from aliby_amd.extraction import features as feat
    from oracle import cp_measure_restated as cpm

    assert ref.NAMES == feat.sizeshape_names() == cpm.sizeshape_names()


# ---------------------------------------------------------------------------------------------------- the catalogue's inputs
AREAS = {1: 1, 2: 2, 3: 4, 4: 9, 5: 9, 6: 7, 7: 7, 9: 40, 10: 8, 11: 18, 12: 25, 13: 9, 14: 36, 16: 28, 17: 7, 18: 12, 19: 31, 20: 11, 21: 11}
EULER = {9: 0, 10: 2, 11: -7}  # every other shape: 1
BIG_AREAS = {"diagonal80": 80, "diagonal130": 130, "arc220": 312, "arc330": 468, "line400": 400, "line650": 650}

# shape -> (branch of the exact rule in tile 0, the float oracle lands on the exact answer in tile 0, in the mirrored tile 1).
# Mirroring negates I11: an isotropic object with I11 != 0 changes sides, every other branch stays.
ORIENTATION = {
    ("small", 1): ("iso+45", True, True),
    ("small", 2): ("atan2", True, True),     # +90: I11 == 0, I20 < I02
    ("small", 3): ("iso+45", True, True),
    ("small", 4): ("atan2", True, True),     # +90
    ("small", 5): ("atan2", True, True),     # 0
    ("small", 6): ("iso-45", True, True),
    ("small", 7): ("iso+45", True, True),
    ("small", 9): ("iso+45", True, True),
    ("small", 10): ("atan2", True, True),
    ("small", 11): ("iso-45", True, True),   # the checkerboard keeps its main diagonal: I11 = 81
    ("small", 12): ("iso+45", True, True),
    ("small", 13): ("iso+45", True, True),
    ("small", 14): ("iso-45", False, True),  # the L: float a - c = -3.6e-15, the oracle returns +45 where the rule says -45
    ("small", 16): ("iso-45", True, True),   # the right triangle: isotropic with I11 != 0, and the float oracle agrees
    ("small", 17): ("atan2", True, True),
    ("small", 18): ("atan2", True, True),
    ("small", 19): ("atan2", True, True),
    ("small", 20): ("atan2", True, True),
    ("small", 21): ("atan2", True, True),
    ("diagonal80", 1): ("iso-45", True, True),
    ("diagonal130", 1): ("iso-45", True, True),
    ("arc220", 1): ("iso+45", False, False),  # symmetric under r <-> c, I11 < 0; the oracle's float moments are not: perpendicular
    ("arc330", 1): ("iso+45", False, False),
    ("line400", 1): ("atan2", True, True),
    ("line650", 1): ("atan2", True, True),
}
ISOTROPIC_WITH_MIXED_MOMENT = {("small", 6), ("small", 7), ("small", 11), ("small", 14), ("small", 16), ("diagonal80", 1), ("diagonal130", 1),
                               ("arc220", 1), ("arc330", 1)}
ISOTROPIC_WITHOUT = {("small", 1), ("small", 3), ("small", 9), ("small", 12), ("small", 13)}


def _oracle_rows(name):
    from oracle import cp_measure_restated as cpm

    rows = []
    for tile in ref.catalogue(name):
        ss, fe = cpm.get_sizeshape(tile), cpm.get_feret(tile)
        rows.append(np.column_stack([ss[k] for k in ref.NAMES] + [fe["MinFeretDiameter"], fe["MaxFeretDiameter"]]))
    return np.concatenate(rows)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_inputs_are_what_they_are_said_to_be(name):
    lab = ref.catalogue(name)
    want = ref.catalogue_reference(name)
    assert lab.shape[0] == 2 and np.array_equal(lab[1], lab[0][:, ::-1])
    if name == "small":
        assert lab.shape == (2, 64, 96) and int(lab.max()) == ref.N_SMALL and set(ref.SMALL) | set(ref.ABSENT) == set(range(1, ref.N_SMALL + 1))
        per_tile = ref.N_SMALL
        areas, euler = AREAS, EULER
        assert {a & 1 for a in AREAS.values()} == {0, 1}
        # on the frame: the corner pixel, the edges, the last corner
        t = lab[0]
        assert t[0, 0] == 1 and t[0, 4] == 2 and t[0, 95] == 3 and t[63, 2] == 4 and t[10, 0] == 5 and t[63, 95] == 18
        rows_of_10 = np.nonzero((t == 10).any(axis=1))[0]
        assert np.ptp(rows_of_10) + 1 > len(rows_of_10)  # empty rows inside the bounding box
    else:
        per_tile, areas, euler = 1, {1: BIG_AREAS[name]}, {}
    assert len(want["objects"]) == 2 * per_tile
    f = forms(*ref.table_limits(lab))
    assert (f["k_shape_core"], f["k_shape_edt"], f["k_shape_hull"]) == ref.CASES[name]
    for tile in range(2):
        for L in range(1, per_tile + 1):
            o = want["objects"][tile * per_tile + L - 1]
            if L not in areas:
                assert o is None and np.isnan(want["values"][tile * per_tile + L - 1]).all()
                continue
            v = want["values"][tile * per_tile + L - 1]
            assert o["area"] == areas[L] and v[C["EulerNumber"]] == euler.get(L, 1), (name, L)
            assert all(o["raw"][p][q] < 2 ** 53 for p in range(3) for q in range(4))
            I20, I02, I11 = o["iso"]
            if (name, L) in ISOTROPIC_WITH_MIXED_MOMENT:
                assert I20 == I02 and I11 != 0
            elif (name, L) in ISOTROPIC_WITHOUT:
                assert I20 == I02 and I11 == 0
            else:
                assert I20 != I02
            branch = ORIENTATION[name, L][0]
            if tile == 1 and I20 == I02 and I11 != 0:
                branch = {"iso-45": "iso+45", "iso+45": "iso-45"}[branch]
            assert o["branch"] == branch, (name, L, tile)
    if name == "arc330":  # a hull with many vertices: the diamond hull of a convex arc keeps a vertex for most of its rows
        assert want["values"][0, C["ConvexArea"]] > 40 * want["values"][0, C["Area"]]


def test_catalogue_reaches_every_form_of_every_kernel():
    for k in range(3):
        assert {c[k] for c in ref.CASES.values()} == {"lds", "attr", "glob"}


def test_the_l_shape_of_the_issue():
    o = ref.catalogue_reference("small")["objects"][14 - 1]
    I20, I02, I11 = o["iso"]
    assert I20 == I02 and I11 > 0 and o["branch"] == "iso-45" and o["box"] == (10, 10) and o["area"] == 36


# -------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", list(ref.CASES))
def test_reference_against_the_oracle(name):
    """Integer columns equal, the others by the rule the kernels are held to; orientation per object by the table above."""
    got = _oracle_rows(name)
    want = ref.catalogue_reference(name)
    keep = [ref.COL[n] for n in NO_ORIENTATION]
    ref.check(got[:, keep], want, f"oracle, {name}", names=NO_ORIENTATION)
    per_tile = len(want["objects"]) // 2
    k = C["Orientation"]
    for i, o in enumerate(want["objects"]):
        if o is None:
            assert np.isnan(got[i, k])
            continue
        tile, L = divmod(i, per_tile)
        lands = ORIENTATION[name, L + 1][1 + tile]
        exact = want["values"][i, k]
        if lands:
            assert abs(got[i, k] - exact) < 1e-9, (name, L + 1, tile, got[i, k], exact)
        else:  # the perpendicular axis, out of the float atan2 branch
            assert o["branch"] != "atan2" and abs(abs(got[i, k] - exact) - 90.0) < 1e-9, (name, L + 1, tile, got[i, k], exact)


# ------------------------------------------------------------------------------------------------------------ the rule bites
def test_check_refuses_what_the_old_rule_let_through():
    want = ref.catalogue_reference("small")
    good = want["values"].copy()
    ref.check(good, want, "the reference against itself", verbose=False)

    def refused(col, row, value):
        bad = good.copy()
        bad[row, C[col]] = value
        with pytest.raises(AssertionError):
            ref.check(bad, want, "mutated", verbose=False)

    refused("Orientation", 14 - 1, 45.0)                                             # the perpendicular axis of the L
    refused("Orientation", 4 - 1, -90.0)                                             # the other side of the branch cut
    refused("EulerNumber", 7 - 1, 2.0)
    refused("ConvexArea", 19 - 1, good[19 - 1, C["ConvexArea"]] + 1)
    refused("MedianRadius", 20 - 1, np.nextafter(good[20 - 1, C["MedianRadius"]], 9.0))
    refused("MaximumRadius", 20 - 1, math.sqrt(5.0))
    refused("Perimeter", 16 - 1, good[16 - 1, C["Perimeter"]] * (1 + 1e-13))
    refused("MinFeretDiameter", 6 - 1, 1e-300)                                       # 0 is bit for bit
    refused("Area", 8 - 1, 0.0)                                                      # an absent row is NaN
    refused("FormFactor", 1 - 1, 1e308)                                              # the perimeter of one pixel is 0
    refused("CentralMoment_2_1", 17 - 1, 1e-9)
    refused("MinorAxisLength", 4 - 1, 1e-5)                                          # sqrt(1e-14 * scale) is the most a line may show
