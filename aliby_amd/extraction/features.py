"""
Feature-family column layouts shared by the HIP kernels (aliby_amd/csrc/feat_*.hip) and the host.

Key names follow what the reference's tables show for cp_measure output
(examples/01_cell_painting_tiff.py:159-162: "0/max/intensity/Intensity_IntegratedIntensity") and
CellProfiler's published measurement names; cp_measure 0.1.17 itself is not in the container, so the
exact spelling of keys beyond that pattern is "parity unpinned" (SURVEY.md §8c).  The column-count
identity 4 + 6*S + 5*I + 10*P = 632 quoted at examples/01:156-158 is reproduced with S=78, I=16, P=8.
"""

from __future__ import annotations

import math
import numbers
from typing import NamedTuple

INTENSITY_CORE = [
    "Intensity_IntegratedIntensity",
    "Intensity_MeanIntensity",
    "Intensity_StdIntensity",
    "Intensity_MinIntensity",
    "Intensity_MaxIntensity",
]
INTENSITY_EDGE = [
    "Intensity_IntegratedIntensityEdge",
    "Intensity_MeanIntensityEdge",
    "Intensity_StdIntensityEdge",
    "Intensity_MinIntensityEdge",
    "Intensity_MaxIntensityEdge",
]
INTENSITY_TAIL = [
    "Intensity_MassDisplacement",
    "Intensity_LowerQuartileIntensity",
    "Intensity_MedianIntensity",
    "Intensity_MADIntensity",
    "Intensity_UpperQuartileIntensity",
    "Location_CenterMassIntensity_X",
    "Location_CenterMassIntensity_Y",
    "Location_CenterMassIntensity_Z",
    "Location_MaxIntensity_X",
    "Location_MaxIntensity_Y",
    "Location_MaxIntensity_Z",
]


def intensity_names(edge_measurements: bool = True) -> list[str]:
    """Column order written by k_intensity (feat_intensity.hip)."""
    return INTENSITY_CORE + (INTENSITY_EDGE if edge_measurements else []) + INTENSITY_TAIL


SIZESHAPE_BASIC = [
    "Area",
    "BoundingBoxArea",
    "BoundingBoxMaximum_X",
    "BoundingBoxMaximum_Y",
    "BoundingBoxMinimum_X",
    "BoundingBoxMinimum_Y",
    "Center_X",
    "Center_Y",
    "Compactness",
    "ConvexArea",
    "Eccentricity",
    "EquivalentDiameter",
    "EulerNumber",
    "Extent",
    "FormFactor",
    "MajorAxisLength",
    "MaxFeretDiameter",
    "MaximumRadius",
    "MeanRadius",
    "MedianRadius",
    "MinFeretDiameter",
    "MinorAxisLength",
    "Orientation",
    "Perimeter",
    "Solidity",
]


def sizeshape_names() -> list[str]:
    """Column order written by k_shape_* (feat_shape.hip): 25 basic + 53 advanced = 78."""
    names = list(SIZESHAPE_BASIC)
    names += [f"SpatialMoment_{p}_{q}" for p in range(3) for q in range(4)]
    names += [f"CentralMoment_{p}_{q}" for p in range(3) for q in range(4)]
    names += [f"NormalizedMoment_{p}_{q}" for p in range(4) for q in range(4)]
    names += [f"HuMoment_{k}" for k in range(7)]
    names += [f"InertiaTensor_{i}_{j}" for i in range(2) for j in range(2)]
    names += [f"InertiaTensorEigenvalues_{k}" for k in range(2)]
    assert len(names) == 78
    return names


def zernike_indexes(limit: int = 10) -> list[tuple[int, int]]:
    """(n, m) pairs with n < limit and m = n%2, n%2+2, .., n  (centrosome.zernike.get_zernike_indexes)."""
    return [(n, m) for n in range(limit) for m in range(n % 2, n + 1, 2)]


def zernike_names() -> list[str]:
    return [f"Zernike_{n}_{m}" for n, m in zernike_indexes()]


def feret_names() -> list[str]:
    return ["MinFeretDiameter", "MaxFeretDiameter"]


HARALICK = [
    "AngularSecondMoment",
    "Contrast",
    "Correlation",
    "Variance",
    "InverseDifferenceMoment",
    "SumAverage",
    "SumVariance",
    "SumEntropy",
    "Entropy",
    "DifferenceVariance",
    "DifferenceEntropy",
    "InfoMeas1",
    "InfoMeas2",
]


def texture_names(scale: int = 3, gray_levels: int = 256) -> list[str]:
    """13 Haralick statistics x 4 directions; direction-major like mahotas' (4, 13) result."""
    return [f"{h}_{scale}_{d:02d}_{gray_levels}" for d in range(4) for h in HARALICK]


def radial_distribution_names(bin_count: int = 4, scaled: bool = True) -> list[str]:
    """scaled=False adds CellProfiler's overflow ring (everything beyond maximum_radius) as `<stat>_Overflow`."""
    out = []
    for stat in ("FracAtD", "MeanFrac", "RadialCV"):
        out += [f"RadialDistribution_{stat}_{b}of{bin_count}" for b in range(1, bin_count + 1)]
        if not scaled:
            out.append(f"RadialDistribution_{stat}_Overflow")
    return out


def granularity_names(granular_spectrum_length: int = 16) -> list[str]:
    return [f"Granularity_{i}" for i in range(1, int(granular_spectrum_length) + 1)]


def radial_zernike_names() -> list[str]:
    out = [f"RadialDistribution_ZernikeMagnitude_{n}_{m}" for n, m in zernike_indexes()]
    out += [f"RadialDistribution_ZernikePhase_{n}_{m}" for n, m in zernike_indexes()]
    return out


NEIGHBORS_MAX_DISTANCE = 64  # bounds the per-pixel scan of csrc/feat_neighbors.hip; not a structural limit
NEIGHBORS3D_MAX_DISTANCE = 16  # bounds the per-voxel scan of csrc/feat_neighbors3d.hip (about 19 k offsets at 16); not a structural limit


def _neighbors_distance(family: str, cap: int, distance) -> int:
    if distance is None:
        return 1
    if isinstance(distance, bool) or not isinstance(distance, numbers.Integral) or not 1 <= int(distance) <= cap:
        raise ValueError(f"{family}: distance must be None or an integer in 1..{cap}, got {distance!r}")
    return int(distance)


def _neighbors_names(suffix: str) -> list[str]:
    return [f"Neighbors_{n}_{suffix}" for n in ("NumberOfNeighbors", "PercentTouching", "FirstClosestObjectNumber", "FirstClosestDistance",
                                                "SecondClosestObjectNumber", "SecondClosestDistance", "AngleBetweenNeighbors")]


def neighbors_distance(distance=None) -> int:
    """The pixel distance d of the `neighbors` family: None -> 1 (CellProfiler's "Adjacent"), else an integer in 1..64.  Anything
    else is a ValueError.  Needs no device."""
    return _neighbors_distance("neighbors", NEIGHBORS_MAX_DISTANCE, distance)


def neighbors_names(distance=None) -> list[str]:
    """Columns of the `neighbors` family (csrc/feat_neighbors.hip): CellProfiler's MeasureObjectNeighbors with the objects as their own
    neighbours, which cp_measure carries among its multi-mask measurements.  The suffix is "Adjacent" for distance=None (d = 1),
    else str(d).  PARITY UNPINNED: the definition (include/aliby_hip.h, tests/neighbors_ref.py) is recalled from CellProfiler 4 and
    centrosome, neither of which can be run beside this package.  AngleBetweenNeighbors is atan2(|v1 x v2|, v1 . v2), not
    CellProfiler's arccos of the normalised dot product: the same angle, well-conditioned near 0 and 180 degrees (deliberate).
    Not built: "Expand until adjacent", neighbours from a second object set, distances above 64."""
    return _neighbors_names("Adjacent" if distance is None else str(neighbors_distance(distance)))


SECONDARY_MAX_DISTANCE = 64  # bounds the row scan of csrc/feat_secondary.hip; not a structural limit


def secondary_distance(distance) -> int:
    """The N of "Distance - N" (FeatureEngine.secondary_labels, a `secondary_<name>` step): an integer in 1..64, or a float that holds
    one (5.0, as a settings file may spell it).  A bool, any other float, 0, 65 and anything that is not a number are ValueErrors.
    Needs no device."""
    ok = not isinstance(distance, bool) and (isinstance(distance, numbers.Integral)
                                             or (isinstance(distance, numbers.Real) and float(distance).is_integer()))
    if not ok or not 1 <= int(distance) <= SECONDARY_MAX_DISTANCE:
        raise ValueError(f"secondary: distance must be an integer in 1..{SECONDARY_MAX_DISTANCE}, got {distance!r}")
    return int(distance)


SECONDARY3D_MAX_DISTANCE = 255  # N^2 fits the 16-bit distance field of csrc/feat_secondary3d.hip's packed key
SECONDARY3D_MAX_REACH = 64  # voxels along one axis: bounds the scans of csrc/feat_secondary3d.hip; not a structural limit


def secondary_volume_args(distance, spacing=(1, 1, 1)) -> tuple:
    """(N, (sz, sy, sx)) of FeatureEngine.secondary_volume and a `volumesecondary_<name>` step, checked.  N: an integer in 1..255 in
    the units of the lattice, or a float that holds one (as `secondary_distance` takes 5.0).  spacing: three integers in 1..255 — a
    float spacing is refused, also one that holds integers: with integer steps every distance is an exact integer (13 : 5 : 5 stands
    for 0.6 um per plane over 0.23 um per pixel).  The reach N // s must be at most 64 voxels on every axis.  A bool, a str, None and
    anything else are ValueErrors.  Needs no device."""
    ok = not isinstance(distance, bool) and (isinstance(distance, numbers.Integral)
                                             or (isinstance(distance, numbers.Real) and float(distance).is_integer()))
    if not ok or not 1 <= int(distance) <= SECONDARY3D_MAX_DISTANCE:
        raise ValueError(f"secondary_volume: distance must be an integer in 1..{SECONDARY3D_MAX_DISTANCE}, got {distance!r}")
    n = int(distance)
    try:
        steps = None if isinstance(spacing, (str, bytes)) else tuple(spacing)
    except TypeError:
        steps = None
    if steps is None or len(steps) != 3 or any(isinstance(s, bool) or not isinstance(s, numbers.Integral) or not 1 <= int(s) <= 255
                                               for s in steps):
        raise ValueError(f"secondary_volume: spacing must be three integers (sz, sy, sx) in 1..255 (no float spacing), got {spacing!r}")
    steps = tuple(int(s) for s in steps)
    if any(n // s > SECONDARY3D_MAX_REACH for s in steps):
        raise ValueError(f"secondary_volume: distance {n} over spacing {steps} reaches more than {SECONDARY3D_MAX_REACH} voxels along "
                         "an axis")
    return n, steps


PROPAGATE_MAX_SCALED_LAMBDA = 1 << 20  # regularization * image_max: its square fits the weights of csrc/feat_propagate.hip


def _whole_number(value) -> bool:
    return not isinstance(value, bool) and (isinstance(value, numbers.Integral)
                                            or (isinstance(value, numbers.Real) and float(value).is_integer()))


PROPAGATE_OPTIONS = ("threshold", "regularization", "distance", "image_max")  # what a `propagate_<name>` step takes beside `channel`


class PropagateArgs(NamedTuple):
    threshold: int
    regularization: float
    distance: int | None
    image_max: int
    lambda2: int

    def options(self, given=PROPAGATE_OPTIONS) -> dict:
        """The checked values of the options named in `given`, by name."""
        return {key: getattr(self, key) for key in PROPAGATE_OPTIONS if key in given}


def propagate_channel(channel) -> int:
    """The stain channel of a `propagate_<name>` step: a non-negative integer (no bool, no float), else a ValueError."""
    if isinstance(channel, bool) or not isinstance(channel, numbers.Integral) or channel < 0:
        raise ValueError(f"propagate: channel must be a non-negative integer, got {channel!r}")
    return int(channel)


def propagate_args(threshold=0, regularization=0.05, distance=None, image_max=65535) -> PropagateArgs:
    """(threshold, regularization, distance, image_max, lambda2) of FeatureEngine.propagate_labels and a `propagate_<name>` step,
    checked, as a named tuple.  threshold: an integer in 0..65535 (a grey level of the uint16 image; pixels at or above it are passable).
    regularization: a finite float >= 0 (CellProfiler's, 0.05 by default).  distance: None, or an integer in 1..64 that keeps the
    objects within that many pixels of their seeds ("Distance - B" is threshold 0 with a distance).  image_max: an integer in
    1..65535, the grey level that CellProfiler's 0..1 scale maps to 1.  Integers may come as floats that hold one (400.0).
    lambda2 = round((regularization * image_max)^2) in float64, half to even, the integer the kernels add per step;
    regularization * image_max must be at most 2^20.  A bool, a str, a non-finite value and anything out of range are ValueErrors
    that say what is allowed.  Needs no device."""
    if not _whole_number(threshold) or not 0 <= int(threshold) <= 65535:
        raise ValueError(f"propagate: threshold must be an integer in 0..65535, got {threshold!r}")
    if isinstance(regularization, bool) or not isinstance(regularization, numbers.Real) or not math.isfinite(float(regularization)) \
            or float(regularization) < 0:
        raise ValueError(f"propagate: regularization must be a finite number >= 0, got {regularization!r}")
    if distance is not None and (not _whole_number(distance) or not 1 <= int(distance) <= SECONDARY_MAX_DISTANCE):
        raise ValueError(f"propagate: distance must be None or an integer in 1..{SECONDARY_MAX_DISTANCE}, got {distance!r}")
    if not _whole_number(image_max) or not 1 <= int(image_max) <= 65535:
        raise ValueError(f"propagate: image_max must be an integer in 1..65535, got {image_max!r}")
    scaled = float(regularization) * float(int(image_max))
    if scaled > PROPAGATE_MAX_SCALED_LAMBDA:
        raise ValueError(f"propagate: regularization * image_max must be at most 2^20, got {regularization!r} * {image_max!r}")
    return PropagateArgs(int(threshold), float(regularization), None if distance is None else int(distance), int(image_max),
                         int(round(scaled * scaled)))


AUTO_THRESHOLD_OPTIONS = ("method", "classes", "middle", "correction", "bounds")  # the keys of an `auto_threshold` option dict
AUTO_THRESHOLD_NOT_BUILT = ("mce", "minimum_cross_entropy", "li")
AUTO_THRESHOLD_MIDDLE = ("foreground", "background")  # ALIBY_THRESHOLD_MIDDLE_* of include/aliby_hip.h, by index
AUTO_THRESHOLD_MAX_CORRECTION = 16.0


class AutoThresholdArgs(NamedTuple):
    method: str
    classes: int
    middle: str | None  # None with two classes, which have no middle class
    correction: float
    bounds: tuple

    def options(self, given=AUTO_THRESHOLD_OPTIONS) -> dict:
        """The checked values of the options named in `given`, by name (bounds as a list: what a saved step holds; no `middle` with
        two classes).  auto_threshold_options takes the dict back."""
        values = {**self._asdict(), "bounds": list(self.bounds)}
        return {key: values[key] for key in AUTO_THRESHOLD_OPTIONS if key in given and values[key] is not None}

    @property
    def middle_code(self) -> int:
        """ALIBY_THRESHOLD_MIDDLE_* of include/aliby_hip.h (not used with two classes: foreground)."""
        return AUTO_THRESHOLD_MIDDLE.index(self.middle or "foreground")


def auto_threshold_args(method="otsu", classes=2, middle=None, correction=1.0, bounds=(0, 65535)) -> AutoThresholdArgs:
    """(method, classes, middle, correction, bounds) of FeatureEngine.auto_threshold and the `auto_threshold` option of a
    `propagate_<name>` step, checked, as a named tuple.  method: "otsu" (minimum cross-entropy — "mce", "minimum_cross_entropy", "li" —
    is not built).  classes: 2 or 3.  middle: with three classes, "foreground" (the default: the middle class counts as foreground,
    the lower threshold) or "background" (the upper one); with two classes it must not be given and stays None in the tuple, so
    that a checked tuple, and its options(), pass these checks again.  correction: a finite float in
    (0, 16], CellProfiler's threshold correction factor.  bounds: two whole numbers 0 <= lo <= hi <= 65535 that the corrected
    threshold is clamped to.  A bool, a str in a number's place and anything out of range are ValueErrors that say what is allowed.
    Needs no device."""
    if not isinstance(method, str) or method != "otsu":
        if isinstance(method, str) and method in AUTO_THRESHOLD_NOT_BUILT:
            raise ValueError(f"auto_threshold: method {method!r} (minimum cross-entropy) is not built: only 'otsu' is")
        raise ValueError(f"auto_threshold: method must be 'otsu', got {method!r}")
    if isinstance(classes, bool) or not isinstance(classes, numbers.Integral) or int(classes) not in (2, 3):
        raise ValueError(f"auto_threshold: classes must be 2 or 3, got {classes!r}")
    if int(classes) == 2 and middle is not None:
        raise ValueError(f"auto_threshold: middle is an option of three classes only (classes=3), got {middle!r} with classes=2")
    if middle is None and int(classes) == 3:
        middle = "foreground"
    if middle is not None and (not isinstance(middle, str) or middle not in AUTO_THRESHOLD_MIDDLE):
        raise ValueError(f"auto_threshold: middle must be 'foreground' or 'background', got {middle!r}")
    if isinstance(correction, bool) or not isinstance(correction, numbers.Real) or not math.isfinite(float(correction)) \
            or not 0.0 < float(correction) <= AUTO_THRESHOLD_MAX_CORRECTION:
        raise ValueError(f"auto_threshold: correction must be a finite number in (0, 16], got {correction!r}")
    if not isinstance(bounds, (tuple, list)) or len(bounds) != 2 or not all(_whole_number(b) for b in bounds) \
            or not 0 <= int(bounds[0]) <= int(bounds[1]) <= 65535:
        raise ValueError(f"auto_threshold: bounds must be two whole numbers (lo, hi) with 0 <= lo <= hi <= 65535, got {bounds!r}")
    return AutoThresholdArgs("otsu", int(classes), middle, float(correction), (int(bounds[0]), int(bounds[1])))


def auto_threshold_options(options) -> AutoThresholdArgs:
    """auto_threshold_args of an option dict {"method", "classes", "middle", "correction", "bounds"}; anything but a dict, and an
    unknown key, are ValueErrors that name the keys allowed."""
    if not isinstance(options, dict) or set(options) - set(AUTO_THRESHOLD_OPTIONS):
        raise ValueError(f"auto_threshold: the options must be a dict with keys of {list(AUTO_THRESHOLD_OPTIONS)}, got {options!r}")
    return auto_threshold_args(**options)


def relate_names(other: str) -> list[str]:
    """Columns of `FeatureEngine.relate` for rows related to the object set `other` (csrc/feat_relate.hip): CellProfiler's
    RelateObjects — the parent in `other`, the overlap that chose it, the number of children in `other`, the distance between the
    centres and the distance from the centre to the parent's outline.  PARITY UNPINNED: the definition (include/aliby_hip.h,
    tests/relate_ref.py) is recalled from CellProfiler 4 and centrosome, neither of which can be run beside this package.
    ParentOverlap is an extension.  `other` is a non-empty string without "_" (a step's object name is what follows the last "_"
    of its name) and without "/" (the column separator): anything else is a ValueError.  Needs no device.
    Not built: per-parent means of child measurements, "Expand until adjacent" and `neighbors` against a second object set, the
    batched run_positions form.  (Volume labels: `relate3d_names`.)"""
    if not isinstance(other, str) or not other or "_" in other or "/" in other:
        raise ValueError(f"relate: the other object set's name must be a non-empty string without '_' or '/', got {other!r}")
    return [f"Parent_{other}", f"ParentOverlap_{other}", f"Children_{other}_Count", f"Distance_Centroid_{other}",
            f"Distance_Minimum_{other}"]


def relate3d_names(other: str) -> list[str]:
    """Columns of `FeatureEngine.relate3d` for rows related to the object set `other` (csrc/feat_relate3d.hip): the five of
    `relate_names`, on volume labels — overlaps in voxels, distances in the units of the call's `spacing`, the parent's outline taken
    plane by plane.  PARITY UNPINNED like the 2-D family (include/aliby_hip.h, tests/relate3d_ref.py).  Needs no device."""
    return relate_names(other)


COLOC = {
    "pearson": ["Correlation_Pearson", "Correlation_Slope"],
    "manders_fold": ["Correlation_Manders_1", "Correlation_Manders_2"],
    "rwc": ["Correlation_RWC_1", "Correlation_RWC_2"],
    "costes": ["Correlation_Costes_1", "Correlation_Costes_2"],
}


def family_names(family: str, **kw) -> list[str]:
    if family == "intensity":
        return intensity_names(kw.get("edge_measurements", True))
    if family == "sizeshape":
        return sizeshape_names()
    if family == "zernike":
        return zernike_names()
    if family == "feret":
        return feret_names()
    if family == "texture":
        return texture_names(kw.get("scale", 3), kw.get("gray_levels", 256))
    if family == "radial_distribution":
        return radial_distribution_names(kw.get("bin_count", 4), kw.get("scaled", True))
    if family == "radial_zernikes":
        return radial_zernike_names()
    if family == "neighbors":
        return neighbors_names(kw.get("distance"))
    if family in COLOC:
        return list(COLOC[family])
    # the volume families (extraction.families.VOLUME)
    if family == "intensity3d":
        return intensity3d_names()
    if family == "intensity3d_detail":
        return intensity3d_detail_names(kw.get("edge_measurements", True))
    if family == "sizeshape3d":
        return sizeshape3d_names(kw.get("surface_area", False))
    if family == "texture3d":
        return texture3d_names(kw.get("scale", 3), kw.get("gray_levels", 256))
    if family == "neighbors3d":
        return neighbors3d_names(kw.get("distance"))
    if family == "granularity3d":
        return granularity3d_names(kw.get("granular_spectrum_length", 16))
    if family == "projection3d":
        return projection3d_names()
    raise KeyError(family)


def intensity3d_names() -> list[str]:
    """Round-3 extension (a Z-stack measured as a volume; beyond what the reference wires): the moment-based
    statistics of CellProfiler's MeasureObjectIntensity on volumes, named as cp_measure's 2-D `intensity` names them."""
    return ["Volume", "Intensity_IntegratedIntensity", "Intensity_MeanIntensity", "Intensity_StdIntensity", "Intensity_MinIntensity",
            "Intensity_MaxIntensity", "Location_CenterMassIntensity_X", "Location_CenterMassIntensity_Y", "Location_CenterMassIntensity_Z",
            "Location_Center_X", "Location_Center_Y", "Location_Center_Z"]


def intensity3d_detail_names(edge_measurements: bool = True) -> list[str]:
    """Columns of `FeatureEngine.intensity3d_detail` (csrc/feat_intensity3d_detail.hip): `intensity_names(edge_measurements)` without
    the columns `intensity3d` already gives, in that order: the five edge statistics (only with the flag), MassDisplacement, the
    quartiles, median and MAD, and the position of the maximum.  13 columns, or 8.  torch.cat([intensity3d, intensity3d_detail], 1)
    is then the 2-D family's whole column set plus Volume and Location_Center_*.  Parity with cp_measure on volumes is unpinned, like
    the other 3-D families."""
    if not isinstance(edge_measurements, bool):
        raise TypeError(f"edge_measurements must be a bool, got {edge_measurements!r}")
    given = set(intensity3d_names())
    return [name for name in intensity_names(edge_measurements) if name not in given]


def sizeshape3d_names(surface_area: bool = False) -> list[str]:
    """Size and shape of volume labels (csrc/feat_sizeshape3d.hip), named after CellProfiler's 3-D MeasureObjectSizeShape (the
    names cp_measure's `sizeshape` uses for 3-D input; parity with it is unpinned, like intensity3d).  19 columns; with
    `surface_area=True` "SurfaceArea" is appended as column 19 (csrc/feat_surface3d.hip).  That column is opt-in and pinned to
    scikit-image 0.18.3's Lewiner marching-cubes mesh at level 0, the function CellProfiler calls, through a table of per-cell
    areas recorded from it (tests/golden/skimage_marching_cubes_level0.json); at level 0 the vertices sit on the centres of the
    outside voxels, so a single voxel measures 4 sqrt(3), not 6.  Solidity stays absent: a 3-D convex hull has nothing to be exact
    with here."""
    names = ["Volume", "BoundingBoxMinimum_X", "BoundingBoxMinimum_Y", "BoundingBoxMinimum_Z", "BoundingBoxMaximum_X", "BoundingBoxMaximum_Y",
             "BoundingBoxMaximum_Z", "BoundingBoxVolume", "Center_X", "Center_Y", "Center_Z", "Extent", "EquivalentDiameter", "EulerNumber",
             "MajorAxisLength", "MinorAxisLength", "InertiaTensorEigenvalues_0", "InertiaTensorEigenvalues_1", "InertiaTensorEigenvalues_2"]
    return names + ["SurfaceArea"] if surface_area else names


def coloc3d_names(pairs, metrics=("pearson", "manders_fold", "rwc", "costes")) -> list[str]:
    """Columns of `FeatureEngine.coloc3d` (csrc/feat_coloc3d.hip): for every channel pair, in the order given, the two columns of
    every metric, in the order given: "(c0, c1)/<metric>/<name>", e.g. "(0, 1)/pearson/Correlation_Pearson".  That is the 2-D
    multi tree's key "(c0, c1)/<reduction>/<z reduction>/<metric>/<name>" without the two reductions a volume has no use for.
    The names are cp_measure's 2-D ones; parity with cp_measure on volumes is unpinned, like the other 3-D families."""
    metrics = list(metrics)
    unknown = [m for m in metrics if m not in COLOC]
    if unknown or not metrics or len(set(metrics)) != len(metrics):
        raise ValueError(f"metrics must be distinct names out of {sorted(COLOC)}, got {metrics!r}")
    out = []
    for pair in pairs:
        if len(pair) != 2:
            raise ValueError(f"a channel pair is (c0, c1), got {pair!r}")
        c0, c1 = int(pair[0]), int(pair[1])
        if c0 == c1 or c0 < 0 or c1 < 0:
            raise ValueError(f"a channel pair needs two different non-negative channels, got {pair!r}")
        out += [f"({c0}, {c1})/{m}/{name}" for m in metrics for name in COLOC[m]]
    return out


def texture3d_names(scale: int = 3, gray_levels: int = 256) -> list[str]:
    """Columns of `FeatureEngine.texture3d` (csrc/feat_texture3d.hip): the 13 Haralick statistics x 13 directions, direction-major,
    named as the 2-D `texture_names` names its 4 (mahotas' (13, 13) result on a 3-D array).  Which direction a block index stands
    for is the kernel's table (the header of feat_texture3d.hip); that order and parity with cp_measure are unpinned."""
    return [f"{h}_{scale}_{d:02d}_{gray_levels}" for d in range(13) for h in HARALICK]


def neighbors3d_distance(distance=None) -> int:
    """The voxel distance d of `FeatureEngine.neighbors3d`: None -> 1 (CellProfiler's "Adjacent"), else an integer in 1..16.  Anything
    else is a ValueError.  Needs no device."""
    return _neighbors_distance("neighbors3d", NEIGHBORS3D_MAX_DISTANCE, distance)


def neighbors3d_names(distance=None) -> list[str]:
    """Columns of `FeatureEngine.neighbors3d` (csrc/feat_neighbors3d.hip): the seven of `neighbors_names`, on volume labels.  The
    suffix is "Adjacent" for distance=None (d = 1), else str(d).  PARITY UNPINNED: the definition (include/aliby_hip.h,
    tests/neighbors3d_ref.py) is recalled from CellProfiler 4 and centrosome, neither of which can be run beside this package.
    AngleBetweenNeighbors is atan2(|v1 x v2|, v1 . v2), not CellProfiler's arccos of the normalised dot product: the same angle,
    well-conditioned near 0 and 180 degrees (deliberate).  Not built: "Expand until adjacent", neighbours from a second object set,
    physical-unit (anisotropic) balls, distances above 16."""
    return _neighbors_names("Adjacent" if distance is None else str(neighbors3d_distance(distance)))


GRANULARITY3D_MAX_ELEMENT = 16  # bounds the per-voxel scan of the ball in csrc/feat_granularity3d.hip (about 17 k offsets at 16); not a structural limit
GRANULARITY3D_MAX_LENGTH = 64


def granularity3d_names(granular_spectrum_length: int = 16) -> list[str]:
    """Columns of `FeatureEngine.granularity3d` (csrc/feat_granularity3d.hip): Granularity_1..L, the names of the 2-D `granularity`
    (CellProfiler names a volume's spectrum as it names a plane's).  L is an integer in 1..64; parity with CellProfiler is unpinned."""
    if isinstance(granular_spectrum_length, bool) or not isinstance(granular_spectrum_length, numbers.Integral):
        raise TypeError(f"granular_spectrum_length must be an integer, got {granular_spectrum_length!r}")
    if not 1 <= int(granular_spectrum_length) <= GRANULARITY3D_MAX_LENGTH:
        raise ValueError(f"granularity3d: granular_spectrum_length must lie in 1..{GRANULARITY3D_MAX_LENGTH}, got {granular_spectrum_length!r}")
    return granularity_names(int(granular_spectrum_length))


def projection3d_names() -> list[str]:
    """Columns of `FeatureEngine.projection3d` (csrc/feat_projection3d.hip): how the collapse of a 3-D label result (the maximum over
    z, then a sequential relabel: `segment.model.max_project_and_relabel`) sees each volume object.  With `top` the maximum over z
    of a column (y, x): Projection_Area, the columns that hold a voxel of the object; Projection_VisibleArea, those whose top it
    is; Projection_VisibleFraction, their quotient (NaN without voxels); Projection_Label, the label the object carries in the
    collapsed image — the join key to the rows measured on the collapse — or 0 when it is hidden under other objects everywhere.
    The definition is in include/aliby_hip.h, restated in tests/projection3d_ref.py."""
    return ["Projection_Area", "Projection_VisibleArea", "Projection_VisibleFraction", "Projection_Label"]
