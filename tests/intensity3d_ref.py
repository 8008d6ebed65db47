"""
Exact reference of `FeatureEngine.intensity3d` (aliby_amd/csrc/feat_intensity3d.hip), the rule its results are compared by, and
the inputs of its tests that carry a stated precondition (tests/test_cpu_intensity3d_ref.py checks each precondition without a GPU).

A per-object restatement in Python integers, written from the column definitions:

  * every object gets n, sum v, sum v^2, sum x v, sum y v, sum z v, sum x, sum y, sum z, min and max as `int` (`exact_sum`);
  * a quotient column is `float(Fraction(num, den))`: the float64 nearest to the exact quotient (CPython's int / int is
    correctly rounded);
  * the std is `math.sqrt` of the correctly rounded `Fraction(n * sum v^2 - (sum v)^2, n^2)`: one rounding before the root and
    one in it, so within 1 ulp of the true value or so;
  * conventions of the family: a label of 1..n without voxels has Volume 0 and NaN elsewhere; an object whose pixels are all 0
    has NaN intensity-weighted centres; labels above n are ignored.

tests/test_cpu_intensity3d_ref.py pins this file to oracle/volume_restated.intensity3d (float64 NumPy) and to closed forms.
"""
import math
from fractions import Fraction

import numpy as np

NAMES = ["Volume", "Intensity_IntegratedIntensity", "Intensity_MeanIntensity", "Intensity_StdIntensity", "Intensity_MinIntensity",
         "Intensity_MaxIntensity", "Location_CenterMassIntensity_X", "Location_CenterMassIntensity_Y", "Location_CenterMassIntensity_Z",
         "Location_Center_X", "Location_Center_Y", "Location_Center_Z"]
COL = {k: i for i, k in enumerate(NAMES)}
SUMS = ("n", "s", "s2", "xv", "yv", "zv", "sx", "sy", "sz", "min", "max")
EXACT = [COL["Volume"], COL["Intensity_IntegratedIntensity"], COL["Intensity_MinIntensity"], COL["Intensity_MaxIntensity"]]
STD = COL["Intensity_StdIntensity"]
# quotient column -> (numerator, denominator) among SUMS
QUOTIENTS = {"Intensity_MeanIntensity": ("s", "n"), "Location_CenterMassIntensity_X": ("xv", "s"), "Location_CenterMassIntensity_Y": ("yv", "s"),
             "Location_CenterMassIntensity_Z": ("zv", "s"), "Location_Center_X": ("sx", "n"), "Location_Center_Y": ("sy", "n"),
             "Location_Center_Z": ("sz", "n")}
TWO53 = 1 << 53
RTOL = 1e-10  # the family's bound (tests/test_gpu_volume.py), for the std and for quotients with an operand of 2^53 or more


def exact_sum(a) -> int:
    """Exact sum of a non-negative integer array with entries below 2^40, as a Python int: NumPy adds chunks of 2^20 entries in
    uint64 (below 2^60: no wrap), Python adds the chunk sums."""
    a = np.ascontiguousarray(a, dtype=np.uint64).ravel()
    assert a.size == 0 or int(a.max()) < (1 << 40)
    return sum(int(a[i:i + (1 << 20)].sum(dtype=np.uint64)) for i in range(0, a.size, 1 << 20))


def object_sums(volume, pixels, n=None):
    """volume int [Z,Y,X], pixels uint16 [Z,Y,X] -> one dict of Python ints (keys SUMS) per label 1..n; an absent label has n = 0
    and min / max None.  n defaults to the largest label; labels above n are ignored."""
    volume, pixels = np.asarray(volume), np.asarray(pixels)
    assert volume.ndim == 3 and pixels.shape == volume.shape and pixels.dtype == np.uint16
    n = int(volume.max(initial=0)) if n is None else int(n)
    zz, yy, xx = np.nonzero(volume)
    lab = volume[zz, yy, xx]
    val = pixels[zz, yy, xx].astype(np.uint64)
    out = []
    for k in range(1, n + 1):
        m = lab == k
        v, z, y, x = val[m], zz[m].astype(np.uint64), yy[m].astype(np.uint64), xx[m].astype(np.uint64)
        if v.size == 0:
            out.append(dict.fromkeys(SUMS, 0) | {"min": None, "max": None})
            continue
        out.append({"n": int(v.size), "s": exact_sum(v), "s2": exact_sum(v * v), "xv": exact_sum(x * v), "yv": exact_sum(y * v),
                    "zv": exact_sum(z * v), "sx": exact_sum(x), "sy": exact_sum(y), "sz": exact_sum(z), "min": int(v.min()), "max": int(v.max())})
    return out


def variance_numerator(s) -> int:
    """n * sum v^2 - (sum v)^2 (n^2 times the population variance), exact."""
    return s["n"] * s["s2"] - s["s"] * s["s"]


def row(s) -> np.ndarray:
    """The 12 columns of one object from its integer sums."""
    out = np.full(len(NAMES), np.nan)
    out[COL["Volume"]] = 0.0
    if s["n"] == 0:
        return out
    out[COL["Volume"]] = float(s["n"])
    out[COL["Intensity_IntegratedIntensity"]] = float(s["s"])  # (below 2^53 for any stack the entry accepts: 2^32 voxels of 2^16)
    out[STD] = math.sqrt(float(Fraction(variance_numerator(s), s["n"] * s["n"])))
    out[COL["Intensity_MinIntensity"]], out[COL["Intensity_MaxIntensity"]] = float(s["min"]), float(s["max"])
    for name, (num, den) in QUOTIENTS.items():
        if s[den]:
            out[COL[name]] = float(Fraction(s[num], s[den]))
    return out


def intensity3d(volume, pixels, n=None):
    """-> (float64 [n, 12] in NAMES order, row = label - 1; the list of integer sums the rows were made from)."""
    sums = object_sums(volume, pixels, n)
    return (np.stack([row(s) for s in sums]) if sums else np.zeros((0, len(NAMES)))), sums


def intensity3d_batch(vols, pixels, channel, counts):
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] -> (float64 [sum counts, 12], sums of all rows)."""
    rows, sums = [np.zeros((0, len(NAMES)))], []
    for f, (v, c) in enumerate(zip(vols, counts)):
        r, s = intensity3d(v, pixels[f][channel], c)
        rows.append(r)
        sums += s
    return np.concatenate(rows), sums


def columns_above_2_53(sums) -> set:
    """The quotient columns that have, in some row, an operand of 2^53 or more (not exactly a float64)."""
    return {name for name, (num, den) in QUOTIENTS.items() for s in sums if s[num] >= TWO53 or s[den] >= TWO53}


def check(got, want, sums, tag, above_2_53=()):
    """The comparison rule of the family.  Volume, IntegratedIntensity, Min and Max: the same bits.  A quotient column: the same
    bits in every row whose two operands are below 2^53 (the kernel divides two exactly converted doubles, and IEEE division is
    correctly rounded), else within RTOL.  `above_2_53` is the input's stated precondition: exactly these columns may hold such an
    operand.  Std: within RTOL, and exactly 0.0 where the numerator is 0.  Prints the worst error of each float column."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape == (len(sums), len(NAMES)), (tag, got.shape, want.shape, len(sums))
    assert columns_above_2_53(sums) == set(above_2_53), (tag, columns_above_2_53(sums))
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    gb, wb = got.view(np.uint64), want.view(np.uint64)
    assert np.array_equal(got[:, EXACT], want[:, EXACT], equal_nan=True), (tag, "integer columns", np.argwhere(gb[:, EXACT] != wb[:, EXACT])[:4])
    worst = {}
    for name, (num, den) in QUOTIENTS.items():
        k = COL[name]
        small = np.asarray([s[num] < TWO53 and s[den] < TWO53 for s in sums], bool)
        bad = small & (gb[:, k] != wb[:, k]) & ~np.isnan(want[:, k])  # (NaN sits where NaN is wanted: asserted above)
        assert not bad.any(), (tag, name, "not the correctly rounded quotient", [(int(r), got[r, k], want[r, k]) for r in np.flatnonzero(bad)[:4]])
        worst[name] = _worst(got[:, k], want[:, k])
        assert worst[name] <= RTOL, (tag, name, worst[name])
    zero = np.asarray([s["n"] > 0 and variance_numerator(s) == 0 for s in sums], bool)
    assert (gb[zero, STD] == 0).all(), (tag, "std of a constant object", got[zero, STD][:4])  # the bits of +0.0
    worst[NAMES[STD]] = _worst(got[:, STD], want[:, STD])
    assert worst[NAMES[STD]] <= RTOL, (tag, "std", worst[NAMES[STD]])
    print(f"intensity3d {tag}: {len(sums)} objects, worst relative error " + ", ".join(f"{k.split('_', 1)[1]} {v:.1e}" for k, v in worst.items()))
    return worst


def _worst(g, w):
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(g - w) / np.abs(w)
    rel = np.where(g == w, 0.0, rel)  # (0 against 0)
    rel = rel[~np.isnan(w)]
    return float(rel.max()) if rel.size else 0.0


# ------------------------------------------------------------------------------------------------ inputs with a precondition
# (seed, shape) of tests/sizeshape3d_ref.random_labels: X = 1, 15, 16, 17, 31 and 130, below, at and above the kernel's 16-voxel
# segment, with and without a tail; Z = 1 among them
IRREGULAR_SHAPES = [(0, (6, 40, 1)), (1, (5, 33, 15)), (2, (4, 30, 16)), (3, (7, 29, 17)), (4, (1, 61, 31)), (5, (9, 17, 130))]


def full_range_pixels(seed, vol, n_channels=3):
    """uint16 [C,Z,Y,X] over the whole range; in every channel the first labelled voxel holds 0 and the last 65535."""
    rng = np.random.default_rng(3000 + seed)
    px = rng.integers(0, 65536, size=(n_channels, *vol.shape), dtype=np.uint16)
    idx = np.argwhere(vol > 0)
    if len(idx):
        px[(slice(None), *idx[0])] = 0
        px[(slice(None), *idx[-1])] = 65535
    return px


BOX = (slice(0, 8), slice(1, 129), slice(3, 260))  # 8 x 128 x 257 = 263 168 voxels, a little above 2^18; 257: runs of every length 1..16


def bright_box(kind):
    """-> (labels uint16 [8,130,263], pixels uint16 [1,8,130,263]): label 1 = BOX, with, by `kind`,
    "one_zero": 65535 everywhere and a single 0 (n * sum v^2 above 2^64; std = 65535 sqrt(n - 1) / n);
    "alternating": 65534 / 65535 by the parity of the voxel's rank in the box (an even count: std exactly 0.5);
    "constant": 65535 everywhere (std exactly 0);
    "half_dark": 0 / 65535 by that parity (the numerator itself, n^2 65535^2 / 4, is above 2^64; std exactly 32767.5);
    "nearly_constant": random values in 65531..65535 (sum v^2 / n - mean^2 in float64 keeps six digits of this variance)."""
    vol = np.zeros((8, 130, 263), np.uint16)
    vol[BOX] = 1
    px = np.full(vol.shape, 7, np.uint16)
    n = int(vol.sum())
    if kind == "one_zero":
        vals = np.full(n, 65535, np.uint16)
        vals[n // 3] = 0
    elif kind == "alternating":
        vals = (65534 + (np.arange(n) & 1)).astype(np.uint16)
    elif kind == "half_dark":
        vals = (65535 * (np.arange(n) & 1)).astype(np.uint16)
    elif kind == "nearly_constant":
        vals = np.random.default_rng(53).integers(65531, 65536, size=n, dtype=np.uint16)
    else:
        assert kind == "constant"
        vals = np.full(n, 65535, np.uint16)
    px[vol == 1] = vals
    return vol, px[None]


def widest_stack():
    """-> (labels uint16 [2,64,65536], pixels uint16 [1,2,64,65536]): X = 65536, the widest the entry accepts.  Label 1 is bright
    (60000..65535) and fills x >= 32768 of 55 rows of both planes, so that sum x v is above 2^53; label 2 is a small object at the
    last voxels of the row, x = 65530..65535."""
    rng = np.random.default_rng(65536)
    vol = np.zeros((2, 64, 65536), np.uint16)
    vol[:, 5:60, 32768:] = 1
    vol[1, 61:63, 65530:] = 2
    px = rng.integers(60000, 65536, size=vol.shape, dtype=np.uint16)
    return vol, px[None]


def run_structure():
    """-> (labels uint16 [3,12,100], 5, pixels uint16 [1,3,12,100]): labels 1 and 2 interleaved voxel by voxel along x (a flush per
    voxel); label 3 in runs of 16 from x = 8 (every run straddles a 16-voxel boundary); label 4 one voxel; label 5 over
    all-zero pixels."""
    rng = np.random.default_rng(16)
    vol = np.zeros((3, 12, 100), np.uint16)
    vol[0, :6, :] = 1 + (np.arange(100) & 1)
    for start in range(8, 88, 32):
        vol[1, 2:9, start:start + 16] = 3
    vol[2, 3, 47] = 4
    vol[2, 6:11, 60:99] = 5
    px = rng.integers(0, 65536, size=vol.shape, dtype=np.uint16)
    px[vol == 5] = 0
    return vol, 5, px[None]
