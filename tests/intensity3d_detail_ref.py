"""
Reference of `FeatureEngine.intensity3d_detail` (aliby_amd/csrc/feat_intensity3d_detail.hip), the rule its results are compared by,
and the inputs of its tests.

An independent restatement written from the column definitions (include/aliby_hip.h), object by object over the object's voxel list
in raster order (z, y, x); it does not call the oracle (tests/test_cpu_intensity3d_detail_ref.py pins it to the oracle's
get_intensity on one-plane stacks, to find_boundaries_inner on 3-D labels and to hand values):

  * pixels become exact Python integers: a uint16 is one, a float32 is (integer) * 2^k with one k for the whole array
    (`exact_ints`), so every sum below is an exact `int` whatever the pixel type;
  * a sum or quotient column is `float(Fraction)`, the float64 nearest to the exact value; the edge std is `math.sqrt` of the
    correctly rounded exact variance (n sum v^2 - (sum v)^2) / n^2; MassDisplacement is `math.sqrt` of the correctly rounded
    exact rational dx^2 + dy^2 + dz^2;
  * an order statistic is v[i] (1 - f) + v[i + 1] f in Python floats (float64), q = n p, i = floor(q), f = q - i, or v[i] when
    i = n - 1; the MAD applies it to the sorted float64 |v - median|;
  * an edge voxel has, among its six face neighbours inside the volume, one of another value (`edge_mask`: three shifted
    comparisons, no morphology);
  * the maximum's position is the last voxel of the list that holds the maximum;
  * conventions: a label of 1..n without voxels is a row of NaN; an object without an edge voxel has 0 in the five edge columns;
    MassDisplacement is NaN when the integrated intensity is 0; labels above n are not measured but are "another value".
"""
import math
from fractions import Fraction

import numpy as np

from aliby_amd.extraction.features import INTENSITY_EDGE

TAIL = ["Intensity_MassDisplacement", "Intensity_LowerQuartileIntensity", "Intensity_MedianIntensity", "Intensity_MADIntensity",
        "Intensity_UpperQuartileIntensity", "Location_MaxIntensity_X", "Location_MaxIntensity_Y", "Location_MaxIntensity_Z"]


def names(edge=True):
    return (list(INTENSITY_EDGE) if edge else []) + TAIL


def cols(edge=True):
    return {k: i for i, k in enumerate(names(edge))}


# the columns compared bit for bit with either pixel type, and the further ones with uint16 pixels
BITWISE = ["Intensity_MinIntensityEdge", "Intensity_MaxIntensityEdge", "Intensity_LowerQuartileIntensity", "Intensity_MedianIntensity",
           "Intensity_MADIntensity", "Intensity_UpperQuartileIntensity", "Location_MaxIntensity_X", "Location_MaxIntensity_Y",
           "Location_MaxIntensity_Z"]
BITWISE_U16 = ["Intensity_IntegratedIntensityEdge", "Intensity_MeanIntensityEdge"]
STD_RTOL_U16 = 1e-10  # the rule tests/test_gpu_intensity3d.py holds StdIntensity to
MD_ATOL_U16 = 1e-10   # voxels: each centre is one rounding of a coordinate below 2^16 (2^-37 per component)
EDGE_RTOL_F32 = 1e-9  # float64 tree sums of n <= 2^20 non-negative terms: n 2^-53
MD_ATOL_F32 = 1e-9


def exact_ints(pixels):
    """pixels uint16 or float32 -> (object array of Python ints m, k) with pixel = m * 2^k exactly."""
    p = np.asarray(pixels)
    if p.dtype == np.uint16:
        return p.astype(object), 0
    assert p.dtype == np.float32 and np.isfinite(p).all()
    mant, ex = np.frexp(p.astype(np.float64))          # p = mant * 2^ex, |mant| in [0.5, 1) or 0
    m24 = np.rint(mant * (1 << 24)).astype(np.int64)   # exact: a float32 has 24 significant bits
    ex = np.where(m24 == 0, 0, ex.astype(np.int64) - 24)
    k = int(ex[m24 != 0].min()) if (m24 != 0).any() else 0
    shift = np.where(m24 == 0, 0, ex - k)
    out = np.asarray([int(m) << int(s) for m, s in zip(m24.ravel(), shift.ravel())], dtype=object).reshape(p.shape)
    return out, k


def edge_mask(volume):
    """bool [Z,Y,X]: labelled voxels with a face neighbour inside the volume of another value."""
    vol = np.asarray(volume)
    e = np.zeros(vol.shape, bool)
    for ax in range(vol.ndim):
        lo = [slice(None)] * vol.ndim
        hi = [slice(None)] * vol.ndim
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        d = vol[tuple(lo)] != vol[tuple(hi)]
        e[tuple(lo)] |= d
        e[tuple(hi)] |= d
    return e & (vol != 0)


def order_statistic(sorted_vals, p):
    n = len(sorted_vals)
    q = n * p
    i = int(math.floor(q))
    f = q - i
    if i < n - 1:
        return float(sorted_vals[i]) * (1.0 - f) + float(sorted_vals[i + 1]) * f
    return float(sorted_vals[i])


def _scaled(num, den, k):
    """float64 nearest to (num / den) * 2^k."""
    return float(Fraction(num, den) * Fraction(2) ** k)


def object_row(z, y, x, v, m, k, e, edge=True):
    """One object: coordinates and values of its voxels in raster order (v float64, m the exact ints, pixel = m 2^k), e = edge flags."""
    c = cols(edge)
    out = np.full(len(c), np.nan)
    n = len(v)
    if edge:
        ne = int(e.sum())
        if ne == 0:
            out[:5] = 0.0
        else:
            me = m[e]
            s, s2 = int(me.sum()), int((me * me).sum())
            out[c["Intensity_IntegratedIntensityEdge"]] = _scaled(s, 1, k)
            out[c["Intensity_MeanIntensityEdge"]] = _scaled(s, ne, k)
            out[c["Intensity_StdIntensityEdge"]] = math.sqrt(_scaled(ne * s2 - s * s, ne * ne, 2 * k))
            out[c["Intensity_MinIntensityEdge"]] = float(v[e].min())
            out[c["Intensity_MaxIntensityEdge"]] = float(v[e].max())
    s = int(m.sum())
    if s != 0:
        d2 = Fraction(0)
        for coord in (x, y, z):
            co = coord.astype(object)
            d = Fraction(int(co.sum()), n) - Fraction(int((co * m).sum()), s)
            d2 += d * d
        out[c["Intensity_MassDisplacement"]] = math.sqrt(float(d2))
    sv = np.sort(v)
    med = order_statistic(sv, 0.5)
    out[c["Intensity_LowerQuartileIntensity"]] = order_statistic(sv, 0.25)
    out[c["Intensity_MedianIntensity"]] = med
    out[c["Intensity_UpperQuartileIntensity"]] = order_statistic(sv, 0.75)
    out[c["Intensity_MADIntensity"]] = order_statistic(np.sort(np.abs(v - med)), 0.5)
    last = n - 1 - int(np.argmax(v[::-1]))
    out[c["Location_MaxIntensity_X"]], out[c["Location_MaxIntensity_Y"]], out[c["Location_MaxIntensity_Z"]] = float(x[last]), float(y[last]), float(z[last])
    return out


def detail(volume, pixels, n=None, edge=True):
    """volume int [Z,Y,X], pixels uint16 or float32 [Z,Y,X] -> float64 [n, 13 or 8], row = label - 1.  n defaults to the largest label."""
    volume, pixels = np.asarray(volume), np.asarray(pixels)
    assert volume.ndim == 3 and pixels.shape == volume.shape and pixels.dtype in (np.uint16, np.float32)
    n = int(volume.max(initial=0)) if n is None else int(n)
    out = np.full((n, len(names(edge))), np.nan)
    zz, yy, xx = np.nonzero(volume)  # raster order
    lab = volume[zz, yy, xx].astype(np.int64)
    order = np.argsort(lab, kind="stable")  # by label, raster order inside a label
    zz, yy, xx, lab = zz[order], yy[order], xx[order], lab[order]
    val = pixels[zz, yy, xx]
    ints, k = exact_ints(val)
    flags = edge_mask(volume)[zz, yy, xx]
    v64 = val.astype(np.float64)
    starts = np.searchsorted(lab, np.arange(1, n + 2))
    for r in range(n):
        a, b = int(starts[r]), int(starts[r + 1])
        if b > a:
            out[r] = object_row(zz[a:b], yy[a:b], xx[a:b], v64[a:b], ints[a:b], k, flags[a:b], edge)
    return out


def detail_batch(vols, pixels, channel, counts, edge=True):
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] -> float64 [sum counts, 13 or 8]."""
    rows = [np.zeros((0, len(names(edge))))]
    for f, (v, c) in enumerate(zip(vols, counts)):
        rows.append(detail(v, pixels[f][channel], c, edge))
    return np.concatenate(rows)


def one_voxel_rows(volume, pixels):
    """The closed form for a stack [Z,Y,X] in which every label 1..n is a single voxel with a face neighbour of another value, pixels
    uint16: the voxel is its own edge, quartiles and maximum; the deviations and the displacement are 0 (NaN displacement on a 0)."""
    volume = np.asarray(volume)
    n = int(volume.max())
    zz, yy, xx = np.nonzero(volume)
    assert len(zz) == n and edge_mask(volume)[zz, yy, xx].all()
    order = np.argsort(volume[zz, yy, xx], kind="stable")
    zz, yy, xx = zz[order], yy[order], xx[order]
    v = np.asarray(pixels)[zz, yy, xx].astype(np.float64)
    zero = np.zeros(n)
    return np.stack([v, v, zero, v, v, np.where(v == 0, np.nan, 0.0), v, v, zero, v, xx.astype(np.float64), yy.astype(np.float64),
                     zz.astype(np.float64)], axis=1)


# ------------------------------------------------------------------------------------------------ the comparison rule
def _rel(g, w):
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(g - w) / np.abs(w)
    rel = np.where(g == w, 0.0, rel)  # (0 against 0)
    rel = rel[~np.isnan(w)]
    return float(rel.max()) if rel.size else 0.0


def check(got, want, dtype, tag, edge=True, signed=False):
    """The comparison rule.  NaN exactly where the reference has NaN.  The same bits: the four order statistics, the edge minimum
    and maximum and the maximum's position; with uint16 pixels also the edge sum and mean (one division of exact integers below
    2^53).  uint16: edge std within 1e-10 relative, MassDisplacement within 1e-10 voxels of the exact-rational value.  float32:
    edge sum, mean and std within 1e-9 relative and MassDisplacement within 1e-9 voxels, on non-negative pixels only
    (`signed=True`: those four columns are not compared).  Prints every figure before it asserts."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    c = cols(edge)
    u16 = np.dtype(dtype) == np.uint16
    assert got.shape == want.shape and got.shape[1] == len(c), (tag, got.shape, want.shape)
    bitwise = [k for k in BITWISE + (BITWISE_U16 if u16 else []) if k in c]
    close = {}
    if not signed:
        close["Intensity_MassDisplacement"] = ("abs", MD_ATOL_U16 if u16 else MD_ATOL_F32)
        if edge:
            close["Intensity_StdIntensityEdge"] = ("rel", STD_RTOL_U16 if u16 else EDGE_RTOL_F32)
            if not u16:
                close["Intensity_IntegratedIntensityEdge"] = close["Intensity_MeanIntensityEdge"] = ("rel", EDGE_RTOL_F32)
    compared = [c[k] for k in bitwise + list(close)]
    nan_g, nan_w = np.isnan(got[:, compared]), np.isnan(want[:, compared])
    figures = {}
    for k, (kind, tol) in close.items():
        g, w = got[:, c[k]], want[:, c[k]]
        if kind == "rel":
            figures[k] = _rel(g, w)
        else:
            d = np.abs(g - w)[~np.isnan(w) & ~np.isnan(g)]
            figures[k] = float(d.max()) if d.size else 0.0
    gb, wb = got.view(np.uint64), want.view(np.uint64)
    wrong = {k: int(((gb[:, c[k]] != wb[:, c[k]]) & ~(np.isnan(got[:, c[k]]) & np.isnan(want[:, c[k]]))).sum()) for k in bitwise}
    print(f"intensity3d_detail {tag}: {want.shape[0]} objects, rows with other bits " + ", ".join(f"{k.split('_', 1)[1]} {v}" for k, v in wrong.items())
          + "; worst error " + ", ".join(f"{k.split('_', 1)[1]} {v:.2e}" for k, v in figures.items()))
    assert np.array_equal(nan_g, nan_w), (tag, "NaN pattern", np.argwhere(nan_g != nan_w)[:4])
    for k in bitwise:
        bad = np.flatnonzero((gb[:, c[k]] != wb[:, c[k]]) & ~np.isnan(want[:, c[k]]))
        assert bad.size == 0, (tag, k, "not the same bits", [(int(r), got[r, c[k]], want[r, c[k]]) for r in bad[:4]])
    for k, (kind, tol) in close.items():
        assert figures[k] <= tol, (tag, k, figures[k], tol)
    return figures


# ------------------------------------------------------------------------------------------------ inputs
def unit_float(pixels_u16):
    return (np.asarray(pixels_u16).astype(np.float32) / np.float32(65535.0)).astype(np.float32)


def as_mode(px, mode):
    """mode "u16": the uint16 pixels; "f32": float32 in [0, 1]; "f32_signed": float32 in [-1, 1] (the bit-exact columns only)."""
    if mode == "u16":
        return px
    f = unit_float(px)
    return f if mode == "f32" else (f * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def tied_pixels(seed, vol):
    """uint16 [Z,Y,X]: a few values only, 0 and 65535 among them (heavy ties inside every object); the objects whose label is a
    multiple of 3 hold one value throughout, label 3 the value 0."""
    rng = np.random.default_rng(5000 + seed)
    px = rng.choice(np.asarray([0, 7, 7, 1000, 1000, 1000, 40000, 65535], np.uint16), size=vol.shape)
    for lab in range(3, int(vol.max()) + 1, 3):
        px[vol == lab] = 0 if lab == 3 else 1000 + lab
    return px


def raster_runs(shape, sizes, gap=1, start=1):
    """labels uint16 `shape`: label j + 1 = sizes[j] consecutive voxels of the flattened stack, `gap` background voxels between two
    objects.  An object longer than a row wraps: its box is wider than the object."""
    flat = np.zeros(int(np.prod(shape)), np.uint16)
    at = start
    for j, s in enumerate(sizes):
        flat[at:at + s] = j + 1
        at += s + gap
    assert at - gap <= flat.size
    return flat.reshape(shape)


def pow2_sizes(kmax=10):
    return [s for k in range(1, kmax + 1) for s in ((1 << k) - 1, 1 << k, (1 << k) + 1)]


def power_of_two_volume():
    """-> (labels [4,64,64], n, pixels uint16): objects of 2^k - 1, 2^k and 2^k + 1 voxels, k = 1..10: each side of every sort padding."""
    sizes = pow2_sizes()
    vol = raster_runs((4, 64, 64), sizes)
    return vol, len(sizes), np.random.default_rng(77).integers(0, 65536, size=vol.shape, dtype=np.uint16)


def budget_volume(lds_voxels):
    """-> (labels [48,64,64], 4, pixels uint16): objects of lds_voxels - 1, lds_voxels and lds_voxels + 1 voxels and a small one: both
    forms of the kernel in one launch."""
    sizes = [lds_voxels - 1, lds_voxels, lds_voxels + 1, 37]
    vol = raster_runs((48, 64, 64), sizes, gap=70)
    return vol, 4, np.random.default_rng(78).integers(0, 65536, size=vol.shape, dtype=np.uint16)


def form_pair(lds_voxels):
    """-> (vols [2][Z,64,64], pixels uint16 [2,1,Z,64,64]): stack 0 holds one object of exactly lds_voxels voxels; stack 1 the same
    object, same pixels, and one more voxel after its last, holding the object's median value.  The values are four plateaus placed so
    that every order statistic, of the values and of the deviations, reads inside one plateau in both stacks: the order statistics
    and the maximum's position are the same numbers on both sides of the budget."""
    n = lds_voxels
    assert n % 4096 == 0
    zdim = n // 4096 + 2
    vol = raster_runs((zdim, 64, 64), [n], start=100)
    plateaus = [(100, n * 4000 // 16384), (5000, n * 4000 // 16384), (6000, n * 4200 // 16384)]
    vals = np.concatenate([np.full(c, v, np.uint16) for v, c in plateaus])
    vals = np.concatenate([vals, np.full(n - len(vals), 9000, np.uint16)])
    np.random.default_rng(79).shuffle(vals)
    px = np.full(vol.shape, 123, np.uint16)
    px[vol == 1] = vals
    vol2, px2 = vol.copy(), px.copy()
    vol2.reshape(-1)[100 + n] = 1
    px2.reshape(-1)[100 + n] = 6000
    return [vol, vol2], np.stack([px, px2])[:, None]


def faces_volume():
    """-> (labels [6,7,8], count 8, pixels uint16): label 1..6 on one face of the stack each (1 also on a corner, 2 along an edge), label 7
    in the middle around an enclosed background voxel, and a voxel of label 9 (above the count of 8) that touches 7 and nothing else;
    label 8 is absent."""
    vol = np.zeros((6, 7, 8), np.uint16)
    vol[0, 0:2, 0:2] = 1       # face z = 0, corner (0, 0, 0)
    vol[5, 0, 3:7] = 2         # face z = Z - 1, along the edge y = 0
    vol[2:4, 0, 6:8] = 3       # faces y = 0 and x = X - 1
    vol[2:4, 6, 0:3] = 4       # faces y = Y - 1 and x = 0
    vol[4:6, 5:7, 6:8] = 5     # the corner (Z - 1, Y - 1, X - 1)
    vol[1:3, 3:5, 0] = 6       # face x = 0
    vol[1:4, 2:5, 3:6] = 7
    vol[2, 3, 4] = 0           # the enclosed background voxel
    vol[4, 3, 4] = 9           # above the count: not measured, but another value next to 7
    px = np.random.default_rng(80).integers(0, 65536, size=vol.shape, dtype=np.uint16)
    return vol, 8, px


def single_voxels(shape=(40, 40, 41), n=65535, seed=81):
    """-> (labels, pixels uint16): n one-voxel objects on the first n voxels of the stack, labels in a shuffled order."""
    flat = np.zeros(int(np.prod(shape)), np.uint16)
    flat[:n] = np.random.default_rng(seed).permutation(n).astype(np.uint16) + 1
    vol = flat.reshape(shape)
    return vol, np.random.default_rng(seed + 1).integers(0, 65536, size=shape, dtype=np.uint16)


def keep_touching(volume, lab):
    """The stack with every voxel of another label erased unless it is a face neighbour of object `lab`."""
    vol = np.asarray(volume)
    near = vol == lab
    grown = near.copy()
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        grown[tuple(lo)] |= near[tuple(hi)]
        grown[tuple(hi)] |= near[tuple(lo)]
    return np.where(grown, vol, 0).astype(vol.dtype)
