"""
TEST INFRASTRUCTURE — an exact per-object reference of the 2-D size/shape kernels (aliby_amd/csrc/feat_shape.hip: k_shape_core,
k_shape_edt, k_shape_hull; aliby_amd/csrc/hull.h), the rule they are compared by, and the shape catalogue of
tests/test_cpu_shape_ref.py and tests/test_gpu_shape.py.  It shares no code and no formulation with aliby_amd or with
oracle/cp_measure_restated.py (tests/test_cpu_shape_ref.py pins it to that oracle and to closed forms):

    Euler number     8-connected components minus holes (4-connected background components of the 1-padded crop that do not
                     touch the pad), by labelling — no bit-quads
    Perimeter        three integer class counts from the 4-neighbour inner border and the 3 x 3 code table published for
                     skimage.measure.perimeter(neighbourhood=4); the value is c1 + c2 sqrt(2) + c3 (1 + sqrt(2)) / 2
    ConvexArea       bounding-box pixel centres inside or on the hull of all 4 Area diamond-offset points, in doubled integer
                     coordinates: a gift-wrapped hull of all the points, exact half-plane tests
    Feret diameters  no hull: max = sqrt of the largest squared distance of two pixels; min = the smallest width over the
                     directions of pixel pairs that have every pixel on one side, from integer cross products
    EDT radii        squared distance to the nearest background cell of the 1-padded crop by brute force over integers; maximum and
                     median are correctly rounded roots (an even count takes the float64 mean of the two middle roots, as
                     numpy.median of the float64 distances does); the mean is math.fsum of the roots over N
    moments          raw: Python integers.  Central: exact rationals about the exact centroid (sum of (n r - Sr)^p (n c - Sc)^q
                     over n^(p+q)).  Everything derived: the published formulas on those values at 60 digits (decimal), rounded
                     to float64 once
    Orientation      skimage's rule in exact arithmetic: I20 == I02 -> -45 deg if I11 > 0 else +45 deg; otherwise
                     0.5 atan2(2 I11, I20 - I02) (the integers n S2 - S1 S1: the ratio is exact; math.atan2 of two exactly
                     represented integers is within an ulp, 1e-14 degrees).  An integer zero has no sign: I11 == 0 with
                     I20 < I02 (a horizontal line) is atan2(0, negative) = +pi, +90 deg

Beside every column that is a sum or difference of terms the reference returns the sum of the terms' magnitudes (`scale`): what
the same formula gives with every term replaced by its absolute value, carried from the pixels' terms through products and sums.
The rule (`check`) measures the error of such a column against that scale; through a final square root sqrt(x) the allowance
d on x becomes min(sqrt(d), d / sqrt(x)), which bounds |sqrt(x +- d) - sqrt(x)| for every x >= 0.
"""
import functools
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
from scipy import ndimage as ndi  # connected-component labelling only

getcontext().prec = 60
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")
SQRT2 = Decimal(2).sqrt()

NAMES = (["Area", "BoundingBoxArea", "BoundingBoxMaximum_X", "BoundingBoxMaximum_Y", "BoundingBoxMinimum_X", "BoundingBoxMinimum_Y",
          "Center_X", "Center_Y", "Compactness", "ConvexArea", "Eccentricity", "EquivalentDiameter", "EulerNumber", "Extent", "FormFactor",
          "MajorAxisLength", "MaxFeretDiameter", "MaximumRadius", "MeanRadius", "MedianRadius", "MinFeretDiameter", "MinorAxisLength",
          "Orientation", "Perimeter", "Solidity"]
         + [f"SpatialMoment_{p}_{q}" for p in range(3) for q in range(4)]
         + [f"CentralMoment_{p}_{q}" for p in range(3) for q in range(4)]
         + [f"NormalizedMoment_{p}_{q}" for p in range(4) for q in range(4)]
         + [f"HuMoment_{k}" for k in range(7)]
         + [f"InertiaTensor_{i}_{j}" for i in range(2) for j in range(2)]
         + [f"InertiaTensorEigenvalues_{k}" for k in range(2)])
N_SS = 78
ALL_NAMES = NAMES + ["MinFeret", "MaxFeret"]  # the feret family's two columns
COL = {n: i for i, n in enumerate(ALL_NAMES)}
assert len(NAMES) == N_SS and len(COL) == 80

# ---- the rule --------------------------------------------------------------------------------------------------------------
# Bit for bit: integers below 2^53 and correctly rounded square roots of such integers.
BITWISE = tuple(["Area", "BoundingBoxArea", "BoundingBoxMaximum_X", "BoundingBoxMaximum_Y", "BoundingBoxMinimum_X", "BoundingBoxMinimum_Y",
                 "EulerNumber", "ConvexArea", "MaximumRadius", "MedianRadius"] + [f"SpatialMoment_{p}_{q}" for p in range(3) for q in range(4)])
# Sums of N float64 terms in an unspecified order: 4 N 2^-53 of the sum of the terms' magnitudes (tests/cell_ref.py).
SUMMED = tuple(["MeanRadius"] + [f"CentralMoment_{p}_{q}" for p in range(3) for q in range(4)])
ORIENTATION_ATOL_DEG = 1e-12
DERIVED_RTOL = 1e-14
U = 2.0 ** -53
FERET = ("MinFeretDiameter", "MaxFeretDiameter", "MinFeret", "MaxFeret")  # bit for bit where the reference is 0


class V:
    """A value at 60 digits with the sum of its terms' magnitudes."""
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = _dec(v)
        self.s = abs(self.v) if s is None else _dec(s)

    def __add__(self, o):
        o = _v(o)
        return V(self.v + o.v, self.s + o.s)

    def __sub__(self, o):
        o = _v(o)
        return V(self.v - o.v, self.s + o.s)

    def __mul__(self, o):
        o = _v(o)
        return V(self.v * o.v, self.s * o.s)

    __rmul__ = __mul__

    def over(self, d):
        """divided by a positive number that is no difference of terms"""
        d = _dec(d)
        assert d > 0
        return V(self.v / d, self.s / d)


def _dec(x):
    if isinstance(x, Decimal):
        return x
    if isinstance(x, Fraction):
        return Decimal(x.numerator) / Decimal(x.denominator)
    return Decimal(x)


def _v(x):
    return x if isinstance(x, V) else V(x)


def sqrt_scale(x, x_scale, eps=DERIVED_RTOL):
    """The scale s with eps * s = the bound of |sqrt(x +- d) - sqrt(x)| for d = eps * x_scale."""
    d = _dec(eps) * _dec(x_scale)
    bound = d.sqrt()
    if x > 0:
        bound = min(bound, d / _dec(x).sqrt())
    return bound / _dec(eps)


# ---- integer geometry --------------------------------------------------------------------------------------------------------
def _min_d2(py, px, qy, qx):
    out = np.empty(len(py), np.int64)
    qy, qx = qy.astype(np.int64)[None, :], qx.astype(np.int64)[None, :]
    step = max(1, (1 << 22) // max(qy.shape[1], 1))
    for s in range(0, len(py), step):
        dy = py[s:s + step].astype(np.int64)[:, None] - qy
        dx = px[s:s + step].astype(np.int64)[:, None] - qx
        out[s:s + step] = (dy * dy + dx * dx).min(axis=1)
    return out


def euler_number(img):
    _, n_obj = ndi.label(img, structure=np.ones((3, 3), int))
    _, n_bg = ndi.label(~np.pad(img, 1), structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    return n_obj - (n_bg - 1)  # the pad ring is connected: exactly one background component touches it


def perimeter_counts(img):
    """-> (c1, c2, c3): border pixels of weight 1, sqrt(2) and (1 + sqrt(2)) / 2."""
    m = np.pad(img, 2).astype(np.int64)
    core = m[1:-1, 1:-1]
    inner = core & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]  # the 4-neighbour erosion
    b = np.pad(core - inner, 1)
    code = (b[1:-1, 1:-1] + 2 * (b[:-2, 1:-1] + b[2:, 1:-1] + b[1:-1, :-2] + b[1:-1, 2:])
            + 10 * (b[:-2, :-2] + b[:-2, 2:] + b[2:, :-2] + b[2:, 2:]))
    code = code[(core - inner) == 1]
    return (int(np.isin(code, (5, 7, 15, 17, 25, 27)).sum()), int(np.isin(code, (21, 33)).sum()), int(np.isin(code, (13, 23)).sum()))


def _gift_wrap(pts):
    """Hull vertices in order (turning one way), collinear points dropped; pts: a list of distinct integer pairs, not all collinear."""
    start = min(pts)
    hull, p = [], start
    while True:
        hull.append(p)
        q = None
        for k in pts:
            if k == p:
                continue
            if q is None:
                q = k
                continue
            cr = (q[0] - p[0]) * (k[1] - p[1]) - (q[1] - p[1]) * (k[0] - p[0])
            if cr < 0 or (cr == 0 and (k[0] - p[0]) ** 2 + (k[1] - p[1]) ** 2 > (q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2):
                q = k
        p = q
        if p == start:
            return hull
        assert len(hull) <= len(pts)


def convex_area(img):
    rr, cc = np.nonzero(img)
    pts = set()
    for r, c in zip(rr.tolist(), cc.tolist()):
        pts.update(((2 * r - 1, 2 * c), (2 * r + 1, 2 * c), (2 * r, 2 * c - 1), (2 * r, 2 * c + 1)))
    hull = _gift_wrap(sorted(pts))
    R, Cc = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    R, Cc = 2 * R.astype(np.int64), 2 * Cc.astype(np.int64)
    inside = np.ones(img.shape, bool)
    for i, a in enumerate(hull):
        b = hull[(i + 1) % len(hull)]
        # _gift_wrap keeps every point on the side where this cross product is >= 0
        inside &= (b[0] - a[0]) * (Cc - a[1]) - (b[1] - a[1]) * (R - a[0]) >= 0
    assert inside[img].all()
    return int(inside.sum())


def feret(img):
    """-> (min squared as a Fraction, max squared as an int), no hull."""
    rr, cc = np.nonzero(img)
    r, c = rr.astype(np.int64), cc.astype(np.int64)
    n = len(r)
    if n == 1:
        return Fraction(0), 0
    d2max = max(int(((r - r[i]) ** 2 + (c - c[i]) ** 2).max()) for i in range(n))
    if not ((r[1] - r[0]) * (c - c[0]) - (c[1] - c[0]) * (r - r[0])).any():
        return Fraction(0), d2max  # every pixel on the line through the first two: no width (and n^3 cross products spared)
    best_max, best_min = d2max, None
    for i in range(n):
        er, ec = r - r[i], c - c[i]                    # directions i -> j
        cross = er[:, None] * ec[None, :] - ec[:, None] * er[None, :]     # [j, k]: (pj - pi) x (pk - pi)
        lo, hi = cross.min(axis=1), cross.max(axis=1)
        for j in np.nonzero(((lo >= 0) | (hi <= 0)) & ((er != 0) | (ec != 0)))[0].tolist():
            w2 = Fraction(int(max(hi[j], -lo[j])) ** 2, int(er[j] * er[j] + ec[j] * ec[j]))
            if best_min is None or w2 < best_min:
                best_min = w2
    return best_min, best_max


def edt_d2(img):
    m = np.pad(img, 1)
    oy, ox = np.nonzero(m)
    by, bx = np.nonzero(~m)
    return np.sort(_min_d2(oy, ox, by, bx))


# ---- one object ---------------------------------------------------------------------------------------------------------------
def _hu(nu):
    """skimage.measure.moments_hu as published, on values that carry their scale."""
    t0, t1 = nu[3][0] + nu[1][2], nu[2][1] + nu[0][3]
    q0, q1 = t0 * t0, t1 * t1
    n4 = 4 * nu[1][1]
    s, d = nu[2][0] + nu[0][2], nu[2][0] - nu[0][2]
    hu = [None] * 7
    hu[0] = s
    hu[1] = d * d + n4 * nu[1][1]
    hu[3] = q0 + q1
    hu[5] = d * (q0 - q1) + n4 * t0 * t1
    t0 = t0 * (q0 - 3 * q1)
    t1 = t1 * (3 * q0 - q1)
    q0 = nu[3][0] - 3 * nu[1][2]
    q1 = 3 * nu[2][1] - nu[0][3]
    hu[2] = q0 * q0 + q1 * q1
    hu[4] = q0 * t0 + q1 * t1
    hu[6] = q1 * t0 - q0 * t1
    return hu


def measure(img, y0, x0):
    """One object from its bounding-box crop (bool [h, w]) and the crop's corner -> dict(values [80], scale [80], ...)."""
    h, w = img.shape
    rr, cc = np.nonzero(img)
    rs, cs = rr.tolist(), cc.tolist()
    n = len(rs)
    val = {k: None for k in ALL_NAMES}
    scale = {}

    def put(name, x):
        if isinstance(x, V):
            val[name], scale[name] = x.v, x.s
        else:
            val[name] = x

    put("Area", n)
    put("BoundingBoxArea", h * w)
    put("BoundingBoxMaximum_X", x0 + w)
    put("BoundingBoxMaximum_Y", y0 + h)
    put("BoundingBoxMinimum_X", x0)
    put("BoundingBoxMinimum_Y", y0)
    put("EulerNumber", euler_number(img))
    counts = perimeter_counts(img)
    per = counts[0] + counts[1] * SQRT2 + counts[2] * (1 + SQRT2) / 2
    put("Perimeter", per)
    fpa = 4 * PI * n
    put("Compactness", per * per / fpa)  # (4 pi Area >= 4 pi > 1: the published max(.., 1) never acts)
    put("FormFactor", fpa / (per * per) if per else math.inf)
    put("EquivalentDiameter", (4 * Decimal(n) / PI).sqrt())
    put("Extent", Fraction(n, h * w))
    cvx = convex_area(img)
    put("ConvexArea", cvx)
    put("Solidity", Fraction(n, cvx))
    fmin2, fmax2 = feret(img)
    for a, b in (("MinFeretDiameter", "MaxFeretDiameter"), ("MinFeret", "MaxFeret")):
        put(a, _dec(fmin2).sqrt())
        put(b, math.sqrt(fmax2))
    d2 = edt_d2(img).tolist()
    roots = [math.sqrt(v) for v in d2]
    put("MaximumRadius", roots[-1])
    put("MedianRadius", roots[n // 2] if n & 1 else 0.5 * (roots[n // 2 - 1] + roots[n // 2]))
    put("MeanRadius", math.fsum(roots) / n)

    raw = [[sum(r ** p * c ** q for r, c in zip(rs, cs)) for q in range(4)] for p in range(4)]
    for p in range(3):
        for q in range(4):
            put(f"SpatialMoment_{p}_{q}", raw[p][q])
    Sr, Sc = raw[1][0], raw[0][1]
    put("Center_X", x0 + Fraction(Sc, n))
    put("Center_Y", y0 + Fraction(Sr, n))
    us, vs = [n * r - Sr for r in rs], [n * c - Sc for c in cs]
    mu = [[V(Fraction(sum(u ** p * v ** q for u, v in zip(us, vs)), n ** (p + q)),
             Fraction(sum(abs(u) ** p * abs(v) ** q for u, v in zip(us, vs)), n ** (p + q))) for q in range(4)] for p in range(4)]
    for p in range(3):
        for q in range(4):
            put(f"CentralMoment_{p}_{q}", mu[p][q])
    nu = [[None] * 4 for _ in range(4)]
    for p in range(4):
        for q in range(4):
            if p + q < 2:
                put(f"NormalizedMoment_{p}_{q}", math.nan)
                continue
            k = p + q + 2  # mu00 ^ (k / 2)
            nu[p][q] = mu[p][q].over(Decimal(n) ** (k // 2) * (Decimal(n).sqrt() if k & 1 else 1))
            put(f"NormalizedMoment_{p}_{q}", nu[p][q])
    for k, x in enumerate(_hu(nu)):
        put(f"HuMoment_{k}", x)

    # inertia tensor [[mu02, -mu11], [-mu11, mu20]] / mu00 from the integers I = n S2 - S1 S1 (mu = I / n)
    I20, I02, I11 = n * raw[2][0] - Sr * Sr, n * raw[0][2] - Sc * Sc, n * raw[1][1] - Sr * Sc
    assert mu[2][0].v == _dec(Fraction(I20, n)) and mu[1][1].v == _dec(Fraction(I11, n))
    nn = n * n
    put("InertiaTensor_0_0", V(Fraction(I02, nn)))
    put("InertiaTensor_1_1", V(Fraction(I20, nn)))
    for k in ("InertiaTensor_0_1", "InertiaTensor_1_0"):
        put(k, V(Fraction(-I11, nn), mu[1][1].s / n))
    hs = Decimal(I20 + I02) / (2 * nn)
    rad = Decimal((I20 - I02) ** 2 + 4 * I11 ** 2).sqrt() / (2 * nn)
    l1, l2 = V(hs + rad), V(max(hs - rad, Decimal(0)), hs + rad)
    if (I20 - I02) ** 2 + 4 * I11 ** 2 == (I20 + I02) ** 2:  # a line: the smaller eigenvalue is exactly 0
        l2 = V(0, hs + rad)
    put("InertiaTensorEigenvalues_0", l1)
    put("InertiaTensorEigenvalues_1", l2)
    put("MajorAxisLength", V(4 * l1.v.sqrt(), 4 * sqrt_scale(l1.v, l1.s)))
    put("MinorAxisLength", V(4 * l2.v.sqrt(), 4 * sqrt_scale(l2.v, l2.s)))
    if l1.v == 0:
        put("Eccentricity", 0)
    else:
        x = V(1) - l2.over(l1.v)
        put("Eccentricity", V(x.v.sqrt(), sqrt_scale(x.v, x.s)))
    if I20 == I02:
        branch = "iso-45" if I11 > 0 else "iso+45"
        put("Orientation", -45 if I11 > 0 else 45)
    else:
        branch = "atan2"
        put("Orientation", Decimal(math.atan2(2 * I11, I20 - I02)) * 90 / PI)

    out_v, out_s = np.empty(80), np.full(80, np.nan)
    for k, name in enumerate(ALL_NAMES):
        x = val[name]
        out_v[k] = float(x)
        if name in scale:
            out_s[k] = float(scale[name])
    return dict(values=out_v, scale=out_s, branch=branch, perimeter_counts=counts, raw=raw, iso=(I20, I02, I11), area=n, d2=d2,
                box=(h, w))


def reference(labels, n=None):
    """One label image [Y, X] -> dict(values [n, 80], scale [n, 80], objects: per label the dict of `measure` or None).
    Rows are labels 1 .. n (n: the image's maximum by default); an absent label is NaN in all 80 columns."""
    labels = np.asarray(labels)
    n = int(labels.max()) if n is None else n
    values, scale, objects = np.full((n, 80), np.nan), np.full((n, 80), np.nan), []
    for L in range(1, n + 1):
        ys, xs = np.nonzero(labels == L)
        if len(ys) == 0:
            objects.append(None)
            continue
        y0, x0 = int(ys.min()), int(xs.min())
        o = measure(labels[y0:int(ys.max()) + 1, x0:int(xs.max()) + 1] == L, y0, x0)
        values[L - 1], scale[L - 1] = o["values"], o["scale"]
        objects.append(o)
    return dict(values=values, scale=scale, objects=objects)


def reference_batch(labels):
    """[F, Y, X] with the same number of rows per tile (the largest label of each) -> the rows tile after tile."""
    refs = [reference(t) for t in labels]
    return dict(values=np.concatenate([r["values"] for r in refs]), scale=np.concatenate([r["scale"] for r in refs]),
                objects=[o for r in refs for o in r["objects"]])


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Equal bit for bit, NaN in the same places (whatever the NaN's payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def check(got, ref, what, names=ALL_NAMES, bitwise=BITWISE, verbose=True):
    """got [n, len(names)] against the reference's rows by the rule of the module docstring; prints the worst error of each class
    (in units of its allowance) before it asserts.  -> {class: (worst error / allowance, column)}."""
    got = np.asarray(got, np.float64)
    want, scale = ref["values"], ref["scale"]
    assert got.shape == (len(want), len(names)), (what, got.shape)
    areas = np.asarray([o["area"] if o else 0 for o in ref["objects"]], float)
    present = areas > 0
    worst, failures = {}, []

    def note(cls, name, ratio, rows):
        ratio = np.where(np.isnan(ratio), 0.0, ratio)
        if len(ratio) and ratio.max() >= worst.get(cls, (-1.0, ""))[0]:
            worst[cls] = (float(ratio.max()), name)
        for i in np.nonzero(ratio > 1.0)[0]:
            failures.append((cls, name, int(rows[i]), float(g[rows[i]]), float(w[rows[i]]), float(ratio[i])))

    for j, name in enumerate(names):
        k = COL[name]
        g, w, s = got[:, j], want[:, k], scale[:, k]
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            failures.append(("nan pattern", name, -1, 0.0, 0.0, 0.0))
            continue
        rows = np.nonzero(present & ~np.isnan(w))[0]
        if name in bitwise:
            if not same_bits(g, w):
                failures.append(("bit for bit", name, -1, 0.0, 0.0, 0.0))
            continue
        if not np.array_equal(g[rows][np.isinf(w[rows])], w[rows][np.isinf(w[rows])]):  # (FormFactor of a perimeter of 0)
            failures.append(("infinite", name, -1, 0.0, 0.0, 0.0))
            continue
        rows = rows[np.isfinite(w[rows])]
        s = np.where(np.isnan(s), np.abs(w), s)[rows]
        err = np.abs(g[rows] - w[rows])
        if name in FERET:
            zero = w[rows] == 0
            if not same_bits(g[rows][zero], w[rows][zero]):
                failures.append(("bit for bit where 0", name, -1, 0.0, 0.0, 0.0))
        if name == "Orientation":
            note("orientation / 1e-12 deg", name, err / ORIENTATION_ATOL_DEG, rows)
        elif name in SUMMED:
            allow = 4 * areas[rows] * U * s
            note("summed / (4 N 2^-53 scale)", name, np.where(err == 0, 0.0, err / np.where(allow > 0, allow, np.finfo(float).tiny)), rows)
        else:
            allow = DERIVED_RTOL * s
            note("derived / (1e-14 scale)", name, np.where(err == 0, 0.0, err / np.where(allow > 0, allow, np.finfo(float).tiny)), rows)
    if verbose:
        print(f"[{what}] " + "; ".join(f"{c}: {r:.3g} ({n})" for c, (r, n) in sorted(worst.items())))
    assert not failures, (what, failures[:8])
    return worst


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
def _draw(tile, L, y, x, rows):
    for i, row in enumerate(rows):
        for j, ch in enumerate(row):
            if ch == "X":
                assert tile[y + i, x + j] == 0
                tile[y + i, x + j] = L


def _arc(R):
    """A one-pixel-thick, 8-connected quarter circle of radius R in a (R + 1)^2 box, symmetric under r <-> c."""
    m = np.zeros((R + 1, R + 1), bool)
    for c in range(R + 1):
        r = int(round(math.sqrt(R * R - c * c)))
        m[r, c] = m[c, r] = True
    return m


# label -> (name, top row, left column, picture) on the 64 x 96 tile; labels 8 and 15 are absent
SMALL = {
    1: ("pixel in the corner", 0, 0, ["X"]),
    2: ("1x2 on the top edge", 0, 4, ["XX"]),
    3: ("2x2 in the top right corner", 0, 94, ["XX", "XX"]),
    4: ("1x9 on the bottom edge", 63, 2, ["XXXXXXXXX"]),
    5: ("9x1 on the left edge", 10, 0, ["X"] * 9),
    6: ("diagonal down-right, 7", 4, 10, ["." * i + "X" for i in range(7)]),
    7: ("diagonal down-left, 7", 4, 20, ["." * (6 - i) + "X" for i in range(7)]),
    9: ("ring", 4, 30, ["XXXXXXX", "XXXXXXX", "XX...XX", "XX...XX", "XX...XX", "XXXXXXX", "XXXXXXX"]),
    10: ("two components, empty rows between", 4, 40, ["XXX...", "XXX...", "......", "......", "......", "....XX"]),
    11: ("6x6 checkerboard", 4, 50, ["X.X.X.", ".X.X.X"] * 3),
    12: ("5x5 square", 14, 24, ["XXXXX"] * 5),
    13: ("plus sign", 14, 32, ["..X..", "..X..", "XXXXX", "..X..", "..X.."]),
    14: ("L of a 10x2 and a 2x10 bar", 22, 4, ["XX........"] * 8 + ["XXXXXXXXXX"] * 2),
    16: ("right triangle", 22, 18, ["X" * (i + 1) for i in range(7)]),
    17: ("S heptomino", 22, 28, ["XXX..", "..X..", "..XXX"]),
    18: ("3x4 block in the last corner", 61, 92, ["XXXX"] * 3),
    19: ("one-pixel spiral", 36, 4, ["XXXXXXX", "......X", "XXXXX.X", "X...X.X", "X.XXX.X", "X.....X", "XXXXXXX"]),
    20: ("barrel", 36, 14, [".X.", "XXX", "XXX", "XXX", ".X."]),
    21: ("one-pixel C", 36, 20, ["XXXX", "X...", "X...", "X...", "XXXX"]),
}
N_SMALL = 21
ABSENT = (8, 15)


def _small_tile():
    t = np.zeros((64, 96), np.uint16)
    for L, (_, y, x, rows) in SMALL.items():
        _draw(t, L, y, x, rows)
    return t


def _mirrored(tile):
    return np.stack([tile, tile[:, ::-1]]).copy()


def _single(shape, mask, y, x):
    t = np.zeros(shape, np.uint16)
    t[y:y + mask.shape[0], x:x + mask.shape[1]][mask] = 1
    return t


# case -> the launch form of (k_shape_core, k_shape_edt, k_shape_hull) that the table's true limits select, by `forms` of
# tests/test_gpu_object_forms.py ("lds", "attr": LDS above 48 KiB, "glob"); asserted by tests/test_cpu_shape_ref.py
CASES = {
    "small": ("lds", "lds", "lds"),
    "diagonal80": ("lds", "attr", "lds"),       # (h + 2)(w + 2) = 6724 cells: 52.5 KiB
    "diagonal130": ("lds", "glob", "lds"),      # 17424 cells > 16384
    "arc220": ("attr", "glob", "lds"),          # (h + 4)(w + 4) = 50625 bytes
    "arc330": ("glob", "glob", "attr"),         # 112225 bytes; 152 * 331 + 48 = 50360 bytes of hull rows
    "line400": ("lds", "lds", "attr"),
    "line650": ("lds", "lds", "glob"),          # 152 * 650 + 48 = 98848 bytes > 96 KiB
}


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """-> labels uint16 [2, Y, X]: tile 1 is tile 0 mirrored left-right (the tile offset and the X columns matter)."""
    if name == "small":
        lab = _mirrored(_small_tile())
    elif name.startswith("diagonal"):
        n = int(name[8:])
        lab = _mirrored(_single((n + 8, n + 8), np.eye(n, dtype=bool), 3, 5))
    elif name.startswith("arc"):
        R = int(name[3:])
        lab = _mirrored(_single((R + 6, R + 6), _arc(R), 2, 3))
    elif name.startswith("line"):
        n = int(name[4:])
        lab = _mirrored(_single((n + 10, 8), np.ones((n, 1), bool), 6, 2))
    else:
        raise KeyError(name)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def catalogue_reference(name):
    return reference_batch(catalogue(name))


def table_limits(labels):
    """(max_h, max_w, max_area) of the object table of a batch."""
    mh = mw = ma = 0
    for t in labels:
        for L in range(1, int(t.max()) + 1):
            ys, xs = np.nonzero(t == L)
            if len(ys):
                mh, mw, ma = max(mh, int(np.ptp(ys)) + 1), max(mw, int(np.ptp(xs)) + 1), max(ma, len(ys))
    return mh, mw, ma
