"""
TEST INFRASTRUCTURE — references of the three 2-D kernels that are driven by an object's geometry and are not size/shape
kernels: k_mec and k_zernike / k_zernike_multi (aliby_amd/csrc/feat_zernike.hip) and k_radial_geometry / k_radial_stats
(aliby_amd/csrc/feat_radial.hip); the winding shapes that go with the catalogue of tests/shape_ref.py; and the rules the results
are compared by.  Plain Python on integers, `fractions`, `decimal` and `mpmath`: it imports nothing of aliby_amd, and it shares
no formulation with oracle/zernike_restated.py (Welzl in float64) or oracle/radial_restated.py (scipy's EDT, float Dijkstra).
tests/test_cpu_geometry_ref.py pins it to those oracles and checks the preconditions of tests/test_gpu_geometry.py.

    mec_exact        the hull of the pixel centres by gift wrapping over ALL the pixels (no row extremes), then every pair and
                     every non-collinear triple of hull vertices in rationals: the smallest circle that contains every vertex.
                     At most 40 hull vertices (the enumeration is cubic).
    mec_certificate  no search: a given float circle is the minimum one if every point is inside r (1 + 1e-12) and the points
                     within 1e-9 r of it hold two antipodal points or three whose triangle contains the centre (the minimum
                     enclosing circle is unique).  For the arcs, whose hulls are the largest (32 vertices at
                     radius 220: a digitised arc is not strictly convex; the enumeration above still confirms it there).
    mec_exact_near   the exact circle of such an object: the circles through pairs and non-obtuse triples of the points that lie
                     within 1e-9 r of a float answer, the one that contains every point in exact arithmetic.  A pair is antipodal
                     on its own circle and a non-obtuse triangle contains its circumcentre, so containing every point proves it.
    zernike_ref      about the exact centre c and r^2 (rationals), y = (i - ci) / r and x = (j - cj) / r: rho^2 = x^2 + y^2 is a
                     rational and (y + i x)^m = (U + i V)^m / (q r)^m with integers U, V.  The sum over the pixels of
                     R_nm(rho^2) (y + i x)^m is therefore taken EXACTLY, as a Gaussian integer over a per-column constant, and
                     only the division by r^m, the magnitude, pi and atan2 are rounded — at 50 digits (mpmath).  A pixel is
                     outside the disc where rho^2 > 1, decided in integers.  S = the sum of the terms' magnitudes (float64).
    radial_codes     d^2 to the nearest non-object pixel of the FRAME by brute force in integers; centre = the last raster pixel of
                     maximal d^2; Dijkstra over the 8-neighbourhood on exact (edge steps, diagonal steps) pairs, cost
                     e / sqrt(2) + d at 50 digits (two different pairs never cost the same: sqrt(2) is irrational); ring =
                     floor(bin_count nrm) at 50 digits; wedge = (i > ic) + 2 (j > jc) + 4 (|i - ic| > |j - jc|);
                     code = 0x80 | wedge << 4 | ring, 0 where no path leads.
    radial_columns   FracAtD, MeanFrac in rationals, RadialCV at 50 digits, from a code map and a pixel plane.
"""
import functools
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import mpmath
import numpy as np

from tests import shape_ref

DIGITS = 50
U53 = 2.0 ** -53
ZERNIKE_NM = tuple((n, m) for n in range(10) for m in range(n % 2, n + 1, 2))  # centrosome's get_zernike_indexes(10)
assert len(ZERNIKE_NM) == 30
EPS = Fraction(2.220446049250313e-16)  # numpy's float64 eps, the constant of MeanFrac
VANISHING = 1e-9  # a moment below it has no phase (tests/test_gpu_object_forms.py, compare)


# ---- minimum enclosing circle -------------------------------------------------------------------------------------------------
def hull_vertices(points):
    """Hull vertices in order of the distinct integer points, collinear points dropped: one point -> 1, a straight line -> 2."""
    pts = sorted(set((int(r), int(c)) for r, c in points))
    if len(pts) == 1:
        return pts
    start = pts[0]
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


def _circle2(a, b):
    return Fraction(a[0] + b[0], 2), Fraction(a[1] + b[1], 2), Fraction((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2, 4)


def _circle3(a, b, c):
    """Circumcircle in rationals, None where the three are collinear."""
    d = 2 * (a[0] * (b[1] - c[1]) + b[0] * (c[1] - a[1]) + c[0] * (a[1] - b[1]))
    if d == 0:
        return None
    a2, b2, c2 = a[0] ** 2 + a[1] ** 2, b[0] ** 2 + b[1] ** 2, c[0] ** 2 + c[1] ** 2
    ci = Fraction(a2 * (b[1] - c[1]) + b2 * (c[1] - a[1]) + c2 * (a[1] - b[1]), d)
    cj = Fraction(a2 * (c[0] - b[0]) + b2 * (a[0] - c[0]) + c2 * (b[0] - a[0]), d)
    return ci, cj, (a[0] - ci) ** 2 + (a[1] - cj) ** 2


def _contains(circle, pts):
    ci, cj, r2 = circle
    return all((p[0] - ci) ** 2 + (p[1] - cj) ** 2 <= r2 for p in pts)


def mec_exact(points):
    """-> (ci, cj, r^2) as Fractions: every pair and every non-collinear triple of the hull vertices, the smallest circle that
    contains them all."""
    hv = hull_vertices(points)
    assert len(hv) <= 40, len(hv)
    if len(hv) == 1:
        return Fraction(hv[0][0]), Fraction(hv[0][1]), Fraction(0)
    best = None
    for i in range(len(hv)):
        for j in range(i + 1, len(hv)):
            c = _circle2(hv[i], hv[j])
            if (best is None or c[2] < best[2]) and _contains(c, hv):
                best = c
            for k in range(j + 1, len(hv)):
                c = _circle3(hv[i], hv[j], hv[k])
                if c is not None and (best is None or c[2] < best[2]) and _contains(c, hv):
                    best = c
    assert best is not None
    return best


def _support(points, ci, cj, r):
    ci, cj, r = Fraction(float(ci)), Fraction(float(cj)), Fraction(float(r))
    lo, hi = (r * (1 - Fraction(1, 10 ** 9))) ** 2, (r * (1 + Fraction(1, 10 ** 12))) ** 2
    d2 = [(p[0] - ci) ** 2 + (p[1] - cj) ** 2 for p in points]
    return (ci, cj, r), [p for p, d in zip(points, d2) if d >= lo], all(d <= hi for d in d2)


def mec_certificate(points, ci, cj, r):
    """True where the float circle (ci, cj, r) is the minimum enclosing circle of the integer points, by the certificate of the
    module docstring; exact arithmetic on the floats as they are."""
    pts = sorted(set((int(a), int(b)) for a, b in points))
    (ci, cj, r), sup, inside = _support(pts, ci, cj, r)
    if not inside:
        return False
    if r == 0:
        return len(pts) == 1
    tol = r / 10 ** 9
    for a in range(len(sup)):
        for b in range(a + 1, len(sup)):
            mi, mj = Fraction(sup[a][0] + sup[b][0], 2) - ci, Fraction(sup[a][1] + sup[b][1], 2) - cj
            if mi * mi + mj * mj <= tol * tol:
                return True  # antipodal
    for a in range(len(sup)):
        for b in range(a + 1, len(sup)):
            for c in range(b + 1, len(sup)):
                A, B, C = sup[a], sup[b], sup[c]
                s = [(Q[0] - P[0]) * (cj - P[1]) - (Q[1] - P[1]) * (ci - P[0]) for P, Q in ((A, B), (B, C), (C, A))]
                if all(v >= -tol * r for v in s) or all(v <= tol * r for v in s):
                    if (B[0] - A[0]) * (C[1] - A[1]) != (B[1] - A[1]) * (C[0] - A[0]):
                        return True
    return False


def mec_exact_near(points, ci, cj, r):
    """-> (ci, cj, r^2) as Fractions from a float answer, proven in exact arithmetic (module docstring)."""
    pts = sorted(set((int(a), int(b)) for a, b in points))
    if len(pts) == 1:
        return Fraction(pts[0][0]), Fraction(pts[0][1]), Fraction(0)
    _, sup, _ = _support(pts, ci, cj, r)
    assert 2 <= len(sup) <= 40, len(sup)
    for a in range(len(sup)):
        for b in range(a + 1, len(sup)):
            c = _circle2(sup[a], sup[b])
            if _contains(c, pts):
                return c
            for k in range(b + 1, len(sup)):
                A, B, C = sup[a], sup[b], sup[k]
                e = sorted(((A[0] - B[0]) ** 2 + (A[1] - B[1]) ** 2, (A[0] - C[0]) ** 2 + (A[1] - C[1]) ** 2, (B[0] - C[0]) ** 2 + (B[1] - C[1]) ** 2))
                c = _circle3(A, B, C)
                if c is not None and e[2] <= e[0] + e[1] and _contains(c, pts):
                    return c
    raise AssertionError("the float circle is not the minimum enclosing circle")


# ---- Zernike moments ----------------------------------------------------------------------------------------------------------
def _lut(n, m):
    """(-1)^t (n - t)! / (t! ((n + m) / 2 - t)! ((n - m) / 2 - t)!) for t = 0 .. (n - m) / 2: integers."""
    out = []
    for t in range((n - m) // 2 + 1):
        f = Fraction((-1) ** t * math.factorial(n - t), math.factorial(t) * math.factorial((n + m) // 2 - t) * math.factorial((n - m) // 2 - t))
        assert f.denominator == 1
        out.append(int(f))
    return out


_LUT = {nm: _lut(*nm) for nm in ZERNIKE_NM}


def _exact_weights(weights):
    """values -> (integers W, the integer den) with value = W / den exactly (uint16: den = 1; float32: a power of two)"""
    if weights.dtype.kind in "ui":
        return [int(v) for v in weights], 1
    fr = [Fraction(float(v)) for v in weights]
    den = max(f.denominator for f in fr)  # powers of two: the largest is the common one
    return [int(f * den) for f in fr], den


def zernike_ref(mask, y0, x0, weights=None, circle=None):
    """One object from its bounding-box crop (bool [h, w]), the crop's corner and, for radial_zernikes, the pixel crop [h, w].
    circle: (ci, cj, r^2) as Fractions where mec_exact cannot give it (the arcs).
    -> dict(mag [30], phase [30] (weighted only), S [30], normaliser, vanishing: the number of moments below 1e-9).
    mag = |sum Z| / (pi r^2) unweighted, |sum w Z| / N weighted; phase = atan2(Re, Im); S = sum |w| |Z| (not normalised)."""
    ii, jj = np.nonzero(mask)
    pts = [(int(i) + y0, int(j) + x0) for i, j in zip(ii, jj)]
    ci, cj, r2 = circle if circle is not None else mec_exact(pts)
    nan = np.full(30, np.nan)
    if r2 == 0:  # one pixel: x and y are 0 / 0
        return dict(mag=nan, phase=None if weights is None else nan.copy(), S=nan.copy(), normaliser=0.0, vanishing=0, circle=(ci, cj, r2))
    W, wden = ([1] * len(pts), 1) if weights is None else _exact_weights(np.asarray(weights)[ii, jj])
    q = ci.denominator * cj.denominator // math.gcd(ci.denominator, cj.denominator)
    Ci, Cj = int(ci * q), int(cj * q)
    P, Q = r2.numerator, r2.denominator
    Dn = q * q * P  # rho^2 = N2 / Dn
    re, im, S = [0] * 30, [0] * 30, [0.0] * 30
    dpow = [Dn ** t for t in range(6)]
    for (i, j), w in zip(pts, W):
        Uu, Vv = i * q - Ci, j * q - Cj
        N2 = (Uu * Uu + Vv * Vv) * Q
        if N2 > Dn:
            continue
        rho = math.sqrt(N2 / Dn)
        pw = [(1, 0)]
        for _ in range(9):
            a, b = pw[-1]
            pw.append((a * Uu - b * Vv, a * Vv + b * Uu))  # (y + i x)^m with y the row and x the column offset
        wf = abs(w) / wden
        for col, (n, m) in enumerate(ZERNIKE_NM):
            k = (n - m) // 2
            R = 0
            for t, c in enumerate(_LUT[(n, m)]):
                R = R * N2 + c * dpow[t]  # R_nm(rho^2) Dn^k
            re[col] += w * R * pw[m][0]
            im[col] += w * R * pw[m][1]
            S[col] += wf * (abs(R) / dpow[k]) * rho ** m
    with mpmath.workdps(DIGITS):
        r = mpmath.sqrt(mpmath.mpf(P) / Q)
        norm = mpmath.pi * r * r if weights is None else mpmath.mpf(len(pts))
        mag, phase, vanishing = np.empty(30), np.empty(30), 0
        for col, (n, m) in enumerate(ZERNIKE_NM):
            scale = mpmath.mpf(Dn) ** ((n - m) // 2) * (q * r) ** m * wden
            vr, vi = mpmath.mpf(re[col]) / scale, mpmath.mpf(im[col]) / scale
            mg = mpmath.sqrt(vr * vr + vi * vi) / norm
            mag[col] = float(mg)
            phase[col] = float(mpmath.atan2(mpmath.mpf(re[col]), mpmath.mpf(im[col])))
            vanishing += int(mg < VANISHING)
        return dict(mag=mag, phase=None if weights is None else phase, S=np.asarray(S), normaliser=float(norm), vanishing=vanishing,
                    circle=(ci, cj, r2))


def rho2_of_pixels(mask, y0, x0, circle):
    """-> the exact rho^2 of every object pixel (Fractions), r^2 > 0"""
    ci, cj, r2 = circle
    ii, jj = np.nonzero(mask)
    return [((int(i) + y0 - ci) ** 2 + (int(j) + x0 - cj) ** 2) / r2 for i, j in zip(ii, jj)]


# ---- radial geometry ----------------------------------------------------------------------------------------------------------
def _inv_sqrt2():
    return 1 / Decimal(2).sqrt()


def radial_paths(labels_tile, label):
    """One object of one tile -> dict(ys, xs: its pixels in raster order; d2: squared distance to the nearest non-object pixel of
    the frame; centre: index of the last raster pixel of maximal d2; n_max: how many pixels have that d2; e, d: edge and diagonal
    steps of the cheapest path from the centre, -1 where there is none), or None where the label is absent."""
    lab = np.asarray(labels_tile)
    ys, xs = np.nonzero(lab == label)
    if len(ys) == 0:
        return None
    by, bx = np.nonzero(lab != label)
    assert len(by), "an object that fills the frame has no distance to an edge"
    d2 = shape_ref._min_d2(ys, xs, by, bx).tolist()
    top = max(d2)
    centre = max(k for k, v in enumerate(d2) if v == top)
    index = {(int(y), int(x)): k for k, (y, x) in enumerate(zip(ys, xs))}
    e, d = [-1] * len(ys), [-1] * len(ys)
    with localcontext() as ctx:
        ctx.prec = DIGITS
        s = _inv_sqrt2()
        cost = {centre: Decimal(0)}
        e[centre] = d[centre] = 0
        done, frontier = set(), {centre}
        while frontier:
            k = min(frontier, key=cost.__getitem__)  # (plain Dijkstra: a few thousand pixels at most)
            frontier.discard(k)
            done.add(k)
            y, x = int(ys[k]), int(xs[k])
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    n = index.get((y + dy, x + dx))
                    if n is None or n in done or (dy == 0 and dx == 0):
                        continue
                    ne, nd = (e[k], d[k] + 1) if dy and dx else (e[k] + 1, d[k])
                    c = ne * s + nd
                    if n not in cost or c < cost[n]:
                        cost[n], e[n], d[n] = c, ne, nd
                        frontier.add(n)
    return dict(ys=ys, xs=xs, d2=d2, centre=centre, n_max=d2.count(top), e=e, d=d)


def radial_codes(labels_tile, label, bin_count, maximum_radius=None, detail=False):
    """-> uint8 [Y, X]: the expected code of every pixel of the object, 0 elsewhere (and 0 on its pixels no path reaches).
    detail=True: -> (codes, [bin_count * nrm per reached pixel as a Decimal], paths)."""
    lab = np.asarray(labels_tile)
    codes = np.zeros(lab.shape, np.uint8)
    p = radial_paths(lab, label)
    if p is None:
        return (codes, [], None) if detail else codes
    yc, xc = int(p["ys"][p["centre"]]), int(p["xs"][p["centre"]])
    scaled_values = []
    with localcontext() as ctx:
        ctx.prec = DIGITS
        s = _inv_sqrt2()
        for k in range(len(p["ys"])):
            if p["e"][k] < 0:
                continue
            dfrom = p["e"][k] * s + p["d"][k]
            if maximum_radius is None:
                nrm = dfrom / (dfrom + Decimal(p["d2"][k]).sqrt() + Decimal("0.001"))
            else:
                nrm = dfrom / Decimal(maximum_radius)
            v = nrm * bin_count
            scaled_values.append(v)
            ring = min(int(v), bin_count)
            y, x = int(p["ys"][k]), int(p["xs"][k])
            wedge = (y > yc) + 2 * (x > xc) + 4 * (abs(y - yc) > abs(x - xc))
            codes[y, x] = 0x80 | (wedge << 4) | ring
    return (codes, scaled_values, p) if detail else codes


def radial_columns(codes, plane, bin_count, rings):
    """The coded pixels of ONE object (codes: uint8 [Y, X], 0 elsewhere) and a pixel plane [Y, X] -> float64 [3 * rings]:
    FracAtD, MeanFrac (rationals, rounded once) and RadialCV (50 digits) per ring."""
    ys, xs = np.nonzero(codes & 0x80)
    integer = plane.dtype.kind in "ui"
    tot, cnt = [Fraction(0)] * (bin_count + 1), [0] * (bin_count + 1)
    wsum, wcnt = {}, {}
    for y, x in zip(ys.tolist(), xs.tolist()):
        c = int(codes[y, x])
        b, wd = c & 15, (c >> 4) & 7
        v = Fraction(int(plane[y, x])) if integer else Fraction(float(plane[y, x]))
        tot[b] += v
        cnt[b] += 1
        wsum[b, wd] = wsum.get((b, wd), Fraction(0)) + v
        wcnt[b, wd] = wcnt.get((b, wd), 0) + 1
    T, N = sum(tot), sum(cnt)
    out = np.empty(3 * rings)
    with mpmath.workdps(DIGITS):
        for b in range(rings):
            fd = tot[b] / T
            out[b] = float(fd)
            out[rings + b] = float(fd / (Fraction(cnt[b], N) + EPS))
            means = [wsum[b, k] / wcnt[b, k] for k in range(8) if (b, k) in wcnt]
            if means:
                mean = sum(means) / len(means)
                var = sum((m - mean) ** 2 for m in means) / len(means)
                out[2 * rings + b] = float(mpmath.sqrt(mpmath.mpf(var.numerator) / var.denominator) / (mpmath.mpf(mean.numerator) / mean.denominator))
            else:
                out[2 * rings + b] = 0.0
    return out


# ---- the winding shapes -------------------------------------------------------------------------------------------------------
def _serpentine(h, w, thick=1):
    """Full rows (bands of `thick` lines) every 2 * thick lines, joined at alternating ends: one path of about h w / 2 pixels."""
    m = np.zeros((h, w), bool)
    pitch = 2 * thick
    assert (h - thick) % pitch == 0
    for k, r in enumerate(range(0, h, pitch)):
        m[r:r + thick] = True
        if r + pitch < h:
            m[r + thick:r + pitch, w - thick:] |= (k % 2 == 0)
            m[r + thick:r + pitch, :thick] |= (k % 2 == 1)
    return m


def _square_spiral(n):
    """A one-pixel line that winds inwards from the top left corner with one pixel of background between its turns."""
    m = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turned = False

    def inside(yy, xx):
        return 0 <= yy < n and 0 <= xx < n

    while True:
        ny, nx = y + dy, x + dx
        if inside(ny, nx) and not m[ny, nx] and not (inside(ny + dy, nx + dx) and m[ny + dy, nx + dx]):
            y, x = ny, nx
            m[y, x] = True
            turned = False
            continue
        if turned:
            return m
        dy, dx, turned = dx, -dy, True  # turn right


def _two_components():
    m = np.zeros((15, 24), bool)
    m[0:5, 0:5] = True             # holds the centre (d^2 = 9 in its middle)
    m[:, 8:] = _serpentine(15, 16)  # no path leads here
    return m


# name -> (mask, whether its cheapest paths are meant to be longer than the sweeps the box once allowed)
WINDING = {
    "serpentine31x32": (lambda: _serpentine(31, 32), True),
    "serpentine32x31": (lambda: _serpentine(31, 32).T.copy(), True),
    "spiral33": (lambda: _square_spiral(33), True),
    "serpentine46x48_thick": (lambda: _serpentine(46, 48, 2), True),
    "two_components": (_two_components, False),
}
AREAS = {"serpentine31x32": 527, "serpentine32x31": 527, "spiral33": 577, "serpentine46x48_thick": 1196, "two_components": 160}


def old_sweep_cap(h, w):
    """The number of relaxation sweeps k_radial_geometry once stopped at, whatever was left to do."""
    return 4 * (h + w) + 8


@functools.lru_cache(maxsize=None)
def winding(name):
    """-> labels uint16 [2, Y, X]: the shape at (3, 5) in a tile 8 larger than its box, and the tile mirrored left-right."""
    mask = WINDING[name][0]()
    assert int(mask.sum()) == AREAS[name], (name, int(mask.sum()))
    lab = shape_ref._mirrored(shape_ref._single((mask.shape[0] + 8, mask.shape[1] + 8), mask, 3, 5))
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def frame_cases():
    """-> labels uint16 [2, 12, 16]: tile 0 holds a 5 x 6 block that fills the frame's first corner and a 4 x 4 block in its last
    one; tile 1 an object that touches all four borders and leaves one pixel of background."""
    lab = np.zeros((2, 12, 16), np.uint16)
    lab[0, 0:5, 0:6] = 1
    lab[0, 8:12, 12:16] = 2
    lab[1] = 1
    lab[1, 4, 9] = 0
    lab.setflags(write=False)
    return lab


EXTRA = ("frame12x16",)


@functools.lru_cache(maxsize=None)
def acute():
    """-> labels uint16 [2, 14, 16]: a filled triangle with the corners (2, 3), (2, 9), (7, 6).  Every circle of the catalogue and
    of the winding shapes rests on two antipodal pixels; this one rests on three — centre (18/5, 6), r = 17/5."""
    t = np.zeros((14, 16), np.uint16)
    for r in range(2, 8):
        for c in range(3, 10):
            if 5 * abs(c - 6) <= 3 * (7 - r):
                t[r, c] = 1
    lab = shape_ref._mirrored(t)
    lab.setflags(write=False)
    return lab


def labels_of(name):
    if name in shape_ref.CASES:
        return shape_ref.catalogue(name)
    if name in WINDING:
        return winding(name)
    if name == "acute":
        return acute()
    assert name == "frame12x16", name
    return frame_cases()


def objects_of(name):
    """-> [(tile, label)] for every label 1 .. max of every tile (absent ones too), in the order of the object table's rows"""
    return [(t, L) for t, tile in enumerate(labels_of(name)) for L in range(1, int(tile.max()) + 1)]


def crop(tile, label):
    """-> (mask crop, y0, x0) or None"""
    ys, xs = np.nonzero(tile == label)
    if len(ys) == 0:
        return None
    y0, x0 = int(ys.min()), int(xs.min())
    return tile[y0:int(ys.max()) + 1, x0:int(xs.max()) + 1] == label, y0, x0


# ---- pixel planes ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes(name, mode="u16"):
    """-> [F, 3, Y, X]: channel 0 holds 1 + 7 * (raster rank in the tile) mod 65521 — distinct values within any 65521 consecutive
    pixels; channels 1 and 2 other such ramps.  mode "f32": the same as float32 in [0, 1] (u16 / 65535)."""
    lab = labels_of(name)
    F, Y, X = lab.shape
    rank = np.arange(Y * X, dtype=np.int64).reshape(Y, X)
    px = np.stack([(1 + 7 * rank) % 65521, (3 + 11 * rank) % 65521, (65520 - 5 * rank) % 65521]).astype(np.uint16)
    px = np.broadcast_to(px, (F, 3, Y, X)).copy()
    if mode == "f32":
        px = (px.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    else:
        assert mode == "u16"
    px.setflags(write=False)
    return px


# ---- per case: the references, once ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_mec(name):
    """zr.minimum_enclosing_circle per row: [n, 3] (ci, cj, r), NaN where absent (CPU, float64)"""
    from oracle import zernike_restated as zr

    rows = []
    for tile in labels_of(name):
        n = int(tile.max())
        centres, radii = zr.minimum_enclosing_circle(np.asarray(tile), np.arange(1, n + 1))
        rows.append(np.column_stack([np.asarray(centres, float).reshape(n, 2), np.asarray(radii, float)]))
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def circles(name):
    """-> per row (ci, cj, r^2) as Fractions and the number of hull vertices, None where absent.  mec_exact where the hull has at
    most 40 vertices; for the arcs the exact circle near the oracle's answer (the third field says which)."""
    out = []
    want = oracle_mec(name)
    lab = labels_of(name)
    for row, (t, L) in enumerate(objects_of(name)):
        ys, xs = np.nonzero(lab[t] == L)
        if len(ys) == 0:
            out.append(None)
            continue
        pts = list(zip(ys.tolist(), xs.tolist()))
        hv = hull_vertices(pts)
        if name.startswith("arc"):
            circle = mec_exact_near(pts, *want[row])
            assert len(hv) > 40 or circle == mec_exact(pts)  # (the digitised arcs are not strictly convex: few vertices are left)
        else:
            circle = mec_exact(pts)
        out.append((circle, len(hv), not name.startswith("arc")))
    return out


@functools.lru_cache(maxsize=None)
def zernike_case(name, family):
    """family: "zernike" (unweighted), "u16" or "f32" (radial_zernikes of channel 0 of `planes`) -> dict of per-row arrays:
    mag [n, 30], phase [n, 30], S [n, 30], normaliser [n], vanishing [n], present [n]"""
    lab = labels_of(name)
    px = None if family == "zernike" else planes(name, family)
    rows = objects_of(name)
    out = dict(mag=np.full((len(rows), 30), np.nan), phase=np.full((len(rows), 30), np.nan), S=np.full((len(rows), 30), np.nan),
               normaliser=np.full(len(rows), np.nan), vanishing=np.zeros(len(rows), int), present=np.zeros(len(rows), bool))
    for row, ((t, L), circ) in enumerate(zip(rows, circles(name))):
        if circ is None:
            continue
        mask, y0, x0 = crop(lab[t], L)
        w = None if px is None else px[t, 0, y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]]
        z = zernike_ref(mask, y0, x0, w, circle=circ[0])
        out["present"][row] = True
        out["mag"][row], out["S"][row], out["normaliser"][row], out["vanishing"][row] = z["mag"], z["S"], z["normaliser"], z["vanishing"]
        if z["phase"] is not None:
            out["phase"][row] = z["phase"]
    return out


ZERNIKE_CASES = ("small", "diagonal80", "arc220", "line400") + tuple(WINDING)


@functools.lru_cache(maxsize=None)
def oracle_zernike(name, family):
    """The float64 oracle's magnitudes [n, 30] (CPU)"""
    from oracle import zernike_restated as zr

    cols = []
    for t, tile in enumerate(labels_of(name)):
        tile = np.asarray(tile)
        if family == "zernike":
            res = zr.get_zernike(tile)
            cols.append(np.column_stack([res[f"Zernike_{n}_{m}"] for n, m in ZERNIKE_NM]))
        else:
            res = zr.get_radial_zernikes(tile, planes(name, family)[t, 0])
            cols.append(np.column_stack([res[f"RadialDistribution_ZernikeMagnitude_{n}_{m}"] for n, m in ZERNIKE_NM]))
    return np.concatenate(cols)


@functools.lru_cache(maxsize=None)
def oracle_distance(family):
    """-> [30]: per column the largest distance of the float64 oracle from zernike_ref over every object of ZERNIKE_CASES, in
    units of 2^-53 S / normaliser.  Measured on the CPU against the 50-digit reference; the GPU tolerance is set from it."""
    worst = np.zeros(30)
    for name in ZERNIKE_CASES:
        ref, got = zernike_case(name, family), oracle_zernike(name, family)
        for row in np.nonzero(ref["present"] & (ref["normaliser"] > 0))[0]:
            unit = U53 * ref["S"][row] / ref["normaliser"][row]
            err = np.abs(got[row] - ref["mag"][row])
            worst = np.maximum(worst, np.where(err == 0, 0.0, err / np.where(unit > 0, unit, np.finfo(float).tiny)))
    return worst


def zernike_tolerance(family, S, normaliser, want):
    """-> [30] absolute tolerance of one row's magnitudes: 8 max(oracle's distance, 64) 2^-53 S / normaliser — 8 for the kernel's
    other order of summation (64 lane partials, then a tree), 64 where the oracle happens to be exact — and never looser than the
    project's rule (1e-4 relative, 1e-8 absolute)."""
    derived = 8 * np.maximum(oracle_distance(family), 64.0) * U53 * S / normaliser
    return np.minimum(derived, 1e-4 * np.abs(want) + 1e-8)


@functools.lru_cache(maxsize=None)
def radial_case(name, bin_count, maximum_radius=None):
    """-> (codes uint8 [F, Y, X] of every object of the case, [per row: (codes of that object alone, bin_count * nrm values,
    paths) or None])"""
    lab = labels_of(name)
    total = np.zeros(lab.shape, np.uint8)
    per_row = []
    for t, L in objects_of(name):
        codes, values, p = radial_codes(lab[t], L, bin_count, maximum_radius, detail=True)
        if p is None:
            per_row.append(None)
            continue
        assert not (total[t] & codes).any()
        total[t] |= codes
        per_row.append((codes, values, p))
    return total, per_row


def path_steps(p):
    """The number of steps on the cheapest path to the farthest reached pixel."""
    with localcontext() as ctx:
        ctx.prec = DIGITS
        s = _inv_sqrt2()
        k = max((k for k in range(len(p["e"])) if p["e"][k] >= 0), key=lambda k: p["e"][k] * s + p["d"][k])
    return p["e"][k] + p["d"][k]
