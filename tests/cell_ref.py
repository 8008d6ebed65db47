"""
TEST INFRASTRUCTURE — an exact reference of the per-cell metric kernels (aliby_amd/csrc/feat_cell.hip: k_cell;
aliby_amd/csrc/feat_extra.hip: k_cell_ratio, k_trap_background), the rule they are compared by, and the inputs of
tests/test_gpu_cell.py.  Written per object from the label image and one plane, in Python integers, exact rationals and correctly
rounded float64 operations; it shares no code with aliby_amd or with oracle/cell_metrics.py (tests/test_cpu_cell_ref.py pins it to
that oracle and to closed forms, and checks the stated precondition of every input built here).

Mask columns: the squared Euclidean distance transform d2 of the 1-padded mask by brute force over integers (the nearest pixel
that is not the object; the pad ring is one).  conical_volume = 4 sum sqrt(d2); the cone top is {d2 == max d2}; dn = distance to the
nearest top; cone_top = distance from a top to the nearest object pixel that is no top; min_ax = round(sqrt(max d2)),
maj_ax = round(max dn + sum cone_top / 2).  An object whose every pixel is a top has no such pixel: the reference module then asks
scipy for the distance transform of a frame without background, and scipy answers with the distance to the point one row above
the first column of the padded frame (oracle/cell_metrics.py, tests/test_gpu_edge_cases.py) — that number is returned here too.
"""
import functools
import math
from fractions import Fraction

import numpy as np

COLUMNS = ("area", "centroid_x", "centroid_y", "conical_volume", "eccentricity", "spherical_volume", "volume", "min_ax", "maj_ax",
           "mean", "median", "std", "total", "total_squared", "max2p5pc", "max5px_median", "moment_of_inertia")
COL = {n: i for i, n in enumerate(COLUMNS)}
N_MASK = 9  # columns 0..8 need no pixels

# ---- the rule --------------------------------------------------------------------------------------------------------------
# Bit for bit: integers below 2^53, or one or two correctly rounded IEEE operations on such integers (a quotient; a quotient of a
# quotient; a rounding to the nearest integer of a value kept 1e-6 away from a tie by the inputs).
EXACT_BOTH = ("area", "centroid_x", "centroid_y", "min_ax", "maj_ax", "median")
EXACT_U16 = ("total", "total_squared", "mean", "max2p5pc", "max5px_median")
# Sums of N non-negative float64 terms in an unspecified order: relative 4 N 2^-53 (recursive summation loses at most (N - 1) u,
# each term carries at most 3 u of its own, a reduction tree is no worse), floor 1e-13.
SUMMED_BOTH = ("conical_volume", "std", "moment_of_inertia")
SUMMED_F32 = ("mean", "total", "total_squared", "max2p5pc", "max5px_median")
# Fewer than ten float64 operations on exact inputs (the axes, the area).
DERIVED = ("volume", "eccentricity", "spherical_volume")
DERIVED_RTOL = 1e-14
SUM_FLOOR = 1e-13
U = 2.0 ** -53
TIE_MARGIN = 1e-6


def _min_d2(py, px, qy, qx):
    """For every point p the smallest squared distance to a point of q, as int64 (brute force, in chunks)."""
    out = np.empty(len(py), np.int64)
    qy, qx = qy.astype(np.int64)[None, :], qx.astype(np.int64)[None, :]
    step = max(1, (1 << 22) // max(qy.shape[1], 1))
    for s in range(0, len(py), step):
        dy = py[s:s + step].astype(np.int64)[:, None] - qy
        dx = px[s:s + step].astype(np.int64)[:, None] - qx
        out[s:s + step] = (dy * dy + dx * dx).min(axis=1)
    return out


def _half_integer_distance(x):
    return abs(x - (math.floor(x) + 0.5))


def _absent_row():
    row = np.full(len(COLUMNS), np.nan)
    # an all-False mask in the reference module: the sums are 0, both axes round to 0 (volume = 4 pi 0 0 / 3 = 0), the quotients
    # are 0 / 0
    for name in ("area", "conical_volume", "spherical_volume", "volume", "min_ax", "maj_ax", "total", "total_squared"):
        row[COL[name]] = 0.0
    return row


def _mask_columns(lab, L, row):
    ys, xs = np.nonzero(lab == L)
    n = len(ys)
    y0, x0 = int(ys.min()), int(xs.min())
    h, w = int(ys.max()) - y0 + 1, int(xs.max()) - x0 + 1
    m = np.zeros((h + 2, w + 2), bool)
    m[ys - y0 + 1, xs - x0 + 1] = True
    oy, ox = np.nonzero(m)
    by, bx = np.nonzero(~m)
    d2 = _min_d2(oy, ox, by, bx)
    dmax = int(d2.max())
    top = d2 == dmax
    ty, tx = oy[top], ox[top]
    max_dn = math.sqrt(int(_min_d2(oy, ox, ty, tx).max()))
    all_top = bool(top.all())
    if not all_top:
        cone = [math.sqrt(int(v)) for v in _min_d2(ty, tx, oy[~top], ox[~top])]
    else:  # rows and columns of the padded full frame; the point is (-1, 0)
        cone = [math.sqrt((int(r) + y0 + 1) ** 2 + (int(c) + x0) ** 2) for r, c in zip(ty, tx)]
    major = max_dn + math.fsum(cone) / 2.0
    min_ax, maj_ax = float(round(math.sqrt(dmax))), float(round(major))
    row[COL["area"]] = float(n)
    row[COL["centroid_x"]] = int((xs.astype(np.int64) + 1).sum()) / n  # int / int: correctly rounded
    row[COL["centroid_y"]] = int((ys.astype(np.int64) + 1).sum()) / n
    row[COL["conical_volume"]] = 4.0 * math.fsum(math.sqrt(int(v)) for v in d2)
    row[COL["eccentricity"]] = math.sqrt(maj_ax ** 2 - min_ax ** 2) / maj_ax
    r = math.sqrt(n / math.pi)
    row[COL["spherical_volume"]] = (4 * math.pi * r ** 3) / 3
    row[COL["volume"]] = (4 * math.pi * min_ax ** 2 * maj_ax) / 3
    row[COL["min_ax"]], row[COL["maj_ax"]] = min_ax, maj_ax
    return dict(n=n, box=(h, w), all_top=all_top, n_top_pixels=int(top.sum()), major=major, tie=_half_integer_distance(major),
                sqrt_tie=_half_integer_distance(math.sqrt(dmax)), ys=ys, xs=xs, y0=y0, x0=x0)


def _f(q):
    """Correctly rounded float64 of an exact int or Fraction."""
    return float(q) if isinstance(q, Fraction) else q / 1


def _pixel_columns(plane, info, row):
    ys, xs, n = info["ys"], info["xs"], info["n"]
    raw = plane[ys, xs]
    is_u16 = plane.dtype == np.uint16
    if is_u16:
        v = [int(t) for t in raw]
        squares = [(t * t) & 0xFFFF for t in v]  # uint16 ** 2 wraps
        info["true_sq"] = sum(t * t for t in v)
    else:
        assert plane.dtype == np.float32
        v = [Fraction(float(t)) for t in raw]
        squares = [Fraction(float(t * t)) for t in raw]  # the square is taken in float32
    s = sum(v)
    srt = sorted(v)
    med = float(srt[n // 2]) if n & 1 else (float(srt[n // 2 - 1]) + float(srt[n // 2])) * 0.5  # both exact in float64
    n_top = int(math.ceil(n * 0.025))  # the float product, as the reference takes it
    var_num = n * sum(t * t for t in v) - s * s
    row[COL["mean"]] = _f(Fraction(s, n))
    row[COL["median"]] = med
    row[COL["std"]] = math.sqrt(_f(Fraction(var_num, n * n)))
    row[COL["total"]] = _f(Fraction(s))
    row[COL["total_squared"]] = _f(Fraction(sum(squares)))
    row[COL["max2p5pc"]] = _f(Fraction(sum(srt[n - n_top:]), n_top))
    if n > 5 and med != 0.0:
        row[COL["max5px_median"]] = (_f(Fraction(sum(srt[n - 5:]))) / 5.0) / med
    if s != 0:
        cx = [int(x) - info["x0"] + 1 for x in xs]  # any origin: the moments are central
        cy = [int(y) - info["y0"] + 1 for y in ys]
        sx, sy = sum(t * c for t, c in zip(v, cx)), sum(t * c for t, c in zip(v, cy))
        sxx, syy = sum(t * c * c for t, c in zip(v, cx)), sum(t * c * c for t, c in zip(v, cy))
        # mu20 = sum v (x - sx / s)^2 = (s sxx - sx^2) / s, likewise mu02; the moment is (mu20 + mu02) / s^2
        row[COL["moment_of_inertia"]] = _f(Fraction(s * sxx - sx * sx + s * syy - sy * sy, s * s * s))
    info["n_top"] = n_top


def cell_metrics(lab, plane, n):
    """lab [Y, X] uint16, plane [Y, X] uint16 / float32 or None, rows for labels 1..n -> (float64 [n, 17], meta per row).
    Without a plane columns 9..16 of present objects are NaN (nothing is written there)."""
    want = np.full((n, len(COLUMNS)), np.nan)
    meta = []
    present = set(np.unique(lab).tolist())
    for L in range(1, n + 1):
        if L not in present:
            want[L - 1] = _absent_row()
            meta.append(dict(n=0, tie=0.5, sqrt_tie=0.5, all_top=False))
            continue
        info = _mask_columns(lab, L, want[L - 1])
        if plane is not None:
            _pixel_columns(plane, info, want[L - 1])
        meta.append(info)
    return want, meta


def cell_metrics_batch(labels, planes, channel, counts):
    """labels [F, Y, X], planes [F, C, Y, X] or None -> the rows of every tile, tile after tile."""
    rows, meta = [], []
    for f, n in enumerate(counts):
        w, m = cell_metrics(labels[f], None if planes is None else planes[f, channel], int(n))
        rows.append(w)
        meta += m
    return np.concatenate(rows) if rows else np.zeros((0, len(COLUMNS))), meta


def ratio(lab, p0, p1, n):
    """cell.ratio for labels 1..n: the median of p0 / p1 over the object (float64 quotients of uint16 pixels, float32 quotients of
    float32 pixels; the midpoint of an even count in float64), NaN when the object is absent or any p1 of it is 0."""
    out = np.full(n, np.nan)
    for L in range(1, n + 1):
        ys, xs = np.nonzero(lab == L)
        a, b = p0[ys, xs], p1[ys, xs]
        if len(ys) == 0 or (b == 0).any():
            continue
        if p0.dtype == np.uint16:
            q = sorted(float(s) / float(t) for s, t in zip(a, b))
        else:
            q = sorted(float(np.float32(s) / np.float32(t)) for s, t in zip(a, b))
        k = len(q)
        out[L - 1] = q[k // 2] if k & 1 else (q[k // 2 - 1] + q[k // 2]) * 0.5
    return out


def trap_background(lab, plane):
    """(median, mean of the five largest) of the pixels under no label; (NaN, NaN) when every pixel is labelled."""
    bg = sorted(float(t) for t in plane[lab == 0])
    k = len(bg)
    if k == 0:
        return math.nan, math.nan
    med = bg[k // 2] if k & 1 else (bg[k // 2 - 1] + bg[k // 2]) * 0.5
    top = bg[-5:]
    return med, _f(Fraction(sum(Fraction(t) for t in top), len(top)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _terms(name, info):
    if name == "max2p5pc":
        return info.get("n_top", 1)
    if name == "max5px_median":
        return 5
    return info["n"]


def check(got, want, meta, what, dtype="u16", pixels=True):
    """The rule of the head of this file; prints the worst relative error of every column and returns it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (len(meta), len(COLUMNS)), (what, got.shape, want.shape, len(meta))
    worst = {}
    bad = []
    exact = EXACT_BOTH + (EXACT_U16 if dtype == "u16" else ())
    for name in COLUMNS[: len(COLUMNS) if pixels else N_MASK]:
        j = COL[name]
        g, w = got[:, j], want[:, j]
        nan = np.isnan(w)
        if not np.array_equal(np.isnan(g), nan):
            bad.append((name, "NaN rows", np.flatnonzero(np.isnan(g) != nan)[:6].tolist()))
            continue
        g, w, rows = g[~nan], w[~nan], np.flatnonzero(~nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(w == 0, np.where(g == 0, 0.0, np.inf), np.abs(g - w) / np.abs(w))
        worst[name] = float(rel.max()) if len(rel) else 0.0
        if name in exact:
            ok = _bits(g) == _bits(w)
        elif name in DERIVED:
            ok = rel <= DERIVED_RTOL
        else:
            assert name in SUMMED_BOTH or (dtype != "u16" and name in SUMMED_F32), name
            tol = np.asarray([max(4.0 * _terms(name, meta[i]) * U, SUM_FLOOR) for i in rows])
            ok = rel <= tol
        if not ok.all():
            k = int(np.flatnonzero(~ok)[0])
            bad.append((name, int(rows[k]), float(g[k]), float(w[k]), float(rel[k]), int((~ok).sum())))
    print(f"[cell {what} {dtype}] worst relative error: " + ", ".join(f"{k}={v:.2e}" for k, v in worst.items()))
    assert not bad, f"{what} ({dtype}) (column, row, kernel, reference, relative error, rows): {bad}"
    return worst


# ---- the launch form, restated from aliby_features_cell and block_bitonic_sort -------------------------------------------------
def table_limits(labels, counts=None):
    """(max_h, max_w, max_area, the label supplying each) over every present object of [F, Y, X] labels, as the object table has them."""
    best = dict(h=(0, None), w=(0, None), area=(0, None))
    for f in range(labels.shape[0]):
        for L in np.unique(labels[f]):
            if L == 0 or (counts is not None and L > counts[f]):
                continue
            ys, xs = np.nonzero(labels[f] == L)
            for key, val in (("h", int(ys.max() - ys.min()) + 1), ("w", int(xs.max() - xs.min()) + 1), ("area", len(ys))):
                if val > best[key][0]:
                    best[key] = (val, (f, int(L)))
    return best["h"][0], best["w"][0], best["area"][0], (best["h"][1], best["w"][1], best["area"][1])


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def launch_form(max_h, max_w, max_area):
    """("lds", threads) or ("global", 256): LDS while (max_h + 2)(max_w + 2) 8 + pow2(max_area) 4 <= 128 KiB (the cell count
    rounded up to a multiple of 4, the value count at least 64), threads 64 / 128 / 256 by max_h max_w <= 2048 / <= 8192 / above."""
    cells = ((max_h + 2) * (max_w + 2) + 3) & ~3
    need = cells * 8 + max(64, _pow2(max_area)) * 4
    if need > 128 * 1024:
        return ("global", 256)
    work = max_h * max_w
    return ("lds", 64 if work <= 2048 else (128 if work <= 8192 else 256))


def sort_form(threads, area):
    n2 = _pow2(area)
    if threads > 64:
        return "several waves, generic loop"
    if n2 <= 64:
        return "one wave, padded in registers"
    if n2 <= 512:
        return f"one wave, {n2} in registers"
    if n2 == 1024:
        return "one wave, two register halves and an LDS merge"
    return "one wave, generic loop"


# ---- inputs ------------------------------------------------------------------------------------------------------------------
LADDER = ((1, 1), (2, 2), (5, 5), (6, 3), (63, 8), (64, 8), (65, 8), (128, 16), (129, 16), (256, 16), (257, 16), (512, 32), (513, 32),
          (1024, 32), (1025, 33), (2048, 64))  # (area, row width): full rows and one partial row
LADDER_AREAS = tuple(a for a, _ in LADDER)
ZERO_MEDIAN_AREA = 257
LADDER_FRAME = (144, 280)
SPARSE_BOX = {64: None, 128: 90, 256: 100}


def as_unit_float(px):
    """uint16 -> float32 in [0, 1]; equal values stay equal, 0 stays 0."""
    return (px.astype(np.float64) / 65535.0).astype(np.float32)


def _with_duplicates(values, zero_median=False, extremes=False):
    """The values of one object, rearranged: the three middle order statistics equal, the two largest equal, and the fifth and sixth
    largest equal (a duplicate across the top-five boundary)."""
    s = np.sort(values)
    n = len(s)
    if n >= 16:
        s[n // 2 - 1] = s[n // 2 + 1] = s[n // 2]
        s[n - 2] = s[n - 1]
        s[n - 6] = s[n - 5]
    if zero_median:
        s[: n // 2 + 12] = 0
    if extremes:
        s[0], s[-2], s[-1] = 0, 65535, 65535
    return s


def area_ladder(block, dtype="u16"):
    """-> (labels [1, Y, X], planes [1, 1, Y, X], areas of labels 1..16).  Label 17 (block 128 / 256) is a diagonal band."""
    Y, X = LADDER_FRAME
    lab = np.zeros((Y, X), np.uint16)
    x, y, shelf = 104, 1, 0
    for k, (area, w) in enumerate(LADDER):
        h = -(-area // w)
        if x + w + 1 > X:
            x, y, shelf = 104, y + shelf + 2, 0
        m = np.zeros(h * w, bool)
        m[:area] = True
        lab[y:y + h, x:x + w][m.reshape(h, w)] = k + 1
        x, shelf = x + w + 2, max(shelf, h)
    assert y + shelf < Y
    side = SPARSE_BOX[block]
    if side:
        rr, cc = np.mgrid[:side, :side]
        lab[2:2 + side, 2:2 + side][np.abs(rr - cc) <= 4] = len(LADDER) + 1
    rng = np.random.default_rng(2025)
    px = rng.integers(0, 65536, size=(Y, X)).astype(np.uint16)
    for k, (area, _) in enumerate(LADDER):
        sel = lab == k + 1
        vals = _with_duplicates(px[sel], zero_median=area == ZERO_MEDIAN_AREA, extremes=area == 2048)
        px[sel] = vals[rng.permutation(area)]
    planes = px[None, None]
    return lab[None], (planes if dtype == "u16" else as_unit_float(planes)), LADDER_AREAS


def _pixels(seed, shape, dtype):
    px = np.random.default_rng(seed).integers(0, 65536, size=shape).astype(np.uint16)
    return px if dtype == "u16" else as_unit_float(px)


def _band(side, half):
    rr, cc = np.mgrid[:side, :side]
    return np.abs(rr - cc) <= half


def global_scratch_case(dtype="u16"):
    """A band in a 128 x 128 box (label 1), the tallest object (2), the widest (3) and the largest (4): max_h, max_w and max_area
    come from three objects, none of them the band.  -> (labels [1, Y, X], planes [1, 2, Y, X], channel)."""
    lab = np.zeros((162, 212), np.uint16)
    lab[:128, :128][_band(128, 7)] = 1
    lab[2:152, 134:138] = 2
    lab[155:159, 1:151] = 3
    lab[10:58, 150:198] = 4
    lab[70:73, 150:153] = 5
    return lab[None], _pixels(7, (1, 2) + lab.shape, dtype), 1


def global_stride_case(dtype="u16"):
    """The band, and 620 objects of 3 x 3 to 5 x 5 pixels on a 6-pixel grid beside it: more objects than the 512 workgroups of
    the global form.  -> (labels [1, Y, X], planes [1, 1, Y, X], channel)."""
    lab = np.zeros((160, 640), np.uint16)
    lab[:128, :128][_band(128, 7)] = 1
    rng = np.random.default_rng(11)
    k = 1
    for gx in range(132, 640 - 6, 6):
        for gy in range(1, 160 - 6, 6):
            if k > 620:
                break
            k += 1
            h, w = rng.integers(3, 6, size=2)
            lab[gy:gy + h, gx:gx + w] = k
    assert k == 621
    return lab[None], _pixels(13, (1, 1) + lab.shape, dtype), 0


def sparse_ids_case(dtype="u16"):
    """Labels 1, 4 and 9 of 1..9: a cross that touches all four frame borders, one pixel, and a 2 x 2 block."""
    lab = np.zeros((24, 31), np.uint16)
    lab[10:13, :] = 1
    lab[:, 14:17] = 1
    lab[3, 5] = 4
    lab[18:20, 24:26] = 9
    return lab[None], _pixels(17, (1, 1) + lab.shape, dtype), 0


def two_tile_batch(dtype="u16"):
    """Two tiles, three channels, channel 2 read; the second tile is empty.  -> (labels [2, Y, X], planes [2, 3, Y, X], channel)."""
    lab = np.zeros((2, 40, 52), np.uint16)
    yy, xx = np.mgrid[:40, :52]
    lab[0][((yy - 14) / 8.6) ** 2 + ((xx - 16) / 12.3) ** 2 <= 1.0] = 1
    lab[0, 28:37, 30:49] = 2
    lab[0, 2:9, 40:47] = 3
    lab[0, 30:33, 3:12] = 4
    return lab, _pixels(19, (2, 3, 40, 52), dtype), 2


def _signed_floats(rng, shape):
    """float32 in [-1, 1] without zeros, every value present several times."""
    pool = rng.uniform(0.05, 1.0, size=97).astype(np.float32) * rng.choice(np.float32([-1, 1]), size=97)
    return pool[rng.integers(0, len(pool), size=shape)]


RATIO_OBJECTS = {1: "1 pixel", 2: "2 pixels", 3: "35 pixels", 4: "36 pixels", 5: "20 pixels, one zero in channel 2",
                 6: "21 pixels, one zero in channel 0", 7: "45 pixels"}


def ratio_case(dtype="u16"):
    """Seven objects (RATIO_OBJECTS), three channels.  dtype "u16", "f32" ([0, 1]) or "f32_signed" (negative values, duplicates, a
    -0.0 as the zero of object 5, +0.0 and -0.0 among the numerators of object 7).  -> (labels [1, Y, X], planes [1, 3, Y, X])."""
    lab = np.zeros((30, 44), np.uint16)
    lab[1, 1] = 1
    lab[1, 4:6] = 2
    lab[4:9, 2:9] = 3
    lab[4:10, 12:18] = 4
    lab[12:16, 2:7] = 5
    lab[12:15, 10:17] = 6
    lab[18:27, 3:8] = 7
    rng = np.random.default_rng(23)
    shape = (1, 3) + lab.shape
    if dtype == "f32_signed":
        px = _signed_floats(rng, shape)
    else:
        px = rng.integers(1, 65536, size=shape).astype(np.uint16)
        if dtype == "f32":
            px = as_unit_float(px)
    zero = np.float32(-0.0) if dtype == "f32_signed" else 0
    px[0, 2, 13, 4] = zero
    px[0, 0, 13, 12] = 0
    if dtype == "f32_signed":
        px[0, 0, 19, 4], px[0, 0, 22, 6] = np.float32(0.0), np.float32(-0.0)
        px[0, 2, 19, 4], px[0, 2, 22, 6] = np.float32(0.5), np.float32(0.5)
    return lab[None], px


def ratio_limit_case():
    """One object of exactly 16384 pixels (the most the kernel sorts in LDS) and a small one."""
    lab = np.zeros((130, 136), np.uint16)
    lab[1:129, 1:129] = 1
    lab[3:6, 131:134] = 2
    px = np.random.default_rng(29).integers(1, 65536, size=(1, 2) + lab.shape).astype(np.uint16)
    return lab[None], px


TRAP_BACKGROUND_COUNTS = (0, 1, 4, 5, 6, 40, 77)


def trap_case(dtype="u16"):
    """Seven tiles of 12 x 13 pixels with TRAP_BACKGROUND_COUNTS pixels under no label, two channels, channel 1 read; duplicates at
    the median and among the five largest.  "f32_signed": ten negatives, -0.0 and +0.0 below a positive median.
    -> (labels [7, Y, X], planes [7, 2, Y, X], channel)."""
    F, Y, X = len(TRAP_BACKGROUND_COUNTS), 12, 13
    rng = np.random.default_rng(31)
    lab = np.empty((F, Y, X), np.uint16)
    if dtype == "f32_signed":
        px = _signed_floats(rng, (F, 2, Y, X))
    else:
        px = rng.integers(0, 65536, size=(F, 2, Y, X)).astype(np.uint16)
    for f, k in enumerate(TRAP_BACKGROUND_COUNTS):
        flat = np.full(Y * X, 1 + f % 3, np.uint16)
        where = rng.permutation(Y * X)[:k]
        flat[where] = 0
        lab[f] = flat.reshape(Y, X)
        if k >= 40:
            if dtype == "f32_signed":
                vals = np.sort(np.abs(px[f, 1].ravel()[where]))
                vals[:10] *= -1
                vals[10], vals[11], vals[12] = -0.0, 0.0, 0.0
            else:
                vals = np.sort(px[f, 1].ravel()[where])
            vals[k // 2 - 1] = vals[k // 2 + 1] = vals[k // 2]
            vals[k - 2] = vals[k - 1]
            vals[k - 6] = vals[k - 5]
            px[f, 1].reshape(-1)[where] = vals[rng.permutation(k)]
        elif k >= 4 and dtype != "f32_signed":
            px[f, 1].reshape(-1)[where[:2]] = 65535  # the largest value, twice
    if dtype == "f32":
        px = as_unit_float(px)
    return lab, px, 1


_BUILDERS = {
    "ladder64": lambda d: area_ladder(64, d)[:2] + (0,),
    "ladder128": lambda d: area_ladder(128, d)[:2] + (0,),
    "ladder256": lambda d: area_ladder(256, d)[:2] + (0,),
    "global_scratch": global_scratch_case,
    "global_stride": global_stride_case,
    "sparse_ids": sparse_ids_case,
    "two_tiles": two_tile_batch,
}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name, dtype="u16"):
    """One input and its reference, computed once per process and read-only: dict(labels, planes, channel, counts, want, meta)."""
    labels, planes, channel = _BUILDERS[name](dtype)
    counts = [int(t.max()) for t in labels]
    want, meta = cell_metrics_batch(labels, planes, channel, counts)
    for a in (labels, planes, want):
        a.setflags(write=False)
    return dict(labels=labels, planes=planes, channel=channel, counts=counts, want=want, meta=meta)
