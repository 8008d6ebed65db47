"""
Exact reference of the 21 columns of `FeatureEngine.intensity` (aliby_amd/csrc/feat_intensity.hip, k_intensity) and the rule its
results are compared by.  tests/test_cpu_intensity_ref.py pins this file to oracle/cp_measure_restated.get_intensity and to
hand-computed rows.

A per-object restatement written from the column definitions (CellProfiler's MeasureObjectIntensity, as the kernel's header
restates it), over Python integers and `fractions.Fraction`.  None of the oracle's code paths is used (no labelled sums of
scipy.ndimage, no lexsort).  A uint16 pixel is an `int`; a float32 pixel converts to a `Fraction` exactly.

  * Sums (Integrated, sum x v, sum y v, sum v^2, ...) are exact.
  * Mean and the centres of mass are `float(Fraction)`: the float64 nearest to the exact quotient.
  * The variance (N sum v^2 - (sum v)^2) / N^2 is an exact rational, rounded once, then `math.sqrt`.
  * Quartiles: with s the sorted values, index N q, qi its integer part and qf its fraction (0, .25, .5 or .75),
    s[qi] (1 - qf) + s[qi + 1] qf if qi < N - 1, else s[qi].  MAD: the same rule at q = 1/2 applied to the sorted |v - median|,
    where the median is the float64 the previous step returned.
  * Edge pixels: a pixel of the object with a 4-neighbour INSIDE THE FRAME that carries another label (0 included): skimage's
    find_boundaries(mode="inner", connectivity=1) replicates the border, so the frame itself is no boundary.  An object without
    an edge pixel has 0 in the five edge columns.
  * Location_MaxIntensity: the LAST raveled occurrence of the maximum.  scipy.ndimage.maximum_position, which CellProfiler calls,
    sorts unstably, so which of several maxima it returns is implementation-defined; the oracle documents the last one as its
    choice, the kernel follows it, and so does this file.  Z is 0.
  * Location_CenterMassIntensity_Z is 0 * S / S with S the integrated intensity: 0 for a plane, and NaN, like X and Y, when S = 0.
  * MassDisplacement: the distance between the centre of the pixels and the intensity-weighted centre, from the exact rationals.
  * A label without pixels has NaN in every column.

The comparison rule (`check`)
-----------------------------
Bit-equal columns, uint16 pixels: Integrated, Mean, Min, Max and the same four on the edge, the quartiles, the median, the MAD,
CenterMassIntensity_X/Y/Z and MaxIntensity_X/Y/Z.  Every sum is an integer below 2^53 (at most 2^10 pixels of 20 x 20 objects,
values below 2^16, coordinates below 2^7: sum x v < 2^33), so a float64 accumulation of it is exact in any order, and every
quotient of two such sums is, by IEEE division, the correctly rounded value of an exact rational, which is what `float(Fraction)`
returns.  An interpolated quartile of integers with weights that are multiples of 1/4 is exact.  (The bound on the sums is
asserted per object: `meta["small"]`.)

Bit-equal columns, float32 pixels: the same without the sums and quotients of sums (Integrated, Mean, their edge versions,
CenterMassIntensity_X/Y).  A quartile is the sum of two products that are each exact in float64 (24 x 2 bits), so it is
correctly rounded however it is evaluated, with or without a fused multiply-add.  The MAD is bit-equal where every |v - median|
and the interpolated result are float64 numbers (`meta["mad_exact"]`, worked out per object; true for unit floats of uint16
pixels, whose exponents span 16 bits); elsewhere it goes by the relative bound.

Std and StdEdge: relative 1e-12, and exactly 0.0 on a flat object.  The kernel is two-pass: N <= 2^10 non-negative terms
(v - mean)^2, each with a relative error of about 3 * 2^-53 (one rounding of the difference, whose operand `mean` is itself
within 2^-53, entering in second order only since the deviations sum to zero; one of the square), summed with at most 10 more
roundings in a tree or 2^10 in a chain: below 2^10 * 2^-53 + 3 * 2^-53 < 2e-13 relative in the sum, half of that after the root,
plus the division and the root: below 4e-13.  On a flat object the sum N v is exact (34 bits for float32, 26 for uint16), the
mean is v itself and every deviation is exactly 0.

float32 sums, means and centres: relative 1e-12.  Up to 2^10 non-negative terms, each exact (a float32, or a float32 times an
integer below 2^7), summed in float64: below 2^10 * 2^-53 = 1.2e-13 relative; a quotient of two such sums below 2.4e-13.

MassDisplacement: exactly 0.0 wherever the exact displacement is 0 (both centres are then the correctly rounded value of the
same rational: a flat or saturated object); otherwise absolute.  Coordinates are below 2^7.  uint16: each of the four quotients is
within half an ulp of 2^7, 1.4e-14; the two differences and the root add as much again: below 6e-14, bound 1e-12.  float32: each
intensity-weighted centre is a quotient of two sums within 1.2e-13 relative each, so within 2.4e-13 * 2^7 = 3.1e-11 absolute;
two of them under the root: below 4.4e-11, bound 1e-9.  Where the exact displacement is d > 0 but tiny, the absolute error of
sqrt(dx^2 + dy^2) is still that of dx and dy (|sqrt(a^2 + b^2) - sqrt(c^2 + d^2)| <= |(a, b) - (c, d)|), so the bound holds.
"""
import math
from fractions import Fraction

import numpy as np

CORE = ["Intensity_IntegratedIntensity", "Intensity_MeanIntensity", "Intensity_StdIntensity", "Intensity_MinIntensity",
        "Intensity_MaxIntensity"]
EDGE = ["Intensity_IntegratedIntensityEdge", "Intensity_MeanIntensityEdge", "Intensity_StdIntensityEdge", "Intensity_MinIntensityEdge",
        "Intensity_MaxIntensityEdge"]
TAIL = ["Intensity_MassDisplacement", "Intensity_LowerQuartileIntensity", "Intensity_MedianIntensity", "Intensity_MADIntensity",
        "Intensity_UpperQuartileIntensity", "Location_CenterMassIntensity_X", "Location_CenterMassIntensity_Y",
        "Location_CenterMassIntensity_Z", "Location_MaxIntensity_X", "Location_MaxIntensity_Y", "Location_MaxIntensity_Z"]
SUM_COLUMNS = ("Intensity_IntegratedIntensity", "Intensity_MeanIntensity", "Intensity_IntegratedIntensityEdge", "Intensity_MeanIntensityEdge",
               "Location_CenterMassIntensity_X", "Location_CenterMassIntensity_Y")
STD_COLUMNS = ("Intensity_StdIntensity", "Intensity_StdIntensityEdge")
DISPLACEMENT = "Intensity_MassDisplacement"
MAD = "Intensity_MADIntensity"
RTOL = 1e-12
DISPLACEMENT_ATOL = {"u16": 1e-12, "f32": 1e-9}
TWO53 = 1 << 53


def names(edge=True):
    return CORE + (EDGE if edge else []) + TAIL


def exact_columns(mode, edge=True):
    """The columns compared bit for bit (the MAD of float32 pixels only in rows whose meta says `mad_exact`)."""
    loose = set(STD_COLUMNS) | {DISPLACEMENT} | (set(SUM_COLUMNS) if mode == "f32" else set())
    return [n for n in names(edge) if n not in loose]


def _exact(v):
    """A pixel as an exact number: int for an integer type, Fraction for a float type."""
    return int(v) if isinstance(v, (int, np.integer)) else Fraction(float(v))


def _is_float64(q) -> bool:
    return Fraction(float(q)) == q


def quantile(s, q):
    """CellProfiler's rule on the sorted list s, exact: -> Fraction"""
    n = len(s)
    pos = Fraction(n) * q
    qi = int(pos)
    qf = pos - qi
    if qi < n - 1:
        return Fraction(s[qi]) * (1 - qf) + Fraction(s[qi + 1]) * qf
    return Fraction(s[qi])


def _moments(vals):
    """-> (count, exact sum, float mean, float std, float min, float max) of a non-empty list of exact numbers"""
    n, s, s2 = len(vals), sum(vals), sum(v * v for v in vals)
    return n, s, float(Fraction(s, n)), math.sqrt(float(Fraction(n * s2 - s * s, n * n))), float(min(vals)), float(max(vals))


def one_object(labels, pixels, label, edge=True):
    """labels [Y, X], pixels [Y, X] -> ({column: float}, meta) of one label value."""
    Y, X = labels.shape
    cols = dict.fromkeys(names(edge), math.nan)
    pts = [(int(y), int(x)) for y, x in zip(*np.nonzero(labels == label))]  # raster order
    meta = dict(n=len(pts), flat=False, flat_edge=False, dark=False, displacement_zero=False, mad_exact=True, small=True, n_edge=0)
    if not pts:
        return cols, meta
    vals = [_exact(pixels[p]) for p in pts]
    n, s, mean, std, vmin, vmax = _moments(vals)
    cols["Intensity_IntegratedIntensity"] = float(s)
    cols["Intensity_MeanIntensity"], cols["Intensity_StdIntensity"] = mean, std
    cols["Intensity_MinIntensity"], cols["Intensity_MaxIntensity"] = vmin, vmax
    meta["flat"] = min(vals) == max(vals)
    meta["dark"] = s == 0
    if edge:
        def on_edge(y, x):
            return any(0 <= y + dy < Y and 0 <= x + dx < X and labels[y + dy, x + dx] != label for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))

        evals = [v for (y, x), v in zip(pts, vals) if on_edge(y, x)]
        meta["n_edge"] = len(evals)
        if evals:
            _, es, emean, estd, emin, emax = _moments(evals)
            for k, v in zip(EDGE, (float(es), emean, estd, emin, emax)):
                cols[k] = v
            meta["flat_edge"] = min(evals) == max(evals)
        else:
            for k in EDGE:
                cols[k] = 0.0
            meta["flat_edge"] = True
    sx, sy = sum(x for _, x in pts), sum(y for y, _ in pts)
    sxv, syv = sum(x * v for (_, x), v in zip(pts, vals)), sum(y * v for (y, _), v in zip(pts, vals))
    meta["small"] = all(t < TWO53 for t in (s, sxv, syv) if isinstance(t, int))  # (integer pixels: the exactness argument)
    if s != 0:
        cmi_x, cmi_y = Fraction(sxv) / s, Fraction(syv) / s
        dx, dy = Fraction(sx, n) - cmi_x, Fraction(sy, n) - cmi_y
        cols["Location_CenterMassIntensity_X"], cols["Location_CenterMassIntensity_Y"] = float(cmi_x), float(cmi_y)
        cols["Location_CenterMassIntensity_Z"] = 0.0  # 0 * S / S
        cols[DISPLACEMENT] = math.sqrt(float(dx * dx + dy * dy))
        meta["displacement_zero"] = dx == 0 and dy == 0
    srt = sorted(vals)
    cols["Intensity_LowerQuartileIntensity"] = float(quantile(srt, Fraction(1, 4)))
    cols["Intensity_UpperQuartileIntensity"] = float(quantile(srt, Fraction(3, 4)))
    median = float(quantile(srt, Fraction(1, 2)))
    cols["Intensity_MedianIntensity"] = median
    dev = sorted(abs(Fraction(v) - Fraction(median)) for v in vals)
    mad = quantile(dev, Fraction(1, 2))
    cols[MAD] = float(mad)
    meta["mad_exact"] = _is_float64(mad) and all(_is_float64(d) for d in dev)
    top = max(vals)
    ymax, xmax = [p for p, v in zip(pts, vals) if v == top][-1]  # the last raveled occurrence
    cols["Location_MaxIntensity_X"], cols["Location_MaxIntensity_Y"], cols["Location_MaxIntensity_Z"] = float(xmax), float(ymax), 0.0
    return cols, meta


def intensity(labels, pixels, n=None, edge=True):
    """labels [Y, X] with values 0..n, pixels [Y, X] -> (float64 [n, 21 or 16] in `names(edge)` order, row = label - 1; one meta
    dict per row)."""
    labels, pixels = np.asarray(labels), np.asarray(pixels)
    assert labels.ndim == 2 and pixels.shape == labels.shape
    n = int(labels.max(initial=0)) if n is None else int(n)
    order = names(edge)
    rows, metas = np.full((n, len(order)), np.nan), []
    for k in range(n):
        cols, meta = one_object(labels, pixels, k + 1, edge)
        rows[k] = [cols[c] for c in order]
        metas.append(meta)
    return rows, metas


def intensity_batch(labels, pixels, channel, counts, edge=True):
    """labels [F, Y, X], pixels [F, C, Y, X] -> (float64 [sum counts, ncol], metas), tile after tile."""
    rows, metas = [np.zeros((0, len(names(edge))))], []
    for f, c in enumerate(counts):
        r, m = intensity(labels[f], pixels[f][channel], c, edge)
        rows.append(r)
        metas += m
    return np.concatenate(rows), metas


def _relative(g, w):
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(g - w) / np.abs(w)
    return np.where(g == w, 0.0, rel)


def check(got, want, meta, tag, mode, edge=True):
    """The comparison rule of the module docstring.  got, want: [rows, 21 or 16]; meta: one dict per row (from `intensity`).
    Prints the worst error of each column that is not compared bit for bit."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got, float)
    order = names(edge)
    assert got.shape == want.shape == (len(meta), len(order)), (tag, got.shape, want.shape, len(meta))
    assert all(m["small"] for m in meta), (tag, "a sum of 2^53 or more: the exactness argument does not hold")
    objects = lambda rows: [(int(r), meta[r]["n"], "all pixels 0" if meta[r]["dark"] else "") for r in rows]  # noqa: E731
    for j, name in enumerate(order):
        g, w = got[:, j], want[:, j]
        nan = np.isnan(g) != np.isnan(w)
        assert not nan.any(), (tag, name, "NaN against a number in rows (row, area, note)", objects(np.flatnonzero(nan)), g[nan], w[nan])
    present = np.asarray([m["n"] > 0 for m in meta], bool)
    exact = exact_columns(mode, edge)
    worst = {}
    for j, name in enumerate(order):
        g, w = got[:, j], want[:, j]
        ok = ~np.isnan(w)
        if name in exact:
            rows = ok & np.asarray([name != MAD or m["mad_exact"] for m in meta], bool)
            bad = rows & (g.view(np.uint64) != w.view(np.uint64))
            assert not bad.any(), (tag, name, "not the same bits in rows (row, area, note)", objects(np.flatnonzero(bad)), g[bad], w[bad])
            ok = ok & ~rows
            if not ok.any():
                continue
        if name == DISPLACEMENT:
            zero = ok & np.asarray([m["displacement_zero"] for m in meta], bool)
            assert (g[zero].view(np.uint64) == 0).all(), (tag, name, "not exactly 0.0 in rows", objects(np.flatnonzero(zero & (g != 0))), g[zero])
            worst[name] = float(np.abs(g[ok] - w[ok]).max(initial=0.0))
            assert worst[name] <= DISPLACEMENT_ATOL[mode], (tag, name, worst[name], g[ok], w[ok])
            continue
        if name in STD_COLUMNS:
            key = "flat" if name == "Intensity_StdIntensity" else "flat_edge"
            zero = ok & present & np.asarray([m[key] for m in meta], bool)
            assert (g[zero].view(np.uint64) == 0).all(), (tag, name, "std of a flat object is not exactly 0.0", objects(np.flatnonzero(zero & (g != 0))))
        rel = _relative(g[ok], w[ok])
        worst[name] = float(rel.max(initial=0.0))
        assert worst[name] <= RTOL, (tag, name, worst[name], objects(np.flatnonzero(ok)[rel > RTOL]), g[ok][rel > RTOL], w[ok][rel > RTOL])
    print(f"intensity {tag} ({mode}, {len(meta)} rows): worst error " + ", ".join(f"{k.split('_', 1)[1]} {v:.1e}" for k, v in worst.items()))
    return worst
