"""
CPU restatement of the `neighbors` family (aliby_amd/csrc/feat_neighbors.hip; the definition is in include/aliby_hip.h):
CellProfiler's MeasureObjectNeighbors with the objects as their own neighbours.  PARITY with cp_measure / CellProfiler is UNPINNED:
the definition is recalled from CellProfiler 4's measureobjectneighbors.py and centrosome's outline / strel_disk, and neither can be
run here.  tests/test_cpu_neighbors_ref.py pins this file to hand values and to scipy.ndimage.

Direct loops over the definition: every offset of the disc T is visited once and the label image is compared with itself shifted by
that offset, over the part of the frame where both ends exist (offsets that leave the frame are dropped).  No dilation routine.

  S = {dy^2 + dx^2 <= d^2}, T = {dy^2 + dx^2 <= d^2 + d}; the outline of L = its pixels on the frame's first / last row or column, or
  with one of the 8 neighbours carrying another value.  Columns (NAMES): the number of distinct foreign labels reached from L's
  pixels through S; 100 t / p with p the outline pixels and t those that reach a foreign label through T; label and centre distance
  of the closest and second closest present object (lower key dy dy + dx dx, then lower label; 0 where there is none); the angle
  atan2(|v1 x v2|, v1 . v2) in degrees between the two (NaN for a zero vector, 0 without a second).  A label without pixels: NaN.
"""
import math

import numpy as np

STEMS = ("NumberOfNeighbors", "PercentTouching", "FirstClosestObjectNumber", "FirstClosestDistance", "SecondClosestObjectNumber",
         "SecondClosestDistance", "AngleBetweenNeighbors")
EXACT = (0, 1, 2, 4)  # columns that are integers or ratios of integers: bit-equal on the GPU
DISTANCES = (None, 2, 5, 9)


def names(distance=None):
    s = "Adjacent" if distance is None else str(distance)
    return [f"Neighbors_{stem}_{s}" for stem in STEMS]


def disc(d, half=False):
    """Offsets (dy, dx) with dy^2 + dx^2 <= d^2 (+ d when `half`: strel_disk(d + 0.5))."""
    r2 = d * d + (d if half else 0)
    return [(dy, dx) for dy in range(-d, d + 1) for dx in range(-d, d + 1) if dy * dy + dx * dx <= r2]


def _shifted(lab, dy, dx):
    """(labels at q, labels at q + (dy, dx), slices of q) over the q for which q + (dy, dx) is inside the frame."""
    Y, X = lab.shape
    y0, y1, x0, x1 = max(0, -dy), max(min(Y, Y - dy), max(0, -dy)), max(0, -dx), max(min(X, X - dx), max(0, -dx))  # (empty when |dy| >= Y)
    ys, xs = slice(y0, y1), slice(x0, x1)
    yo, xo = slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx)
    return lab[ys, xs], lab[yo, xo], (ys, xs)


def outline(lab):
    """bool [Y,X]: the outline pixels of every object."""
    lab = np.asarray(lab).astype(np.int64)
    out = np.zeros(lab.shape, bool)
    out[0, :] = out[-1, :] = out[:, 0] = out[:, -1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                a, b, q = _shifted(lab, dy, dx)
                out[q] |= a != b
    return out & (lab > 0)


def centres(lab, n):
    """float64 [n, 2] (y, x), NaN for a label without pixels: exact integer sums, one float64 division each."""
    lab = np.asarray(lab).astype(np.int64)
    c = np.full((n, 2), np.nan)
    yy, xx = np.nonzero(lab)
    v = lab[yy, xx]
    for L in np.unique(v):
        if L <= n:
            m = v == L
            area = int(m.sum())
            c[L - 1] = (np.float64(int(yy[m].sum())) / np.float64(area), np.float64(int(xx[m].sum())) / np.float64(area))
    return c


def neighbors(lab, n=None, distance=None):
    """Label image [Y,X] -> float64 [n, 7] (n: the rows, labels 1..n; default the largest label)."""
    lab = np.asarray(lab).astype(np.int64)
    n = int(lab.max()) if n is None else int(n)
    d = 1 if distance is None else int(distance)
    out = np.full((n, 7), np.nan)
    if n == 0:
        return out
    S = set(disc(d))
    reached = np.zeros(lab.shape, bool)  # the pixel reaches a foreign label through T
    pairs = set()  # (L, v): v reached from a pixel of L through S
    for dy, dx in disc(d, half=True):
        a, b, q = _shifted(lab, dy, dx)
        foreign = (a > 0) & (b > 0) & (a != b)
        reached[q] |= foreign
        if (dy, dx) in S and foreign.any():
            pairs.update(np.unique(a[foreign] * 65536 + b[foreign]).tolist())
    edge = outline(lab)
    present = [int(L) for L in np.unique(lab) if 0 < L <= n]
    count = {L: 0 for L in present}
    for code in pairs:
        L, v = divmod(code, 65536)
        if L in count and v <= n:
            count[L] += 1
    c = centres(lab, n)
    for L in present:
        mine = lab == L
        p, t = int((edge & mine).sum()), int((edge & mine & reached).sum())
        row = out[L - 1]
        row[0] = count[L]
        row[1] = np.float64(t) / np.float64(p) * 100.0
        row[2:] = 0.0
        ranked = []
        for v in present:
            if v != L:
                dy, dx = c[v - 1, 0] - c[L - 1, 0], c[v - 1, 1] - c[L - 1, 1]
                ranked.append((float(dy * dy + dx * dx), v, float(dy), float(dx)))
        ranked.sort(key=lambda r: (r[0], r[1]))
        if len(ranked) >= 1:
            row[2], row[3] = ranked[0][1], math.sqrt(ranked[0][0])
        if len(ranked) >= 2:
            row[4], row[5] = ranked[1][1], math.sqrt(ranked[1][0])
            (_, _, v1y, v1x), (_, _, v2y, v2x) = ranked[0], ranked[1]
            if ranked[0][0] == 0.0 or ranked[1][0] == 0.0:
                row[6] = np.nan
            else:
                row[6] = math.atan2(abs(v1x * v2y - v1y * v2x), v1x * v2x + v1y * v2y) * (180.0 / math.pi)
    return out


# ------------------------------------------------------------------------------------------------------------------------ scenes
def _disc_mask(shape, cy, cx, r_lo, r_hi):
    yy, xx = np.mgrid[: shape[0], : shape[1]]
    r2 = (yy - cy) ** 2 + (xx - cx) ** 2
    return (r2 >= r_lo * r_lo) & (r2 <= r_hi * r_hi)


def worked():
    """The worked case of the definition: A and B share an edge, B and C touch at a corner only."""
    lab = np.zeros((6, 8), np.uint16)
    lab[1:3, 1:3] = 1
    lab[1:3, 3:5] = 2
    lab[3:5, 5:7] = 3
    return lab


SMALL = (64, 64)


def small_scenes():
    """name -> uint16 [64,64] label image; the batch of tests/test_gpu_neighbors.py, in this order."""
    s = {}
    s["empty"] = np.zeros(SMALL, np.uint16)  # 0 objects
    one = np.zeros(SMALL, np.uint16)
    one[20:27, 30:41] = 1
    s["one"] = one  # 1 object: no candidate at all
    two = np.zeros(SMALL, np.uint16)
    two[10:14, 10:15] = 1
    two[16:21, 13:20] = 2  # 2 rows of background between them
    s["two"] = two  # 2 objects: a first candidate, no second
    ce = np.zeros(SMALL, np.uint16)  # all four corners and every edge
    ce[0:3, 0:3] = 1
    ce[0:4, 61:64] = 2
    ce[60:64, 0:2] = 3
    ce[61:64, 60:64] = 4
    ce[0:2, 28:36] = 5
    ce[62:64, 20:30] = 6
    ce[30:36, 0:3] = 7
    ce[25:40, 62:64] = 8
    ce[3:5, 3:6] = 9  # diagonal to the corner object
    s["corners_edges"] = ce
    sp = np.zeros(SMALL, np.uint16)
    sp[5, 5] = 1  # one pixel, beside a block
    sp[5:9, 6:10] = 2
    sp[40:44, 45:49] = 3  # farther than 9 from everything
    s["sparse"] = sp
    ring = np.zeros(SMALL, np.uint16)  # a disc inside a ring: coincident centres
    ring[_disc_mask(SMALL, 31, 31, 24, 28)] = 1
    ring[_disc_mask(SMALL, 31, 31, 0, 6)] = 2
    ring[0:2, 0:2] = 3  # a third object, so that the disc and the ring have a second candidate
    s["ring"] = ring
    cross = np.zeros(SMALL, np.uint16)  # four equal objects round a fifth: ties at every rank
    for L, (cy, cx) in zip((1, 2, 3, 4, 5), ((12, 32), (32, 12), (32, 32), (32, 52), (52, 32))):
        cross[cy - 1 : cy + 2, cx - 1 : cx + 2] = L
    s["cross"] = cross
    gaps = np.zeros(SMALL, np.uint16)  # labels 2, 5, 6 and 9 of 1..9
    gaps[4:10, 4:10] = 2
    gaps[4:10, 10:14] = 5
    gaps[10:15, 4:12] = 6
    gaps[40:50, 40:44] = 9
    s["gaps"] = gaps
    s["crowd"] = crowd()
    return s


def crowd(shape=SMALL):
    """A blob (label 1) ringed by more than 64 one-pixel objects whose labels 4, 7, 10, ... spread over a dozen bitmap words."""
    lab = np.zeros(shape, np.uint16)
    lab[_disc_mask(shape, 30, 30, 0, 8)] = 1
    ring = _disc_mask(shape, 30, 30, 9.5, 10.5) | _disc_mask(shape, 30, 30, 11.5, 12.5)
    ys, xs = np.nonzero(ring)
    assert len(ys) > 64
    lab[ys, xs] = 4 + 3 * np.arange(len(ys))
    return lab


def high_labels():
    """Two touching objects labelled 39 999 and 40 000: 40 000 rows, all but two absent."""
    lab = np.zeros(SMALL, np.uint16)
    lab[10:20, 10:20] = 39999
    lab[10:20, 20:26] = 40000
    return lab


BIG = (256, 256)


def big_scenes():
    """name -> uint16 [256,256]: one 200 x 200 object with a small one beside it, and the crowd of `crowd` in a corner."""
    big = np.zeros(BIG, np.uint16)
    big[20:220, 30:230] = 1
    big[222:226, 100:110] = 2
    return {"big": big, "crowd256": crowd(BIG)}


_EXPECTED = {}


def expected(key, lab, n=None, distance=None):
    """The restatement of a scene, computed once per (key, distance) and shared; callers must not write into it."""
    k = (key, distance)
    if k not in _EXPECTED:
        _EXPECTED[k] = neighbors(lab, n=n, distance=distance)
        _EXPECTED[k].setflags(write=False)
    return _EXPECTED[k]
