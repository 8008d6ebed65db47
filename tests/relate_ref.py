"""
CPU restatement of the `relate` family and of the tertiary image (aliby_amd/csrc/feat_relate.hip; the definition is in
include/aliby_hip.h): CellProfiler's RelateObjects and IdentifyTertiaryObjects.  PARITY with CellProfiler is UNPINNED: the definition
is recalled from CellProfiler 4's relateobjects.py and identifytertiaryobjects.py and centrosome's outline, and none of them can be
run here.  tests/test_cpu_relate_ref.py pins this file to hand values and to np.bincount / scipy.ndimage.  No product import.

Per tile, A and B are two label images of one shape [Y,X], 0 = background, labels 1..n_A and 1..n_B (a label may be absent).  Row L
of A relative to B (NAMES):
  Parent             the label p >= 1 of B that covers the most pixels of L, ties to the smallest p; 0 without one or when L is absent
  ParentOverlap      that pixel count; 0 without a parent
  Children count     the B objects whose Parent in A (same rule, roles swapped) is L
  Distance_Centroid  centres (sum y / area, sum x / area), exact integer sums and one float64 division each; dy = py - cy,
                     dx = px - cx, sqrt(dy dy + dx dx); NaN without a parent
  Distance_Minimum   min over the outline pixels (y, x) of the parent of (y - cy)^2 + (x - cx)^2, then one sqrt; NaN without a parent.
                     Outline: pixels on the first or last row or column of the tile, or with an 8-neighbour of another value.
Tertiary image: outer where inner == 0, or (shrink_inner) where the pixel is an outline pixel of its inner object; 0 elsewhere.

The pixels are grouped by label with one stable sort; every object is then a slice of the sorted arrays (no bounding boxes, no
histogram over label pairs).
"""
import numpy as np

STEMS = ("Parent_{}", "ParentOverlap_{}", "Children_{}_Count", "Distance_Centroid_{}", "Distance_Minimum_{}")
EXACT = (0, 1, 2)  # integer columns: bit-equal on the GPU
FLOAT = (3, 4)     # one sqrt of fewer than ten float64 operations: rtol = atol = 1e-12
RTOL = ATOL = 1e-12


def names(other):
    return [s.format(other) for s in STEMS]


def outline(lab):
    """bool [Y,X]: the outline pixels of every object.  The frame is padded with a value no label has, so a pixel on the first or last
    row or column always has an 8-neighbour of another value."""
    lab = np.asarray(lab).astype(np.int64)
    Y, X = lab.shape
    pad = np.full((Y + 2, X + 2), -1, np.int64)
    pad[1:-1, 1:-1] = lab
    edge = np.zeros(lab.shape, bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                edge |= pad[dy:dy + Y, dx:dx + X] != lab
    return edge & (lab > 0)


def _groups(lab, n, mask=None):
    """{label: (ys, xs)} of the pixels of labels 1..n (of those under `mask`), by one stable sort."""
    lab = np.asarray(lab).astype(np.int64)
    keep = (lab > 0) & (lab <= n)
    if mask is not None:
        keep &= mask
    ys, xs = np.nonzero(keep)
    v = lab[ys, xs]
    order = np.argsort(v, kind="stable")
    ys, xs, v = ys[order], xs[order], v[order]
    cuts = np.flatnonzero(np.diff(v)) + 1
    starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts, [len(v)]])
    return {int(v[s]): (ys[s:e], xs[s:e]) for s, e in zip(starts, ends) if e > s}


def centres(lab, n):
    """float64 [n, 2] (y, x), NaN for a label without pixels."""
    c = np.full((n, 2), np.nan)
    for L, (ys, xs) in _groups(lab, n).items():
        c[L - 1] = (np.float64(int(ys.sum())) / np.float64(len(ys)), np.float64(int(xs.sum())) / np.float64(len(xs)))
    return c


def parents(a, b, na, nb):
    """(parent [na], overlap [na]) int64 of A's labels in B."""
    b = np.asarray(b).astype(np.int64)
    parent, overlap = np.zeros(na, np.int64), np.zeros(na, np.int64)
    for L, (ys, xs) in _groups(a, na).items():
        under = b[ys, xs]
        under = under[(under > 0) & (under <= nb)]
        if under.size:
            labels, counts = np.unique(under, return_counts=True)  # ascending labels: argmax takes the smallest on a tie
            k = int(np.argmax(counts))
            parent[L - 1], overlap[L - 1] = labels[k], counts[k]
    return parent, overlap


def relate(a, b, na=None, nb=None):
    """Two label images [Y,X] -> (rows of A relative to B [na, 5], rows of B relative to A [nb, 5]), float64."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert a.shape == b.shape
    na = int(a.max()) if na is None else na
    nb = int(b.max()) if nb is None else nb
    pa_, oa = parents(a, b, na, nb)
    pb_, ob = parents(b, a, nb, na)
    ca, cb = centres(a, na), centres(b, nb)
    return (_rows(na, pa_, oa, pb_, ca, cb, _groups(b, nb, outline(b))),
            _rows(nb, pb_, ob, pa_, cb, ca, _groups(a, na, outline(a))))


def _rows(n, parent, overlap, parent_of_other, centre, centre_other, outline_other):
    out = np.full((n, 5), np.nan)
    out[:, 0], out[:, 1] = parent, overlap
    out[:, 2] = np.bincount(parent_of_other[parent_of_other > 0], minlength=n + 1)[1:n + 1]
    for row in range(n):
        p = int(parent[row])
        if p == 0:
            continue
        cy, cx = centre[row]
        dy, dx = centre_other[p - 1, 0] - cy, centre_other[p - 1, 1] - cx
        out[row, 3] = np.sqrt(dy * dy + dx * dx)
        ys, xs = outline_other[p]
        ey, ex = ys.astype(np.float64) - cy, xs.astype(np.float64) - cx
        out[row, 4] = np.sqrt((ey * ey + ex * ex).min())
    return out


def tertiary(outer, inner, shrink_inner=True):
    outer, inner = np.asarray(outer), np.asarray(inner)
    keep = inner == 0
    if shrink_inner:
        keep |= outline(inner)
    return np.where(keep, outer, 0).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ scenes: (A, B[, n_A, n_B])
def worked():
    """The header's example: a 6 x 8 tile, two cells side by side, three nuclei."""
    b = np.zeros((6, 8), np.uint16)
    b[:, :4], b[:, 4:] = 1, 2
    a = np.zeros((6, 8), np.uint16)
    a[1:3, 1:3] = 1
    a[3:5, 3:5] = 2
    a[0, 6:8] = 3
    return a, b


S = np.sqrt
WORKED_NUCLEI = np.array([[1, 4, 1, 1.0, S(2.5)], [1, 2, 1, S(5.0), S(0.5)], [2, 2, 0, S(7.25), 0.5]])
WORKED_CELLS = np.array([[1, 4, 2], [2, 2, 1]], float)  # (first three columns)
WORKED_TERTIARY_AREAS = {False: (18, 20), True: (24, 24)}


def strip():
    """Child 1 is a 1 x 300 strip crossing 257 single-column parents (labels descending from the left, so the smallest is met last) and
    two 21-wide parents that tie at 21 pixels; child 2 covers the single-column parents only: 257 ties at one pixel."""
    b = np.zeros((5, 300), np.uint16)
    for x in range(257):
        b[:, x] = 257 - x
    b[:, 257:278], b[:, 278:299] = 259, 258
    a = np.zeros((5, 300), np.uint16)
    a[1, :] = 1
    a[3, :257] = 2
    return a, b


def scenes():
    """{name: (A, B, n_A, n_B)}: small tiles, every one another way for the kernels to go wrong."""
    out = {}
    a, b = worked()
    out["worked"] = (a, b, 3, 2)
    # a child without a parent, beside one with
    a, b = np.zeros((9, 11), np.uint16), np.zeros((9, 11), np.uint16)
    b[1:5, 1:6] = 1
    a[2:4, 2:4] = 1
    a[6:8, 7:10] = 2
    out["orphan"] = (a, b, 2, 1)
    # a child whose box contains other children: an L around two small ones, over three parents
    a, b = np.zeros((17, 19), np.uint16), np.zeros((17, 19), np.uint16)
    a[2:15, 2] = 1
    a[14, 2:16] = 1
    a[4:7, 5:9] = 2
    a[8:11, 10:13] = 3
    b[0:9, 0:10], b[9:17, 0:10], b[3:12, 10:19] = 1, 2, 3
    out["nested"] = (a, b, 3, 3)
    # absent labels in both sets, the last label included (the tables are longer than the largest label)
    a, b = np.zeros((12, 13), np.uint16), np.zeros((12, 13), np.uint16)
    a[1:4, 1:4], a[6:9, 6:11] = 1, 3
    b[0:6, 0:7], b[5:11, 5:12] = 2, 4
    out["absent"] = (a, b, 5, 6)
    # objects on all four frame borders, in both sets
    a, b = np.zeros((10, 12), np.uint16), np.zeros((10, 12), np.uint16)
    b[0:5, 0:6], b[0:5, 6:12], b[5:10, 0:6], b[5:10, 6:12] = 1, 2, 3, 4
    a[0, 2:5], a[3:7, 11], a[9, 4:9], a[2:8, 0], a[4:6, 5:7] = 1, 2, 3, 4, 5
    out["borders"] = (a, b, 5, 4)
    return out


def batch3():
    """F = 3 with differing counts: a populated tile, a tile of zeros in both sets, a tile whose B set has no object."""
    a0, b0 = worked()
    pad = lambda t: np.pad(t, ((0, 3), (0, 3)))  # noqa: E731
    a2 = np.zeros((9, 11), np.uint16)
    a2[2:5, 3:8], a2[6:8, 1:4] = 1, 2
    tiles_a = [pad(a0), np.zeros((9, 11), np.uint16), a2]
    tiles_b = [pad(b0), np.zeros((9, 11), np.uint16), np.zeros((9, 11), np.uint16)]
    return tiles_a, tiles_b, [3, 0, 2], [2, 0, 0]


def single_pixel_parents():
    """A 256 x 256 tile whose first 65 534 pixels are one parent each (labels in raster order), with four children; and the same
    children over only the parents they touch, relabelled 1..k in ascending order (ties keep their order).  Returns
    (A, B_many, B_few, old label of every new one)."""
    b = np.zeros(256 * 256, np.int64)
    b[:65534] = np.arange(1, 65535)
    b = b.reshape(256, 256).astype(np.uint16)
    a = np.zeros((256, 256), np.uint16)
    a[10:14, 20:27], a[100:103, 5:8], a[200, 30:95], a[254:256, 250:256] = 1, 2, 3, 4  # (child 4 meets the two pixels without a parent)
    old = np.unique(b[a > 0])
    old = old[old > 0]
    few = np.zeros_like(b)
    under = (a > 0) & (b > 0)
    few[under] = (np.searchsorted(old, b[under]) + 1).astype(np.uint16)
    return a, b, few, old.astype(np.int64)


def tertiary_scenes():
    """{name: (outer, inner)}: the worked example, a 3 x 3 nucleus (loses exactly its interior pixel), a cell under a large nucleus (left
    empty), widths that are and are not multiples of eight, a nucleus across two cells and on the frame."""
    out = {}
    a, b = worked()
    out["worked"] = (b, a)
    outer, inner = np.zeros((9, 16), np.uint16), np.zeros((9, 16), np.uint16)
    outer[1:8, 1:8], outer[2:5, 10:13] = 1, 2
    inner[3:6, 3:6], inner[0:8, 8:16] = 1, 2
    out["three_by_three_w16"] = (outer, inner)
    outer, inner = np.zeros((11, 13), np.uint16), np.zeros((11, 13), np.uint16)
    outer[0:11, 0:6], outer[0:11, 6:13], outer[4:7, 8:11] = 1, 2, 3
    inner[2:9, 3:10], inner[0:3, 10:13] = 1, 2
    out["across_w13"] = (outer, inner)
    return out
