"""
CPU restatement of the `relate3d` family and of the tertiary volume (aliby_amd/csrc/feat_relate3d.hip; the definition is in
include/aliby_hip.h): CellProfiler's RelateObjects and IdentifyTertiaryObjects on volume labels.  PARITY with CellProfiler is UNPINNED:
the definition is recalled from CellProfiler 4's relateobjects.py and identifytertiaryobjects.py and centrosome's outline, and none of
them can be run here.  tests/test_cpu_relate3d_ref.py pins this file to hand values, to np.bincount / scipy.ndimage and, on stacks of
one plane, to tests/relate_ref.py.  No product import.

Per stack, A and B are two label volumes of one shape [Z,Y,X], 0 = background, labels 1..n_A and 1..n_B (a label may be absent; a
value above the count is not measured and counts for nothing).  Row L of A relative to B (NAMES):
  Parent             the label p >= 1 of B under the most voxels of L, ties to the smallest p; 0 without one or when L is absent
  ParentOverlap      that voxel count; 0 without a parent
  Children count     the B objects whose Parent in A (same rule, roles swapped) is L
  Distance_Centroid  centres (sum z, sum y, sum x) / count, exact integer sums and one float64 division each; with spacing
                     (sz, sy, sx): ez = (pz - cz) sz, ey = (py - cy) sy, ex = (px - cx) sx, sqrt((ez ez + ey ey) + ex ex); NaN without
                     a parent
  Distance_Minimum   the same expression with a voxel (z, y, x) for the parent's centre, its minimum over the outline voxels of the
                     parent, then one sqrt; NaN without a parent.  Outline, plane by plane: voxels on the first or last row or column
                     of their plane, or with one of the 8 in-plane neighbours of another value.  The first and last planes are no
                     borders; the voxels above and below do not count.
Tertiary volume: outer where inner == 0, or (shrink_inner) where the voxel is an outline voxel of its inner object; 0 elsewhere.

The voxels are grouped by label with one stable sort; every object is then a slice of the sorted arrays.
"""
import numpy as np

STEMS = ("Parent_{}", "ParentOverlap_{}", "Children_{}_Count", "Distance_Centroid_{}", "Distance_Minimum_{}")
EXACT = (0, 1, 2)  # integer columns: bit-equal on the GPU
FLOAT = (3, 4)     # one sqrt of about a dozen float64 operations in one fixed order: rtol = atol = 1e-12
RTOL = ATOL = 1e-12


def names(other):
    return [s.format(other) for s in STEMS]


def outline(vol):
    """bool [Z,Y,X]: the outline voxels of every object, plane by plane.  Each plane is padded with a value no label has, so a voxel
    on the first or last row or column always has an in-plane neighbour of another value; nothing is compared across planes."""
    vol = np.asarray(vol).astype(np.int64)
    Z, Y, X = vol.shape
    pad = np.full((Z, Y + 2, X + 2), -1, np.int64)
    pad[:, 1:-1, 1:-1] = vol
    edge = np.zeros(vol.shape, bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                edge |= pad[:, dy:dy + Y, dx:dx + X] != vol
    return edge & (vol > 0)


def _groups(vol, n, mask=None):
    """{label: (zs, ys, xs)} of the voxels of labels 1..n (of those under `mask`), by one stable sort."""
    vol = np.asarray(vol).astype(np.int64)
    keep = (vol > 0) & (vol <= n)
    if mask is not None:
        keep &= mask
    zs, ys, xs = np.nonzero(keep)
    v = vol[zs, ys, xs]
    order = np.argsort(v, kind="stable")
    zs, ys, xs, v = zs[order], ys[order], xs[order], v[order]
    cuts = np.flatnonzero(np.diff(v)) + 1
    starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts, [len(v)]])
    return {int(v[s]): (zs[s:e], ys[s:e], xs[s:e]) for s, e in zip(starts, ends) if e > s}


def centres(vol, n):
    """float64 [n, 3] (z, y, x), NaN for a label without voxels."""
    c = np.full((n, 3), np.nan)
    for L, axes in _groups(vol, n).items():
        c[L - 1] = [np.float64(int(q.sum())) / np.float64(len(q)) for q in axes]
    return c


def parents(a, b, na, nb):
    """(parent [na], overlap [na]) int64 of A's labels in B."""
    b = np.asarray(b).astype(np.int64)
    parent, overlap = np.zeros(na, np.int64), np.zeros(na, np.int64)
    for L, (zs, ys, xs) in _groups(a, na).items():
        under = b[zs, ys, xs]
        under = under[(under > 0) & (under <= nb)]
        if under.size:
            labels, counts = np.unique(under, return_counts=True)  # ascending labels: argmax takes the smallest on a tie
            k = int(np.argmax(counts))
            parent[L - 1], overlap[L - 1] = labels[k], counts[k]
    return parent, overlap


def relate3d(a, b, na=None, nb=None, spacing=(1.0, 1.0, 1.0)):
    """Two label volumes [Z,Y,X] -> (rows of A relative to B [na, 5], rows of B relative to A [nb, 5]), float64."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert a.shape == b.shape and a.ndim == 3
    na = int(a.max()) if na is None else na
    nb = int(b.max()) if nb is None else nb
    sp = np.asarray(spacing, np.float64).reshape(3)
    pa_, oa = parents(a, b, na, nb)
    pb_, ob = parents(b, a, nb, na)
    ca, cb = centres(a, na), centres(b, nb)
    return (_rows(na, pa_, oa, pb_, ca, cb, _groups(b, nb, outline(b)), sp),
            _rows(nb, pb_, ob, pa_, cb, ca, _groups(a, na, outline(a)), sp))


def _rows(n, parent, overlap, parent_of_other, centre, centre_other, outline_other, sp):
    out = np.full((n, 5), np.nan)
    out[:, 0], out[:, 1] = parent, overlap
    out[:, 2] = np.bincount(parent_of_other[parent_of_other > 0], minlength=n + 1)[1:n + 1]
    for row in range(n):
        p = int(parent[row])
        if p == 0:
            continue
        cz, cy, cx = centre[row]
        dz, dy, dx = (centre_other[p - 1] - centre[row]) * sp
        out[row, 3] = np.sqrt((dz * dz + dy * dy) + dx * dx)
        zs, ys, xs = outline_other[p]
        ez, ey, ex = (zs.astype(np.float64) - cz) * sp[0], (ys.astype(np.float64) - cy) * sp[1], (xs.astype(np.float64) - cx) * sp[2]
        out[row, 4] = np.sqrt(((ez * ez + ey * ey) + ex * ex).min())
    return out


def relate3d_batch(vols_a, vols_b, counts_a, counts_b, spacing=(1.0, 1.0, 1.0)):
    """Stacks of one call -> (rows of A, rows of B), concatenated in (stack, label) order."""
    rows = [relate3d(a, b, na, nb, spacing) for a, b, na, nb in zip(vols_a, vols_b, counts_a, counts_b)]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


def tertiary(outer, inner, shrink_inner=True):
    outer, inner = np.asarray(outer), np.asarray(inner)
    keep = inner == 0
    if shrink_inner:
        keep |= outline(inner)
    return np.where(keep, outer, 0).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ scenes: (A, B, n_A, n_B)
SHAPE = (3, 12, 16)  # the shape of every scene but the worked one: they go to the GPU as one batch


def worked():
    """The header's example: a [3, 6, 8] stack, two cells side by side on every plane, three nuclei."""
    b = np.zeros((3, 6, 8), np.uint16)
    b[:, :, :4], b[:, :, 4:] = 1, 2
    a = np.zeros((3, 6, 8), np.uint16)
    a[0:2, 1:3, 1:3] = 1
    a[1:3, 3:5, 3:5] = 2
    a[2, 0, 6:8] = 3
    return a, b


S = np.sqrt
WORKED_NUCLEI = np.array([[1, 8, 1, S(1.25), S(2.75)], [1, 4, 1, S(5.25), S(0.75)], [2, 2, 0, S(8.25), 0.5]])
WORKED_CELLS = np.array([[1, 8, 2, S(1.25), S(0.5)], [2, 4, 1, S(5.25), S(2.5)]])
WORKED_TERTIARY_VOLUMES = {False: (60, 66), True: (72, 72)}


def _empty():
    return np.zeros(SHAPE, np.uint16), np.zeros(SHAPE, np.uint16)


def scenes():
    """{name: (A, B, n_A, n_B)}: small stacks, every one another way for the kernels to go wrong."""
    out = {}
    a, b = worked()
    out["worked"] = (a, b, 3, 2)
    # a nucleus across two cells with an exact tie (6 voxels each): the smaller label; the cells differ in size
    a, b = _empty()
    b[0:3, 1:9, 1:6], b[0:2, 1:9, 6:14] = 2, 1
    a[0:2, 3:6, 5:7] = 1
    out["tie"] = (a, b, 1, 2)
    # a nucleus under no cell, beside one with; a second under a value above the count only
    a, b = _empty()
    b[0:2, 1:6, 1:7] = 1
    b[1:3, 7:11, 9:15] = 5
    a[0:2, 2:4, 2:5], a[2, 8:10, 1:4], a[1:3, 8:10, 10:13] = 1, 2, 3
    out["orphan"] = (a, b, 3, 1)
    # absent labels in both sets, the last label included (counts above the largest label)
    a, b = _empty()
    a[0:2, 1:4, 1:4], a[1:3, 6:9, 6:11] = 1, 3
    b[0:3, 0:6, 0:7], b[0:3, 5:11, 5:12] = 2, 4
    out["absent"] = (a, b, 5, 6)
    # a cell with three children, one of them a single voxel
    a, b = _empty()
    b[:, 1:11, 1:15] = 1
    a[0, 2:5, 2:5], a[1:3, 6:9, 8:12], a[1, 3, 12] = 1, 2, 3
    out["three_children"] = (a, b, 3, 1)
    # objects on every face of the volume, in both sets
    a, b = _empty()
    b[:, 0:6, 0:8], b[:, 0:6, 8:16], b[:, 6:12, 0:8], b[:, 6:12, 8:16] = 1, 2, 3, 4
    a[0, 0, 2:5], a[:, 3:7, 15], a[2, 11, 4:9], a[0:2, 2:8, 0], a[1, 5:7, 7:9], a[0, 4:6, 10:12], a[2, 8:10, 3:5] = 1, 2, 3, 4, 5, 6, 7
    out["faces"] = (a, b, 7, 4)
    # a one-voxel parent, and a parent present on one plane only under a child that spans all three
    a, b = _empty()
    b[1, 4, 4] = 1
    b[2, 6:11, 8:14] = 2
    a[0:3, 3:6, 3:6], a[0:3, 7:10, 9:12] = 1, 2
    out["thin_parents"] = (a, b, 2, 2)
    return out


def tertiary_scenes():
    """{name: (outer, inner)} on SHAPE stacks: the nuclei of the scenes inside their cells (caps: a nucleus's first and last plane lose
    their interior), and a cell wholly under a large nucleus."""
    out = {}
    for name in ("three_children", "faces", "absent"):
        a, b, _, _ = scenes()[name]
        out[name] = (b, a)
    outer, inner = _empty()
    outer[:, 1:8, 1:8], outer[0:2, 2:5, 10:13] = 1, 2
    inner[:, 3:6, 3:6], inner[:, 0:8, 8:16] = 1, 2
    out["covered"] = (outer, inner)
    return out
