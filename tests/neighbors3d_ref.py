"""
CPU restatement of `FeatureEngine.neighbors3d` (aliby_amd/csrc/feat_neighbors3d.hip; the definition is in include/aliby_hip.h): the
`neighbors` family (tests/neighbors_ref.py) on volume labels [Z,Y,X].  PARITY with cp_measure / CellProfiler is UNPINNED: the
definition is recalled from CellProfiler 4's measureobjectneighbors.py and centrosome's outline / strel_disk, and neither can be run
here.  tests/test_cpu_neighbors3d_ref.py pins this file to hand values, to scipy.ndimage and to the 2-D restatement.

Direct loops over the definition: every offset of the ball T is visited once and the label volume is compared with itself shifted by
that offset, over the part of the volume where both ends exist (offsets that leave the volume are dropped).  No dilation routine.

  S = {dz^2 + dy^2 + dx^2 <= d^2}, T = {dz^2 + dy^2 + dx^2 <= d^2 + d}; the outline of L, plane by plane = its voxels on the first /
  last row or column of their plane, or with one of the 8 in-plane neighbours carrying another value.  Columns (STEMS): the number of
  distinct foreign labels <= n reached from L's voxels through S; 100 t / p with p the outline voxels and t those that reach a foreign
  non-zero value through T; label and centre distance of the closest and second closest present object (lower key
  (dz dz + dy dy) + dx dx, then lower label; 0 where there is none); the angle atan2(|v1 x v2|, v1 . v2) in degrees between the two
  (NaN for a zero vector, 0 without a second).  A label without voxels: NaN.
"""
import math

import numpy as np

from tests.neighbors_ref import EXACT, STEMS  # noqa: F401 (the 2-D family's columns)

DISTANCES = (None, 2, 5)


def names(distance=None):
    s = "Adjacent" if distance is None else str(distance)
    return [f"Neighbors_{stem}_{s}" for stem in STEMS]


def ball(d, half=False):
    """Offsets (dz, dy, dx) with dz^2 + dy^2 + dx^2 <= d^2 (+ d when `half`: radius d + 0.5)."""
    r2 = d * d + (d if half else 0)
    rng = range(-d, d + 1)
    return [(dz, dy, dx) for dz in rng for dy in rng for dx in rng if dz * dz + dy * dy + dx * dx <= r2]


def _span(n, o):
    lo = max(0, -o)
    return lo, max(min(n, n - o), lo)  # (empty when |o| >= n)


def _shifted(lab, off):
    """(labels at q, labels at q + off, slices of q) over the q for which q + off is inside the volume."""
    spans = [_span(n, o) for n, o in zip(lab.shape, off)]
    here = tuple(slice(lo, hi) for lo, hi in spans)
    there = tuple(slice(lo + o, hi + o) for (lo, hi), o in zip(spans, off))
    return lab[here], lab[there], here


def outline(lab):
    """bool [Z,Y,X]: the outline voxels of every object, plane by plane."""
    lab = np.asarray(lab).astype(np.int64)
    out = np.zeros(lab.shape, bool)
    out[:, 0, :] = out[:, -1, :] = out[:, :, 0] = out[:, :, -1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                a, b, q = _shifted(lab, (0, dy, dx))
                out[q] |= a != b
    return out & (lab > 0)


def centres(lab, n):
    """float64 [n, 3] (z, y, x), NaN for a label without voxels: exact integer sums, one float64 division each."""
    lab = np.asarray(lab).astype(np.int64)
    c = np.full((n, 3), np.nan)
    zz, yy, xx = np.nonzero(lab)
    v = lab[zz, yy, xx]
    for L in np.unique(v):
        if L <= n:
            m = v == L
            cnt = np.float64(int(m.sum()))
            c[L - 1] = (np.float64(int(zz[m].sum())) / cnt, np.float64(int(yy[m].sum())) / cnt, np.float64(int(xx[m].sum())) / cnt)
    return c


def neighbors3d(lab, n=None, distance=None):
    """Label volume [Z,Y,X] -> float64 [n, 7] (n: the rows, labels 1..n; default the largest label)."""
    lab = np.asarray(lab).astype(np.int64)
    assert lab.ndim == 3
    n = int(lab.max()) if n is None else int(n)
    d = 1 if distance is None else int(distance)
    out = np.full((n, 7), np.nan)
    if n == 0:
        return out
    S = set(ball(d))
    reached = np.zeros(lab.shape, bool)  # the voxel reaches a foreign non-zero value through T
    pairs = set()  # (L, v): v reached from a voxel of L through S
    for off in ball(d, half=True):
        a, b, q = _shifted(lab, off)
        foreign = (a > 0) & (b > 0) & (a != b)
        if not foreign.any():
            continue
        reached[q] |= foreign
        if off in S:
            pairs.update(np.unique(a[foreign] * 65536 + b[foreign]).tolist())
    edge = outline(lab)
    present = [int(L) for L in np.unique(lab) if 0 < L <= n]
    count = {L: 0 for L in present}
    for code in pairs:
        L, v = divmod(code, 65536)
        if L in count and v <= n:
            count[L] += 1
    c = centres(lab, n)
    p_of = np.bincount(lab[edge], minlength=n + 1)
    t_of = np.bincount(lab[edge & reached], minlength=n + 1)
    for L in present:
        row = out[L - 1]
        row[0] = count[L]
        row[1] = np.float64(int(t_of[L])) / np.float64(int(p_of[L])) * 100.0
        row[2:] = 0.0
        ranked = []
        for v in present:
            if v != L:
                dz, dy, dx = (np.float64(c[v - 1, k] - c[L - 1, k]) for k in range(3))
                ranked.append((float((dz * dz + dy * dy) + dx * dx), v, float(dz), float(dy), float(dx)))
        ranked.sort(key=lambda r: (r[0], r[1]))
        if len(ranked) >= 1:
            row[2], row[3] = ranked[0][1], math.sqrt(ranked[0][0])
        if len(ranked) >= 2:
            row[4], row[5] = ranked[1][1], math.sqrt(ranked[1][0])
            (_, _, v1z, v1y, v1x), (_, _, v2z, v2y, v2x) = ranked[0], ranked[1]
            if ranked[0][0] == 0.0 or ranked[1][0] == 0.0:
                row[6] = np.nan
            else:
                wz, wy, wx = v1x * v2y - v1y * v2x, v1z * v2x - v1x * v2z, v1y * v2z - v1z * v2y
                row[6] = math.atan2(math.sqrt((wx * wx + wy * wy) + wz * wz), (v1z * v2z + v1y * v2y) + v1x * v2x) * (180.0 / math.pi)
    return out


# ------------------------------------------------------------------------------------------------------------------------ scenes
def _ball_mask(shape, c, r_lo, r_hi):
    zz, yy, xx = np.mgrid[: shape[0], : shape[1], : shape[2]]
    r2 = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2
    return (r2 >= r_lo * r_lo) & (r2 <= r_hi * r_hi)


def worked():
    """The worked case of the definition (include/aliby_hip.h): A and B share a face, B and C meet along one edge across planes."""
    lab = np.zeros((4, 6, 8), np.uint16)
    lab[0:2, 1:3, 1:3] = 1
    lab[0:2, 1:3, 3:5] = 2
    lab[2:4, 3:5, 3:5] = 3
    return lab


SMALL = (13, 36, 44)  # odd, and no multiple of anything


def crowd(shape=SMALL):
    """A ball (label 1) inside a shell of more than 64 one-voxel objects whose labels 4, 7, 10, ... spread over a dozen bitmap words."""
    c = (shape[0] // 2, shape[1] // 2, shape[2] // 2)
    lab = np.zeros(shape, np.uint16)
    lab[_ball_mask(shape, c, 0, 3)] = 1
    zs, ys, xs = np.nonzero(_ball_mask(shape, c, 4.6, 5.2))
    assert len(zs) > 64
    lab[zs, ys, xs] = 4 + 3 * np.arange(len(zs))
    return lab


def small_scenes():
    """name -> (uint16 [13,36,44] label volume, its row count); the batch of tests/test_gpu_neighbors3d.py, in this order."""
    Z, Y, X = SMALL
    s = {}
    s["empty"] = np.zeros(SMALL, np.uint16)  # 0 objects
    one = np.zeros(SMALL, np.uint16)
    one[3:8, 10:17, 20:31] = 1
    s["one"] = one  # 1 object: no candidate at all
    two = np.zeros(SMALL, np.uint16)
    two[2:5, 10:14, 10:15] = 1
    two[6:9, 12:17, 13:20] = 2  # one plane of background between them
    s["two"] = two  # 2 objects: a first candidate, no second
    fec = np.zeros(SMALL, np.uint16)  # every corner, edge and face of the volume: 26 objects two voxels thick, and one beside a corner's
    L = 0
    for kz, (z0, z1) in enumerate(((0, 2), (5, 8), (Z - 2, Z))):
        for ky, (y0, y1) in enumerate(((0, 2), (15, 21), (Y - 2, Y))):
            for kx, (x0, x1) in enumerate(((0, 2), (18, 26), (X - 2, X))):
                if (kz, ky, kx) != (1, 1, 1):
                    L += 1
                    fec[z0:z1, y0:y1, x0:x1] = L
    fec[2:4, 2:4, 2:5] = 27  # diagonal to the corner object
    s["faces_edges_corners"] = fec
    s["full"] = np.ones(SMALL, np.uint16)  # one object filling the whole volume
    sp = np.zeros(SMALL, np.uint16)
    sp[5, 5, 5] = 1  # one voxel, beside a block
    sp[5:8, 5:9, 6:10] = 2
    sp[2:5, 27:31, 35:39] = 3  # farther than 5 from everything
    s["sparse"] = sp
    c = (6, 18, 22)
    shell = np.zeros(SMALL, np.uint16)  # a ball inside a shell: coincident centres
    shell[_ball_mask(SMALL, c, 4.5, 6)] = 1
    shell[_ball_mask(SMALL, c, 0, 2)] = 2
    shell[0:2, 0:2, 0:2] = 3  # a third object, so that the ball and the shell have a second candidate
    s["shell"] = shell
    cross = np.zeros(SMALL, np.uint16)  # six equal objects round a seventh: ties at every rank
    for L, (dz, dy, dx) in enumerate(((-4, 0, 0), (0, -4, 0), (0, 0, -4), (0, 0, 0), (0, 0, 4), (0, 4, 0), (4, 0, 0)), start=1):
        cross[c[0] + dz - 1 : c[0] + dz + 2, c[1] + dy - 1 : c[1] + dy + 2, c[2] + dx - 1 : c[2] + dx + 2] = L
    s["cross"] = cross
    gaps = np.zeros(SMALL, np.uint16)  # labels 2, 5, 6 and 9 of 1..9
    gaps[1:4, 4:10, 4:10] = 2
    gaps[1:4, 4:10, 10:14] = 5
    gaps[4:7, 4:9, 4:12] = 6
    gaps[8:12, 20:30, 30:34] = 9
    s["gaps"] = gaps
    s["crowd"] = crowd()
    scenes = {k: (v, int(v.max())) for k, v in s.items()}
    above = np.zeros(SMALL, np.uint16)  # values above the count: 7 and 9 touch 1 and 2, are not counted and are no rows
    above[3:6, 10:14, 10:14] = 1
    above[3:6, 10:14, 14:18] = 2
    above[6:8, 10:14, 10:14] = 7
    above[3:6, 14:16, 14:18] = 9
    scenes["above"] = (above, 2)
    return scenes


def high_labels():
    """Two touching objects labelled 39 999 and 40 000: 40 000 rows, all but two absent."""
    lab = np.zeros((3, 32, 32), np.uint16)
    lab[0:2, 10:20, 10:20] = 39999
    lab[1:3, 10:20, 20:26] = 40000
    return lab


BIG = (26, 100, 100)


def big_box():
    """One object of 24 x 96 x 96 voxels (every lane of its workgroup strides 864 times) with a small one on one of its faces."""
    lab = np.zeros(BIG, np.uint16)
    lab[1:25, 2:98, 3:99] = 1
    lab[10:13, 98:100, 40:50] = 2
    return lab


def cap_scene():
    """[12,40,40] for the distance cap, d = 16: balls that leave the volume on every side, objects within and beyond reach."""
    lab = np.zeros((12, 40, 40), np.uint16)
    lab[2:9, 3:12, 4:11] = 1
    lab[4:7, 22:27, 8:12] = 2  # 10 from 1 along y
    lab[9:12, 30:40, 20:30] = 3  # beyond 16 from 1, within 16 of 2
    lab[0, 0, 39] = 4
    return lab


_EXPECTED = {}


def expected(key, lab, n=None, distance=None):
    """The restatement of a scene, computed once per (key, distance) and shared; callers must not write into it."""
    k = (key, distance)
    if k not in _EXPECTED:
        _EXPECTED[k] = neighbors3d(lab, n=n, distance=distance)
        _EXPECTED[k].setflags(write=False)
    return _EXPECTED[k]
