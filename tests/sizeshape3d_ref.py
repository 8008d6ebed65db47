"""
CPU restatement of `FeatureEngine.sizeshape3d` (aliby_amd/csrc/feat_sizeshape3d.hip): size and shape of the objects of a
labelled volume, float64 / Python-int numpy, written from the column definitions and sharing no code or method with the kernel.

  * sums are Python ints (exact), the covariance is formed from the exact central moments and handed to numpy.linalg.eigvalsh;
  * the Euler number is that of the union of the object's closed unit cubes, computed by building the SETS of vertices, edges,
    faces and cubes of the object's cubical complex explicitly (each element named by its doubled-coordinate midpoint) and
    counting them: V - E + F - C.  The kernel never builds a set; it classifies 2 x 2 x 2 windows.

tests/test_cpu_sizeshape3d_ref.py pins this file to scipy.ndimage (find_objects, sum, center_of_mass, label), numpy.cov +
eigvalsh, the closed form of a solid ellipsoid and known topologies.  Parity with cp_measure / CellProfiler is unpinned.
"""
import itertools

import numpy as np

NAMES = ["Volume", "BoundingBoxMinimum_X", "BoundingBoxMinimum_Y", "BoundingBoxMinimum_Z", "BoundingBoxMaximum_X", "BoundingBoxMaximum_Y",
         "BoundingBoxMaximum_Z", "BoundingBoxVolume", "Center_X", "Center_Y", "Center_Z", "Extent", "EquivalentDiameter", "EulerNumber",
         "MajorAxisLength", "MinorAxisLength", "InertiaTensorEigenvalues_0", "InertiaTensorEigenvalues_1", "InertiaTensorEigenvalues_2"]
COL = {k: i for i, k in enumerate(NAMES)}
# columns defined on voxel indices alone (spacing does not enter)
INDEX_COLUMNS = [COL[k] for k in NAMES if k.startswith(("BoundingBoxM", "Center_")) or k in ("Extent", "EulerNumber")]


def euler_number(mask) -> int:
    """Euler characteristic of the union of the closed unit cubes of the True voxels of a 3-D mask.
    A cell of the complex is named by twice its midpoint: the cube of voxel v is 2v + (1,1,1); its faces, edges and vertices are
    that point moved by -1 / 0 / +1 per axis (0 keeps the axis' extent): a cell with k axes kept has dimension k."""
    vox = np.argwhere(np.asarray(mask, bool)).astype(np.int64)
    if len(vox) == 0:
        return 0
    centre = 2 * vox + 1
    cells = {0: set(), 1: set(), 2: set(), 3: set()}
    for move in itertools.product((-1, 0, 1), repeat=3):
        dim = sum(1 for m in move if m == 0)
        cells[dim].update(map(tuple, centre + np.asarray(move, np.int64)))
    assert len(cells[3]) == len(vox)
    return len(cells[0]) - len(cells[1]) + len(cells[2]) - len(cells[3])


def covariance(zyx, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """Population covariance [3,3] (axes z, y, x) of integer voxel coordinates [n,3] scaled by spacing, from exact integer sums."""
    n = len(zyx)
    cols = [[int(v) for v in zyx[:, a]] for a in range(3)]
    s1 = [sum(c) for c in cols]
    cov = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            sab = sum(p * q for p, q in zip(cols[a], cols[b]))
            num = n * sab - s1[a] * s1[b]  # exact
            cov[a, b] = cov[b, a] = (num / (n * n)) * (float(spacing[a]) * float(spacing[b]))
    return cov


def sizeshape3d(volume, n=None, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """volume int [Z,Y,X] with labels 1..n (n defaults to the largest label) -> float64 [n, 19] in NAMES order, row = label - 1.
    A label without voxels: Volume 0, NaN elsewhere."""
    volume = np.asarray(volume)
    assert volume.ndim == 3
    n = int(volume.max()) if n is None else int(n)
    dz, dy, dx = (float(s) for s in spacing)
    voxel = dz * dy * dx
    out = np.full((n, len(NAMES)), np.nan)
    for lab in range(1, n + 1):
        mask = volume == lab
        zyx = np.argwhere(mask)
        row = out[lab - 1]
        cnt = len(zyx)
        if cnt == 0:
            row[0] = 0.0
            continue
        lo, hi = zyx.min(axis=0), zyx.max(axis=0) + 1
        box = int(np.prod((hi - lo).astype(np.int64)))
        row[COL["Volume"]] = cnt * voxel
        for k, axis in (("X", 2), ("Y", 1), ("Z", 0)):
            row[COL[f"BoundingBoxMinimum_{k}"]] = lo[axis]
            row[COL[f"BoundingBoxMaximum_{k}"]] = hi[axis]
            row[COL[f"Center_{k}"]] = float(sum(int(v) for v in zyx[:, axis])) / float(cnt)
        row[COL["BoundingBoxVolume"]] = box * voxel
        row[COL["Extent"]] = cnt / box
        row[COL["EquivalentDiameter"]] = (6.0 * cnt * voxel / np.pi) ** (1.0 / 3.0)
        z0, y0, x0 = lo
        z1, y1, x1 = hi
        row[COL["EulerNumber"]] = euler_number(mask[z0:z1, y0:y1, x0:x1])
        cov = covariance(zyx, spacing)
        ev = np.linalg.eigvalsh(cov)  # ascending
        row[COL["MajorAxisLength"]] = np.sqrt(20.0 * max(ev[2], 0.0))
        row[COL["MinorAxisLength"]] = np.sqrt(20.0 * max(ev[0], 0.0))
        tr = cov[0, 0] + cov[1, 1] + cov[2, 2]
        row[COL["InertiaTensorEigenvalues_0"]] = tr - ev[0]
        row[COL["InertiaTensorEigenvalues_1"]] = tr - ev[1]
        row[COL["InertiaTensorEigenvalues_2"]] = tr - ev[2]
    return out


# ------------------------------------------------------------------------------------------------ shapes with known topology
def ball(radius, size=None, centre=None):
    size = size or 2 * int(radius) + 5
    g = np.mgrid[:size, :size, :size].astype(np.float64)
    c = (size - 1) / 2.0 if centre is None else None
    cz, cy, cx = (c, c, c) if centre is None else centre
    return (g[0] - cz) ** 2 + (g[1] - cy) ** 2 + (g[2] - cx) ** 2 <= radius * radius


def topology_cases():
    """(name, bool mask [Z,Y,X], Euler number)."""
    cases = []
    b = ball(10, 27)
    cases.append(("solid ball", b, 1))
    one = b.copy()
    one[ball(3, 27)] = False
    cases.append(("ball with one cavity", one, 2))
    two = b.copy()
    two[ball(2, 27, (13, 13, 8))] = False
    two[ball(2, 27, (13, 13, 18))] = False
    cases.append(("ball with two cavities", two, 3))
    g = np.mgrid[-6:7, -15:16, -15:16].astype(np.float64)
    ring_r = np.sqrt(g[1] ** 2 + g[2] ** 2)
    cases.append(("solid torus", (ring_r - 9.0) ** 2 + g[0] ** 2 <= 9.0, 0))
    corner = np.zeros((4, 4, 4), bool)
    corner[1, 1, 1] = corner[2, 2, 2] = True
    cases.append(("two voxels meeting at a corner", corner, 1))
    far = np.zeros((12, 12, 30), bool)
    far[:11, :11, :11] |= ball(4, 11)
    far[:11, :11, 19:] |= ball(4, 11)
    cases.append(("two far-apart balls under one label", far, 2))
    ring = np.zeros((3, 5, 5), bool)
    ring[1, 1:4, 1:4] = True
    ring[1, 2, 2] = False
    cases.append(("one-voxel-thick ring", ring, 0))
    return cases


def random_labels(seed, shape, n_seeds=12, quantile=None):
    """Random irregular label volume (the generator style of tests/fuzz/): a smoothed noise field thresholded into blobs, cut
    into labels by nearest seed, so that objects touch each other and the faces of the volume.  -> (uint16 [Z,Y,X], n)."""
    from scipy import ndimage as ndi

    rng = np.random.default_rng(seed)
    field = ndi.gaussian_filter(rng.standard_normal(shape), (1.0, 2.0, 2.0))
    fg = field > np.quantile(field, 0.55 if quantile is None else quantile)
    pts = np.stack([rng.integers(0, s, n_seeds) for s in shape], axis=1)
    g = np.stack(np.mgrid[:shape[0], :shape[1], :shape[2]], axis=-1)
    d = ((g[:, :, :, None, :] - pts[None, None, None]) ** 2).sum(-1)
    lab = (d.argmin(-1) + 1) * fg
    present = np.unique(lab[lab > 0])
    lut = np.zeros(n_seeds + 1, np.uint16)
    lut[present] = np.arange(1, len(present) + 1)
    return lut[lab], len(present)
