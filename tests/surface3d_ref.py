"""
CPU restatement of the `SurfaceArea` column of `FeatureEngine.sizeshape3d(..., surface_area=True)` (aliby_amd/csrc/feat_surface3d.hip).

CellProfiler measures, per label, scikit-image's mesh_surface_area of the Lewiner marching-cubes mesh at level 0 of the label's mask
in its bounding box grown by one voxel and clipped to the volume.  On a binary volume that mesh is made cell by cell, and a cell's
triangles depend only on which of its eight voxels are set, so

    SurfaceArea(label) = sum over configurations c = 1 .. 254, in increasing c, of float64(count_c) * area256[c]

where count_c is the number of 2 x 2 x 2 cells of the volume grid (all eight voxels inside the volume, nothing padded) whose
configuration for `== label` is c; bit 4 dz + 2 dy + dx of c stands for voxel (z + dz, y + dy, x + dx).  This file computes that in
NumPy: `histogram` counts with whole-array comparisons (it shares nothing with the kernel's window walk), `surface_area` takes the
sequential float64 sum, one multiplication and one addition per configuration, which is the order the kernel uses, so the two
must agree bit for bit when fed the same table.  A label's cells are looked for in its bounding box grown by one voxel and clipped:
every cell outside it has configuration 0.

`table_from_triangles` builds area256 from the triangle lists of tests/golden/skimage_marching_cubes_level0.json (recorded from
scikit-image by scripts/make_surface3d_fixture.py); tests/test_cpu_surface3d_ref.py pins all of this to scikit-image's own numbers.
"""
import json
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "skimage_marching_cubes_level0.json"
_fixture = None


def fixture() -> dict:
    """The recorded scikit-image data (read once)."""
    global _fixture
    if _fixture is None:
        _fixture = json.loads(FIXTURE.read_text())
    return _fixture


def fixture_volumes():
    """-> [(name, labels uint16 [Z,Y,X], n, {spacing tuple: recorded per-label SurfaceArea float64 [n]})]."""
    out = []
    for v in fixture()["volumes"]:
        lab = np.asarray(v["labels"], np.uint16).reshape(v["shape"])
        out.append((v["name"], lab, int(v["n"]), {tuple(r["spacing"]): np.asarray(r["values"], np.float64) for r in v["surface_area"]}))
    return out


def table_from_triangles(triangles, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
    """triangles[c] = list of triangles, each three (z, y, x) vertices in cell units -> float64 [256]:
    area[c] = sum of 1/2 |((b - a) * s) x ((c - a) * s)| over the triangles of c in list order."""
    s = np.asarray(spacing, np.float64)
    area = np.zeros(256)
    for c, tris in enumerate(triangles):
        total = 0.0
        for a, b, d in np.asarray(tris, np.float64).reshape(-1, 3, 3):
            total += 0.5 * float(np.linalg.norm(np.cross((b - a) * s, (d - a) * s)))
        area[c] = total
    return area


def histogram(mask) -> np.ndarray:
    """bool [Z,Y,X] (each axis >= 2) -> int64 [256]: how many cells of the grid have each configuration."""
    m = np.asarray(mask, bool)
    if m.ndim != 3 or min(m.shape) < 2:
        raise ValueError(f"a marching-cubes cell needs at least 2 x 2 x 2 voxels, got {m.shape}")
    Z, Y, X = m.shape
    cfg = np.zeros((Z - 1, Y - 1, X - 1), np.int64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cfg += m[dz:Z - 1 + dz, dy:Y - 1 + dy, dx:X - 1 + dx].astype(np.int64) << (4 * dz + 2 * dy + dx)
    return np.bincount(cfg.ravel(), minlength=256)


def label_histogram(volume, label) -> np.ndarray:
    """Histogram of `volume == label` over the volume grid, entry 0 left out (set to 0); all zeros for a label without voxels."""
    volume = np.asarray(volume)
    if volume.ndim != 3 or min(volume.shape) < 2:
        raise ValueError(f"a marching-cubes cell needs at least 2 x 2 x 2 voxels, got {volume.shape}")
    zyx = np.argwhere(volume == label)
    if len(zyx) == 0:
        return np.zeros(256, np.int64)
    lo = np.maximum(zyx.min(axis=0) - 1, 0)
    hi = np.minimum(zyx.max(axis=0) + 2, volume.shape)
    h = histogram(volume[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] == label)
    h[0] = 0
    return h


def sum_histogram(hist, area256) -> float:
    total = np.float64(0.0)
    for c in range(1, 255):
        total = total + np.float64(int(hist[c])) * np.float64(area256[c])
    return float(total)


def surface_area(volume, n, spacing, area256) -> np.ndarray:
    """volume int [Z,Y,X] with labels 1..n -> float64 [n], row = label - 1.  A label without voxels: NaN; an object without a
    mixed cell (it fills the volume): 0.  `spacing` is not used beyond what area256 already holds; it is taken so that a call
    names the table's spacing."""
    del spacing
    volume = np.asarray(volume)
    out = np.full(int(n), np.nan)
    for lab in range(1, int(n) + 1):
        h = label_histogram(volume, lab)
        if h.any():  # (entry 255 counts: the object that fills the volume)
            out[lab - 1] = sum_histogram(h, area256)
    return out


def random_labels(seed, shape, n_seeds=10):
    """Touching irregular objects that reach the faces of the volume, for shapes down to (2, 2, 2) -> (uint16 [Z,Y,X], n):
    noise summed with its neighbours, kept above its 45 % quantile, cut into labels by nearest seed (NumPy only)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape)
    for axis in range(3):
        f = f + np.roll(f, 1, axis) + np.roll(f, -1, axis)
    fg = f > np.quantile(f, 0.45)
    pts = np.stack([rng.integers(0, s, n_seeds) for s in shape], axis=1)
    g = np.stack(np.mgrid[:shape[0], :shape[1], :shape[2]], axis=-1)
    lab = (((g[:, :, :, None, :] - pts) ** 2).sum(-1).argmin(-1) + 1) * fg
    present = np.unique(lab[lab > 0])
    lut = np.zeros(n_seeds + 1, np.uint16)
    lut[present] = np.arange(1, len(present) + 1)
    return lut[lab], len(present)
