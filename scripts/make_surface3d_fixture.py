"""
Writes the two files `SurfaceArea` of `FeatureEngine.sizeshape3d(..., surface_area=True)` is pinned with:

  tests/golden/skimage_marching_cubes_level0.json   recorded from scikit-image (data only)
  aliby_amd/csrc/mc_level0_table.h                  the same triangle lists as a C table (plain data)

Run it with an interpreter that has scikit-image (0.18.3 when the committed files were made; the version is written into both
files, CellProfiler's pinned upstream is 0.26.0, so a regeneration with another version shows up as a diff).  It is never run by a
test or on the GPU.

What is recorded.  CellProfiler's 3-D MeasureObjectSizeShape (and cp_measure's `sizeshape` on volumes) measures, per label,

    crop = labels[bbox grown by one voxel, clipped to the volume] == label
    verts, faces, _, _ = skimage.measure.marching_cubes(crop, method="lewiner", spacing=spacing, level=0)
    SurfaceArea = skimage.measure.mesh_surface_area(verts, faces)

For a binary volume at level 0 the triangles Lewiner's tables emit for one 2 x 2 x 2 cell depend only on which of its eight
voxels are set, so the mesh area is a sum over cells of a 256-entry table.  This script takes that table from scikit-image
itself: for each of the 254 mixed configurations it runs marching_cubes on the 2 x 2 x 2 volume at unit spacing, drops the
zero-area triangles and snaps the vertices to thirds of a cell (every vertex lies on a voxel centre, except one interior vertex
of configurations 107, 109, 182 and 214).  Configuration bit 4 dz + 2 dy + dx stands for voxel (z + dz, y + dy, x + dx).

It also records area[256] as scikit-image returns it at three spacings, and a few small label volumes with scikit-image's
per-label result of the loop above at unit and at anisotropic spacing.
"""
import json
import sys
import warnings
from pathlib import Path

import numpy as np
import skimage
from skimage.measure import marching_cubes, mesh_surface_area

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "skimage_marching_cubes_level0.json"
HEADER = ROOT / "aliby_amd" / "csrc" / "mc_level0_table.h"
SPACINGS = [(1.0, 1.0, 1.0), (2.5, 1.0, 1.0), (3.0, 0.7, 1.3)]
VOLUME_SPACINGS = [(1.0, 1.0, 1.0), (3.0, 0.7, 1.3)]


def cell(config):
    v = np.zeros((2, 2, 2), bool)
    for b in range(8):
        if config >> b & 1:
            v[b >> 2, (b >> 1) & 1, b & 1] = True
    return v


def mesh(mask, spacing):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        verts, faces, _, _ = marching_cubes(mask, level=0, method="lewiner", spacing=spacing)
    return verts, faces


def triangles_in_thirds(config):
    """-> int [k, 3, 3]: the triangles of non-zero area of one configuration, vertices (z, y, x) in thirds of a cell."""
    verts, faces = mesh(cell(config), (1.0, 1.0, 1.0))
    thirds = np.rint(verts.astype(np.float64) * 3.0)
    assert np.abs(thirds / 3.0 - verts).max() <= 1e-6, (config, verts)
    tri = thirds[faces].astype(np.int64)  # [k, 3 vertices, 3 coordinates]
    assert tri.min() >= 0 and tri.max() <= 3
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return tri[(cross != 0).any(axis=1)]


def label_areas(labels, n, spacing):
    """The per-label loop of CellProfiler / cp_measure."""
    out = []
    Z, Y, X = labels.shape
    for lab in range(1, n + 1):
        zyx = np.argwhere(labels == lab)
        assert len(zyx), "every label of a fixture volume has voxels"
        (z0, y0, x0), (z1, y1, x1) = zyx.min(axis=0), zyx.max(axis=0) + 1
        crop = labels[max(z0 - 1, 0):min(z1 + 1, Z), max(y0 - 1, 0):min(y1 + 1, Y), max(x0 - 1, 0):min(x1 + 1, X)] == lab
        verts, faces = mesh(crop, spacing)
        out.append(float(mesh_surface_area(verts, faces)))
    return out


def blobs(seed, shape, n_seeds):
    """Touching irregular objects that reach every face: a box-smoothed noise field above its 45 % quantile, cut by nearest seed."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape)
    for axis in range(3):
        f = f + np.roll(f, 1, axis) + np.roll(f, -1, axis)
    fg = f > np.quantile(f, 0.45)
    pts = np.stack([rng.integers(0, s, n_seeds) for s in shape], axis=1)
    g = np.stack(np.mgrid[:shape[0], :shape[1], :shape[2]], axis=-1)
    lab = (((g[:, :, :, None, :] - pts) ** 2).sum(-1).argmin(-1) + 1) * fg
    present = np.unique(lab[lab > 0])
    lut = np.zeros(n_seeds + 1, np.int64)
    lut[present] = np.arange(1, len(present) + 1)
    return lut[lab].astype(np.uint16), len(present)


def shapes():
    """A one-voxel object, a ring (one tunnel), a hollow box (one cavity), two boxes face to face, and a box in a corner."""
    v = np.zeros((8, 12, 16), np.uint16)
    v[2, 2, 2] = 1  # one voxel, interior
    v[4, 1:6, 6:11] = 2  # a ring around a 1 x 3 x 3 hole ...
    v[4, 2:5, 7:10] = 0
    v[3:5, 1:6, 6] = 2  # ... thickened on one side
    v[1:6, 6:11, 1:6] = 3  # hollow box
    v[3, 8, 3] = 0
    v[1:4, 7:11, 11:13] = 4  # two boxes sharing a face
    v[1:4, 7:11, 13:16] = 5  # (this one reaches the high x face)
    v[6:8, 0:2, 13:16] = 6  # a corner of the volume
    v[0, 0, 0] = 7  # one voxel in a corner
    return v, 7


def faces_volume():
    """Objects on every face of the volume, two of them filling a whole face, and a one-voxel-wide bar through the volume."""
    v = np.zeros((6, 9, 11), np.uint16)
    v[0, :, :] = 1  # the whole low z face
    v[5, 2:7, 3:9] = 2  # on the high z face
    v[2:4, 0, 1:10] = 3  # low y
    v[2:5, 8, :] = 4  # high y, edge to edge
    v[1:5, 2:7, 0] = 5  # low x
    v[1:5, 3:6, 10] = 6  # high x
    v[3, 1:8, 5] = 7  # a bar that touches nothing
    return v, 7


def main():
    tris = [np.zeros((0, 3, 3), np.int64)] + [triangles_in_thirds(c) for c in range(1, 255)] + [np.zeros((0, 3, 3), np.int64)]
    total = sum(len(t) for t in tris)
    print(f"{total} triangles of non-zero area, at most {max(len(t) for t in tris)} per configuration", file=sys.stderr)
    area = []
    for sp in SPACINGS:
        row = [0.0]
        for c in range(1, 255):
            verts, faces = mesh(cell(c), sp)
            row.append(float(mesh_surface_area(verts, faces)))
        area.append(row + [0.0])
    volumes = []
    for name, (lab, n) in (("blobs", blobs(7, (6, 10, 14), 9)), ("blobs_thin", blobs(3, (2, 11, 16), 6)), ("shapes", shapes()),
                           ("faces", faces_volume())):
        assert lab.max() == n
        volumes.append({"name": name, "shape": list(lab.shape), "n": n, "labels": [int(x) for x in lab.ravel()],
                        "surface_area": [{"spacing": list(sp), "values": label_areas(lab, n, sp)} for sp in VOLUME_SPACINGS]})
    doc = {
        "what": "skimage.measure.marching_cubes(method='lewiner', level=0) on binary volumes: per-configuration triangles of a "
                "2x2x2 cell, cell areas, and per-label mesh_surface_area of small label volumes (scripts/make_surface3d_fixture.py)",
        "skimage_version": skimage.__version__,
        "numpy_version": np.__version__,
        "cellprofiler_pins_skimage": "0.26.0",
        "bit_order": "configuration bit 4*dz + 2*dy + dx = voxel (z+dz, y+dy, x+dx); vertices are (z, y, x) in cell units",
        "triangles": [[[[float(k) / 3.0 for k in vert] for vert in t] for t in cfg] for cfg in tris],
        "spacings": [list(sp) for sp in SPACINGS],
        "area256": area,
        "volumes": volumes,
    }
    FIXTURE.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    first = np.concatenate([[0], np.cumsum([len(t) for t in tris])])
    flat = np.concatenate(tris).reshape(-1, 9)
    lines = [
        "// mc_level0_table.h: GENERATED by scripts/make_surface3d_fixture.py, do not edit.  Plain data recorded from scikit-image",
        f"// {skimage.__version__} (numpy {np.__version__}): the triangles of non-zero area that skimage.measure.marching_cubes(method=\"lewiner\", level=0)",
        "// emits for one 2 x 2 x 2 cell of a binary volume, per configuration (bit 4 dz + 2 dy + dx = voxel (z + dz, y + dy, x + dx)).",
        "// A triangle is nine numbers, (z, y, x) of its three vertices in THIRDS of a cell; configuration c owns triangles",
        "// MC0_FIRST[c] .. MC0_FIRST[c + 1] - 1, in the order scikit-image emits them.  The same lists, with scikit-image's own areas,",
        "// are in tests/golden/skimage_marching_cubes_level0.json.",
        "#pragma once",
        "",
        f"#define MC0_TRIANGLES {len(flat)}",
        "",
        "static const unsigned short MC0_FIRST[257] = {",
    ]
    for i in range(0, 257, 16):
        lines.append("    " + " ".join(f"{int(v)}," for v in first[i:i + 16]))
    lines += ["};", "", "static const unsigned char MC0_TRI[MC0_TRIANGLES][9] = {"]
    for c in range(256):
        for t in tris[c].reshape(-1, 9):
            lines.append("    {" + ", ".join(str(int(k)) for k in t) + f"}},  // {c}")
    lines += ["};", ""]
    HEADER.write_text("\n".join(lines))
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes) and {HEADER}", file=sys.stderr)


if __name__ == "__main__":
    main()
