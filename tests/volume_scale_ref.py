"""
The stack of tests/test_gpu_volume_scale.py: thin (X = 1) and long enough that every volume kernel runs out of grid and goes
round its grid-stride loop.  tests/test_cpu_volume_scale.py asserts, without a GPU, that it exceeds each cap and where its objects
lie in each kernel's order of work items.

The caps (a kernel's first pass covers this many work items; no C symbol exports them, so they are restated here beside their
source lines) and the order in which each kernel numbers its work items:
"""
import numpy as np

SEGMENT = 16
# feat_intensity3d.hip:49,127 (k_intensity3d) and volume_table.h:24,53 (k_volume_table, the front end of coloc3d and texture3d):
# 32768 workgroups of 256 lanes, a lane per 16-voxel segment; item = ((f * Z + z) * Y + y) * ceil(X / 16) + x / 16
SEGMENT_CAP = 32768 * 256
# feat_sizeshape3d.hip:67,209 (k_sizeshape3d): 65536 workgroups, one per tile of 8 x 8 x 64 corners of the (Z + 1)(Y + 1)(X + 1)
# corner grid; tile = ((f * (Z / 8 + 1) + z / 8) * (Y / 8 + 1) + y / 8) * (X / 64 + 1) + x / 64.  Voxel (z, y, x) is read by the
# corners (z .. z + 1, y .. y + 1, x .. x + 1)
TILE_CAP = 65536
TILE = (8, 8, 64)
# track.hip:203,229 (k_apply_lut, behind stitch_planes): 16384 workgroups of 256 lanes, a lane per voxel of the planes laid out
# [Z, F, Y, X]; item = ((z * F + f) * Y + y) * X + x
VOXEL_CAP = 16384 * 256

SHAPE = (130, 65536, 1)        # one stack [Z, Y, X]: 8 519 680 voxels, 17 MB of labels
BATCH_SHAPE = (2, 65, 65536, 1)  # the same memory as two stacks [F, Z, Y, X]: stack 1 is planes 65..129
N_OBJECTS = 6
# label -> (z0, z1, y0, y1), half-open: the box its voxels are drawn in
BOXES = {1: (3, 13, 100, 141),        # first pass of every kernel
         2: (59, 69, 30000, 30031),   # across z = 64: the pass boundary of k_sizeshape3d (tile row 8) and of k_apply_lut
         3: (90, 100, 65500, 65536),  # beyond the first pass of k_sizeshape3d and k_apply_lut, at the far end of y
         4: (124, 130, 0, 41),        # across z = 128: the pass boundary of k_intensity3d and k_volume_table
         5: (128, 130, 40000, 40051),  # wholly beyond the first pass of every kernel
         6: (129, 130, 65535, 65536)}  # the very last voxel of the stack


def segment_items(f, z, y, x, shape4):
    """Work item of k_intensity3d / k_volume_table that reads voxel (f, z, y, x) of a batch [F, Z, Y, X]."""
    _, Z, Y, X = shape4
    segs = (X + SEGMENT - 1) // SEGMENT
    return ((f * Z + z) * Y + y) * segs + x // SEGMENT


def tile_items(f, z, y, x, shape4):
    """Tiles of k_sizeshape3d that read voxel (f, z, y, x): those of its eight corners -> int64 [8, ...]."""
    _, Z, Y, X = shape4
    ntz, nty, ntx = Z // TILE[0] + 1, Y // TILE[1] + 1, X // TILE[2] + 1
    out = []
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                out.append(((f * ntz + (z + dz) // TILE[0]) * nty + (y + dy) // TILE[1]) * ntx + (x + dx) // TILE[2])
    return np.stack(out)


def voxel_items(f, z, y, x, shape4):
    """Work item of k_apply_lut that writes voxel (f, z, y, x): the planes are laid out [Z, F, Y, X]."""
    F, _, Y, X = shape4
    return ((z * F + f) * Y + y) * X + x


def n_items(shape4):
    """-> (16-voxel segments, sizeshape3d tiles, voxels) of a batch [F, Z, Y, X]."""
    F, Z, Y, X = shape4
    return (F * Z * Y * ((X + SEGMENT - 1) // SEGMENT), F * (Z // TILE[0] + 1) * (Y // TILE[1] + 1) * (X // TILE[2] + 1), F * Z * Y * X)


_CACHE = {}


def stack():
    """-> (labels uint16 [130,65536,1], 6, pixels uint16 [2,130,65536,1]), built once per process.  Each object is an irregular blob
    inside its box (an ellipse with a ragged edge and holes); the two channels inside the boxes are two mixtures of one smooth
    field, each with noise of its own (a correlation well away from 0, so that no Costes probe sits at a sign change), and uniform
    noise elsewhere."""
    if "stack" in _CACHE:
        return _CACHE["stack"]
    from scipy import ndimage as ndi

    rng = np.random.default_rng(130)
    vol = np.zeros(SHAPE, np.uint16)
    px = rng.integers(0, 65536, size=(2, *SHAPE), dtype=np.uint16)
    for lab, (z0, z1, y0, y1) in BOXES.items():
        d, h = z1 - z0, y1 - y0
        zz, yy = np.mgrid[:d, :h]
        r = ((zz - (d - 1) / 2.0) / (d / 2.0)) ** 2 + ((yy - (h - 1) / 2.0) / (h / 2.0)) ** 2
        blob = (r <= 1.0 + 0.3 * rng.standard_normal((d, h))) & (rng.random((d, h)) > 0.08)
        blob[0, :] |= r[0, :] <= 1.0   # the box's first and last plane and its first and last row are reached
        blob[-1, :] |= r[-1, :] <= 1.0
        blob[d // 2, 0] = blob[d // 2, -1] = blob[0, h // 2] = blob[-1, h // 2] = True
        vol[z0:z1, y0:y1, 0][blob] = lab
        shared = ndi.gaussian_filter(rng.standard_normal((d, h)), 1.5)
        for c in range(2):
            own = ndi.gaussian_filter(rng.standard_normal((d, h)), 1.0)
            field = (0.8 - 0.2 * c) * shared / max(shared.std(), 1e-9) + (0.4 + 0.2 * c) * own / max(own.std(), 1e-9)
            field = (field - field.min()) / max(field.max() - field.min(), 1e-9)
            px[c, z0:z1, y0:y1, 0] = np.round(500.0 + 60000.0 * field).astype(np.uint16)
    _CACHE["stack"] = (vol, N_OBJECTS, px)
    return _CACHE["stack"]


def per_plane_labels(vol):
    """Volume labels [Z,Y,X] -> every plane relabelled 1..n_z on its own, by connected component (what a 2-D segmenter would hand
    to stitch_planes)."""
    from scipy import ndimage as ndi

    out = np.zeros(vol.shape, np.uint16)
    for z in range(vol.shape[0]):
        if vol[z].any():
            out[z] = ndi.label(vol[z] > 0)[0]
    return out
