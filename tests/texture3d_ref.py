"""
NumPy reference of `FeatureEngine.texture3d` (aliby_amd/csrc/feat_texture3d.hip) and the inputs of its tests.

What is new on volumes is restated here: the crop of an object's bounding box in (z, y, x) and the 13 symmetric co-occurrence
matrices.  Everything else is the oracle's 2-D code, imported: `img_as_ubyte` and the `gray_levels` rescale for the grey levels,
`haralick_features` for the 13 statistics (oracle/texture_restated.py).  tests/test_cpu_texture3d_ref.py pins this file to the
oracle's 2-D numbers, to a brute-force pair loop and to textbook sums.  Parity with cp_measure / mahotas on volumes is unpinned.

DELTAS_3D is the one place the reference knows the order of the directions (offsets on the array axes z, y, x): mahotas'
`_3d_deltas` as recalled, not as read.  The matrices are symmetrised, so any 13 directions covering one half of the 26 neighbours
give the same numbers; only the column block of a direction rests on the recall.
"""
import numpy as np
from scipy import ndimage as ndi

from oracle.texture_restated import HARALICK, haralick_features, img_as_ubyte

DELTAS_3D = [(1, 0, 0), (1, 1, 0), (0, 1, 0), (1, -1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 1), (1, 0, -1), (0, 1, -1),
             (1, 1, -1), (1, -1, -1)]
N_DIR, N_STAT = len(DELTAS_3D), len(HARALICK)
N_COLS = N_DIR * N_STAT
IN_PLANE = {4: 0, 6: 1, 2: 2, 10: 3}  # 3-D direction block -> the 2-D family's, for a stack of one plane


def grey_levels(pixels, gray_levels=256) -> np.ndarray:
    """Pixels (uint16, or float in [0, 1]) -> the 2-D family's grey levels (oracle.texture_restated.get_texture's first lines)."""
    q = img_as_ubyte(pixels)
    if gray_levels != 256:
        q = (q.astype(np.float64) / 255.0 * (gray_levels - 1)).astype(np.uint8)
    return q


def cooccurrence3d(crop, delta, distance) -> np.ndarray:
    """crop int [d,h,w] -> symmetric int64 matrix of side crop.max() + 1 over the voxel pairs (p, p + distance * delta) inside it
    (grey level 0 is still counted here: haralick_features clears its row and column, as mahotas' ignore_zeros does)."""
    fm1 = int(crop.max()) + 1
    cmat = np.zeros((fm1, fm1), np.int64)
    lo, hi, lo2, hi2 = [], [], [], []
    for n, d in zip(crop.shape, delta):
        s = d * distance
        a, b = max(0, -s), min(n, n - s)
        if b <= a:
            return cmat
        lo.append(a), hi.append(b), lo2.append(a + s), hi2.append(b + s)
    a = crop[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].ravel()
    b = crop[lo2[0]:hi2[0], lo2[1]:hi2[1], lo2[2]:hi2[2]].ravel()
    np.add.at(cmat, (a, b), 1)
    return cmat + cmat.T


def object_crops(volume, grey, n=None):
    """-> one int64 crop [d,h,w] per label 1..n (None for a label without voxels): the bounding box of all the label's voxels,
    every other voxel 0."""
    volume = np.asarray(volume)
    n = int(volume.max()) if n is None else int(n)
    out = []
    for i, sl in enumerate(ndi.find_objects(volume.astype(np.int32), max_label=n)):
        out.append(None if sl is None else np.where(volume[sl] == i + 1, grey[sl], 0).astype(np.int64))
    return out + [None] * (n - len(out))


def texture3d(volume, pixels, n=None, scale=3, gray_levels=256) -> np.ndarray:
    """volume int [Z,Y,X] with labels 1..n, pixels [Z,Y,X] -> float64 [n, 169], row = label - 1, direction-major columns; a
    direction without a pair gives 13 NaN, a label without voxels a row of NaN."""
    crops = object_crops(volume, grey_levels(pixels, gray_levels), n)
    out = np.full((len(crops), N_COLS), np.nan)
    for i, crop in enumerate(crops):
        if crop is None:
            continue
        for d, delta in enumerate(DELTAS_3D):
            try:
                out[i, d * N_STAT:(d + 1) * N_STAT] = haralick_features(cooccurrence3d(crop, delta, scale))
            except ValueError:  # an empty matrix: mahotas raises, CellProfiler records NaN
                pass
    return out


def texture3d_batch(vols, pixels, channel, counts, scale=3, gray_levels=256) -> np.ndarray:
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] -> float64 [sum counts, 169]."""
    rows = [texture3d(v, pixels[f][channel], c, scale, gray_levels) for f, (v, c) in enumerate(zip(vols, counts))]
    return np.concatenate(rows) if rows else np.zeros((0, N_COLS))


# ------------------------------------------------------------------------------------------------ inputs
def budget_volume(lds_voxels):
    """-> (labels, 5, pixels uint16 [1,Z,Y,X], box voxels per label): bounding boxes of exactly lds_voxels voxels, one more row
    than that, one row fewer, about 3 x lds_voxels, and a 1 x 3 x 3 plate (thinner than any scale along z)."""
    from tests.coloc3d_ref import noise_pixels

    w = 64
    assert lds_voxels % (8 * w) == 0
    h = lds_voxels // (8 * w)
    shape = (20, 2 * h + 12, 3 * w + 8)
    vol = np.zeros(shape, np.uint16)
    vol[1:9, 1:1 + h, 1:1 + w] = 1                          # box = lds_voxels exactly
    vol[1:9, 1:2 + h, 2 + w:2 + 2 * w] = 2                  # one more row: 8 (h + 1) w
    vol[1:9, 1:1 + h, 2 + w] = 0                            # (a face carved: the box stays, the object is not its box)
    vol[1, 1, 2 + w] = 2
    vol[11:19, 3 + h:2 + 2 * h, 1:1 + w] = 3                # one row fewer: 8 (h - 1) w
    vol[10:20, 3 + h:10 + 2 * h, 2 + w:7 + 3 * w] = 4       # 10 (h + 7) (2 w + 5)
    vol[10:13, 3 + h:20 + h, 2 + w:30 + w] = 0              # (a corner cut away)
    vol[10, 3 + h, 2 + w] = 4
    vol[0, -3:, -3:] = 5
    boxes = np.asarray([np.prod([s.stop - s.start for s in sl]) for sl in ndi.find_objects(vol.astype(np.int32))])
    return vol, 5, noise_pixels(7, shape, 1), boxes


def stretched_box(lds_voxels):
    """-> (labels [2][Z,Y,X], pixels uint16 [2,1,Z,Y,X]): the same object twice, in stack 1 with one far voxel of its label whose
    pixel is 0 (grey level 0: it joins no pair and leaves the largest grey level alone) that stretches the bounding box
    beyond lds_voxels.  Every matrix of the object is the same in both stacks; the kernel takes the first from LDS and the second
    from global scratch."""
    from tests.coloc3d_ref import noise_pixels

    side = int(np.ceil((4.0 * lds_voxels) ** (1.0 / 3.0))) + 2
    shape = (side, side, side)
    vol = np.zeros(shape, np.uint16)
    zz, yy, xx = np.mgrid[:side, :side, :side]
    vol[((zz - 6) / 5.0) ** 2 + ((yy - 9) / 8.0) ** 2 + ((xx - 10) / 9.0) ** 2 <= 1.0] = 1
    px = noise_pixels(17, shape, 1)
    far = vol.copy()
    far[-1, -1, -1] = 1
    px[0, -1, -1, -1] = 0
    return [vol, far], np.stack([px, px])


def grey_edge_volume():
    """-> (labels, 5, pixels uint16 [1,Z,Y,X]): label 1 takes all 255 non-zero grey levels (uniform noise over a large box), label 2
    one grey level, label 3 only pixels below 128 (grey level 0 everywhere, as uint16 and as unit float), label 4 a single voxel, label 5 a 2 x 9 x 11 plate."""
    rng = np.random.default_rng(77)
    shape = (14, 40, 96)
    vol = np.zeros(shape, np.uint16)
    px = rng.integers(256, 65536, size=shape, dtype=np.uint16)
    vol[1:13, 2:38, 2:50] = 1
    vol[1:9, 2:20, 54:70] = 2
    px[vol == 2] = 77 * 256 + 5
    vol[1:9, 22:38, 54:70] = 3
    px[vol == 3] = rng.integers(0, 128, size=int((vol == 3).sum()), dtype=np.uint16)
    vol[2, 5, 80] = 4
    vol[10:12, 20:29, 76:87] = 5
    return vol, 5, px[None]


def random_case(seed):
    """-> (labels, n, pixels uint16 [1,Z,Y,X], scale): a seeded random volume of touching labels, random scale in 1..4."""
    from tests.coloc3d_ref import noise_pixels
    from tests.sizeshape3d_ref import random_labels

    rng = np.random.default_rng(500 + seed)
    shape = (int(rng.integers(3, 14)), int(rng.integers(24, 56)), int(rng.integers(24, 64)))
    vol, n = random_labels(600 + seed, shape, n_seeds=int(rng.integers(3, 10)))
    return vol, n, noise_pixels(600 + seed, shape, 1), int(rng.integers(1, 5))
