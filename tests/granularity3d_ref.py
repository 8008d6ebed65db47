"""
TEST INFRASTRUCTURE — the definition of `FeatureEngine.granularity3d` (aliby_amd/csrc/feat_granularity3d.hip, include/aliby_hip.h)
restated in NumPy / SciPy, and the edge cases its tests share (tests/test_cpu_granularity3d_ref.py checks, without a GPU, that the
restatement is what it says and that every case really is the edge it claims; tests/test_gpu_granularity3d.py runs the kernels).

PARITY UNPINNED: this is CellProfiler MeasureGranularity's volumetric branch as recalled, like the 2-D family
(oracle/granularity_restated.py); neither CellProfiler nor cp_measure can be run beside this package.

Per stack [Z, Y, X], everything float64 (nothing crosses from one stack of a batch into the next):
  1. shapes: subsampled = ceil(n * subsample_size) per axis when the size is below 1, else n; background = the same rule applied to
     the subsampled shape with image_sample_size (tests/granularity_cases.sampled_shape);
  2. subsample: map_coordinates(order=1) at i / subsample_size — a division, as CellProfiler writes it: i * (1 / size) differs in
     the last place and flips far-edge voxels to 0;
  3. background: resample again by image_sample_size, grey erosion then grey dilation with ball(element_size) under ndimage's
     'reflect' border, trilinear resize back at i * ((b - 1) / (s - 1)), subtract, clamp at 0;
  4. granular_spectrum_length times: erode with ball(1) under 'reflect', reconstruct by dilation under the background-subtracted
     volume (voxels outside the stack never contribute), resize to the stack's shape at i * ((s - 1) / (n - 1)), mean over each
     object's voxels;  Granularity_i = (mean_{i-1} - mean_i) * 100 / max(mean_0, eps),  mean_0 over the ORIGINAL pixels;
  5. the one deliberate departure: where the destination axis of a resize has length 1 its coordinate is 0 (CellProfiler's
     (m - 1) / (n - 1) is 0 / 0 there).  With it a stack of one plane is the 2-D family with the frame as image mask.

The image mask is the whole stack (CellProfiler's default).  Per-object means come from np.bincount (one pass whatever the number
of objects; `means="mask"` takes them as the 2-D restatement does, label by label with ndarray.mean, which is what makes the
one-plane comparison with it bitwise).

The cases (BUILDERS; each returns volume uint16 [F,Z,Y,X], pixels [F,C,Z,Y,X], counts [F], kwargs):
    nondyadic-z / -y / -x   sample size 0.7 with a critical far edge (length 61 or 121) on one axis each
    flat_background         12 x 40 x 48 at the defaults: the background grid is 1 x 3 x 3 under ball(10)
    corridor                6 x 16 x 16: a one-voxel corridor that snakes through three planes; the reconstruction carries a value
                            along more than 200 voxels, one per Jacobi sweep
    batch                   three float32 two-channel stacks of 5 x 30 x 37, the middle one without labels
    faces                   objects on every face of the stack, labels 2 and 65535 only, 65535 rows
    stride_voxels           17 x 512 x 512 at sizes 1 / 1, ball(1): more elements than one pass of the capped image grids (16384 x 256)
    stride_voxels_coarse    the same stack with the background at 0.5 and ball(2), where the reconstructions are not the zero volume
    stride_objects          two stacks of 9 x 61 x 61 whose every voxel is its own object: 66978 rows, above the object grid's 65535
"""
import functools
import time

import numpy as np
from scipy import ndimage as ndi

from tests import granularity_cases as cases2d
from tests.granularity_cases import sampled_shape, textured

RTOL = ATOL = cases2d.RTOL  # the 2-D rule, 1e-9
EPS = float(np.finfo(float).eps)


def ball(radius):
    r = int(radius)
    zz, yy, xx = np.mgrid[-r:r + 1, -r:r + 1, -r:r + 1]
    return (zz * zz + yy * yy + xx * xx) <= r * r


def names(granular_spectrum_length=16):
    return [f"Granularity_{i}" for i in range(1, granular_spectrum_length + 1)]


def geometry(shape, kw):
    """-> (stack shape, subsampled shape, background shape)"""
    sub = sampled_shape(shape, kw.get("subsample_size", 0.25))
    return tuple(int(n) for n in shape), sub, sampled_shape(sub, kw.get("image_sample_size", 0.25))


def sweep_cap(shape, kw):
    """the kernels' hard cap on the Jacobi sweeps of one reconstruction"""
    sub = geometry(shape, kw)[1]
    return sub[0] * sub[1] * sub[2] // 2 + 64


def _sample_coords(dst_shape, size):
    return np.mgrid[0:dst_shape[0], 0:dst_shape[1], 0:dst_shape[2]].astype(float) / size


def _resize_coords(src_shape, dst_shape):
    grid = np.mgrid[0:dst_shape[0], 0:dst_shape[1], 0:dst_shape[2]].astype(float)
    for ax in range(3):
        grid[ax] *= float(src_shape[ax] - 1) / float(dst_shape[ax] - 1) if dst_shape[ax] > 1 else 0.0  # (the departure: 0, not 0 / 0)
    return grid


def dilate_ball1(a):
    """grey dilation with ball(1) in which voxels outside the stack never contribute (ndi.grey_dilation(a, footprint=ball(1),
    mode="constant", cval=-inf), by shifted maxima: exact, and many times faster on the large case)"""
    out = a.copy()
    for ax in range(a.ndim):
        lo = [slice(None)] * a.ndim
        hi = [slice(None)] * a.ndim
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        np.maximum(out[hi], a[lo], out=out[hi])
        np.maximum(out[lo], a[hi], out=out[lo])
    return out


def reconstruction_by_dilation(seed, mask):
    """-> (the largest volume <= mask reachable from seed by geodesic dilations with ball(1), the sweeps that changed something)"""
    rec = np.minimum(seed, mask).astype(np.float64)
    sweeps = 0
    while True:
        grown = np.minimum(dilate_ball1(rec), mask)
        if np.array_equal(grown, rec):
            return rec, sweeps
        rec = grown
        sweeps += 1


def _means(image, labels, n, area, means):
    """mean of `image` over every label 1..n -> [n], NaN for a label without voxels"""
    with np.errstate(invalid="ignore", divide="ignore"):
        if means == "mask":
            return np.array([image[labels == l].mean() if area[l - 1] else np.nan for l in range(1, n + 1)])
        total = np.bincount(labels.ravel(), weights=image.ravel(), minlength=n + 1)[1:n + 1]
        return np.where(area > 0, total / np.maximum(area, 1), np.nan)


def granularity3d(labels, pixels, n, subsample_size=0.25, image_sample_size=0.25, element_size=10, granular_spectrum_length=16,
                  means="bincount", stats=None):
    """One stack: labels [Z,Y,X] (1..n measured, values above n ignored), pixels [Z,Y,X] -> float64 [n, L].  `stats`, a dict, receives
    "sweeps": the changing sweeps of every step's reconstruction."""
    labels = np.asarray(labels)
    orig = np.asarray(pixels).astype(np.float64)
    assert labels.shape == orig.shape and orig.ndim == 3
    L = int(granular_spectrum_length)
    out = np.full((n, L), np.nan)
    if stats is not None:
        stats["sweeps"] = []
    if n == 0:
        return out
    lab = np.where(labels <= n, labels, 0).astype(np.int64)
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:n + 1]
    shape, sub_shape, back_shape = geometry(orig.shape, dict(subsample_size=subsample_size, image_sample_size=image_sample_size))
    # 1. subsample
    pix = ndi.map_coordinates(orig, _sample_coords(sub_shape, subsample_size), order=1) if subsample_size < 1 else orig.copy()
    # 2. background
    back = ndi.map_coordinates(pix, _sample_coords(back_shape, image_sample_size), order=1) if image_sample_size < 1 else pix
    selem = ball(element_size)
    back = ndi.grey_erosion(back, footprint=selem)  # ndimage's default 'reflect' border
    back = ndi.grey_dilation(back, footprint=selem)
    if image_sample_size < 1:
        back = ndi.map_coordinates(back, _resize_coords(back_shape, sub_shape), order=1)
    pix = pix - back
    pix[pix < 0] = 0
    # 3. granular spectrum
    current = _means(orig, lab, n, area, means)
    start = np.maximum(current, EPS)
    ero = pix.copy()
    footprint = ball(1)
    up = _resize_coords(sub_shape, shape)
    for step in range(L):
        ero = ndi.grey_erosion(ero, footprint=footprint)
        rec, sweeps = reconstruction_by_dilation(ero, pix)
        if stats is not None:
            stats["sweeps"].append(sweeps)
        new = _means(ndi.map_coordinates(rec, up, order=1), lab, n, area, means)
        out[:, step] = (current - new) * 100 / start
        current = new
    return out


def expected(volume, pixels, channel, counts, stats=None, **kw):
    """volume [F,Z,Y,X], pixels [F,C,Z,Y,X], counts [F] -> float64 [sum counts, L], rows in (stack, label) order"""
    L = int(kw.get("granular_spectrum_length", 16))
    blocks, all_sweeps = [np.zeros((0, L))], []
    for f, n in enumerate(counts):
        st = {}
        blocks.append(granularity3d(volume[f], pixels[f, channel], int(n), stats=st, **kw))
        all_sweeps.append(st["sweeps"])
    if stats is not None:
        stats["sweeps"] = all_sweeps
    return np.concatenate(blocks)


# ------------------------------------------------------------------------------------------------------------------ the cases
def _blocks(shape, boxes):
    lab = np.zeros(shape, np.uint16)
    for k, box in enumerate(boxes):
        lab[box] = k + 1
    return lab


def _face_boxes(shape):
    """seven blocks: one in the interior, one on the far face of every axis, one on the near faces, one in the far corner and one
    that lies on the last plane, row and column only"""
    Z, Y, X = shape
    s = slice
    return [
        (s(Z // 3, Z // 3 + 3), s(Y // 3, Y // 3 + 3), s(X // 3, X // 3 + 3)),
        (s(Z - 3, Z), s(1, 5), s(1, 6)),
        (s(1, 4), s(Y - 3, Y), s(2, 7)),
        (s(0, 3), s(0, 4), s(X - 3, X)),
        (s(Z - 2, Z), s(Y - 2, Y), s(X - 2, X)),
        (s(Z - 1, Z), s(Y // 2, Y // 2 + 3), s(0, 3)),
        (s(0, 2), s(Y - 1, Y), s(X - 1, X)),
    ]


# name: (stack shape, the axis whose far edge is critical at 0.7)
NONDYADIC = {"z": ((61, 12, 16), 0), "y": ((10, 61, 14), 1), "x": ((9, 14, 121), 2)}
NONDYADIC_KW = dict(subsample_size=0.7, image_sample_size=0.5, element_size=3, granular_spectrum_length=4)


def nondyadic(axis_name, seed=0):
    """One textured uint16 stack, C = 1, with blocks on every far face: a last plane, row or column that wrongly reads 0 (or wrongly
    the voxel) moves their means."""
    shape, _ = NONDYADIC[axis_name]
    rng = np.random.default_rng(7000 + seed)
    lab = _blocks(shape, _face_boxes(shape))
    return lab[None], textured(rng, shape)[None, None], [int(lab.max())], dict(NONDYADIC_KW)


FLAT_KW = dict(subsample_size=0.25, image_sample_size=0.25, element_size=10, granular_spectrum_length=16)


def flat_background(seed=0):
    """12 x 40 x 48 at the defaults: subsampled (3, 10, 12), background grid (1, 3, 3).  ball(10) is longer than every axis of that
    grid, the Z axis has length 1 (its reflection folds onto one plane, its resize coordinate is the 0 of the departure)."""
    shape = (12, 40, 48)
    rng = np.random.default_rng(7100 + seed)
    lab = _blocks(shape, _face_boxes(shape))
    return lab[None], textured(rng, shape)[None, None], [int(lab.max())], dict(FLAT_KW)


CORRIDOR_KW = dict(subsample_size=1.0, image_sample_size=1.0, element_size=10, granular_spectrum_length=3)
CORRIDOR_FAR_END = 4  # label of the object at the corridor's far end


def corridor(seed=0):
    """6 x 16 x 16.  Planes 0, 3 and 5 hold the 2-D serpentine (even rows 1000, odd rows one joining voxel at alternating ends);
    (1..2, 15, 0) joins the end of plane 0 to plane 3, (4, 0, 0) the end of plane 3 to plane 5: one corridor of 1000, one voxel wide.
    A 2 x 5 x 5 blob of 3000 on planes 0-1 at its start survives the erosion (the reflect border stands in for the missing plane);
    the bumps do not.  Objects: the blob, a stretch of plane 0, of plane 3 and of the last row of plane 5."""
    del seed
    n = 16
    px = np.zeros((6, n, n), np.uint16)
    for z in (0, 3, 5):
        px[z, 0::2] = 1000
        for k, y in enumerate(range(1, n, 2)):
            px[z, y, n - 1 if k % 2 == 0 else 0] = 1000
    px[1:3, 15, 0] = 1000
    px[4, 0, 0] = 1000
    px[0:2, 2:7, 2:7] = 3000
    px[0, 10, 9] = 1500
    px[3, 8, 5:7] = 1700
    px[5, 14, 11] = 1400
    lab = np.zeros((6, n, n), np.uint16)
    lab[0:2, 2:7, 2:7] = 1
    lab[0, 10, 3:13] = 2
    lab[3, 8, 3:13] = 3
    lab[5, 14, 3:13] = CORRIDOR_FAR_END
    return lab[None], px[None, None], [4], dict(CORRIDOR_KW)


BATCH_KW = dict(subsample_size=0.5, image_sample_size=0.5, element_size=3, granular_spectrum_length=4)


def batch(seed=0):
    """Three stacks of 5 x 30 x 37 (no multiple of 4), two channels, float32 in [0, 1]; the middle stack has no labels."""
    shape = (5, 30, 37)
    rng = np.random.default_rng(7200 + seed)
    vol = np.zeros((3,) + shape, np.uint16)
    vol[0] = _blocks(shape, _face_boxes(shape))
    vol[2] = _blocks(shape, _face_boxes(shape)[::-1][:5])
    px = np.stack([np.stack([textured(rng, shape) for _ in range(2)]) for _ in range(3)])
    return vol, (px / 65535.0).astype(np.float32), [7, 0, 5], dict(BATCH_KW)


FACES_KW = dict(subsample_size=1.0, image_sample_size=0.5, element_size=1, granular_spectrum_length=2)


def faces(seed=0):
    """6 x 12 x 16: label 2 touches the three near faces, label 65535 the three far ones; counts = 65535, so all other rows are absent."""
    shape = (6, 12, 16)
    rng = np.random.default_rng(7300 + seed)
    lab = np.zeros(shape, np.uint16)
    lab[0:3, 0:6, 0:8] = 2
    lab[3:6, 6:12, 8:16] = 65535
    return lab[None], textured(rng, shape)[None, None], [65535], dict(FACES_KW)


STRIDE_VOXELS_SHAPE = (17, 512, 512)
STRIDE_VOXELS_KW = dict(subsample_size=1.0, image_sample_size=1.0, element_size=1, granular_spectrum_length=2)


def stride_voxels(seed=0):
    """One stack of 17 x 512 x 512, uint16, C = 1: a smooth ramp (2000 + z + y + 2 x: every reconstruction needs a few sweeps only) with
    isolated specks on 0.5 % of the voxels.  Labels: blocks of 4 x 16 x 16 in raster order (5120 of them; the last layer is one plane)."""
    Z, Y, X = STRIDE_VOXELS_SHAPE
    rng = np.random.default_rng(7400 + seed)
    zz, yy, xx = np.ogrid[0:Z, 0:Y, 0:X]
    px = (2000 + zz + yy + 2 * xx).astype(np.float64)
    specks = rng.random((Z, Y, X)) < 0.005
    px[specks] += rng.integers(500, 3000, int(specks.sum()))
    lab = ((zz // 4) * (Y // 16) * (X // 16) + (yy // 16) * (X // 16) + xx // 16 + 1).astype(np.uint16)
    return lab[None], px.astype(np.uint16)[None, None], [int(lab.max())], dict(STRIDE_VOXELS_KW)


STRIDE_VOXELS_COARSE_KW = dict(subsample_size=1.0, image_sample_size=0.5, element_size=2, granular_spectrum_length=1)


def stride_voxels_coarse(seed=0):
    """The stack of `stride_voxels` with a coarser background.  At sizes 1 / 1 the background of ball(1) is the opening by the very
    footprint the spectrum erodes with, and the erosion of f - opening(f) is 0 for every f (at a voxel y of B_x the residual is at
    most f(y) - min f over B_x, whose minimum over B_x is 0): every reconstruction of `stride_voxels` is the zero volume and its
    rows are [100, 0].  Here the sweeps, the subtraction and the means run past the first pass of their grids on a volume that is
    not zero."""
    if seed:
        return stride_voxels(seed)[:3] + (dict(STRIDE_VOXELS_COARSE_KW),)
    return case("stride_voxels")[:3] + (dict(STRIDE_VOXELS_COARSE_KW),)


STRIDE_OBJECTS_SHAPE = (9, 61, 61)
STRIDE_OBJECTS_KW = dict(subsample_size=1.0, image_sample_size=0.5, element_size=2, granular_spectrum_length=2)


def stride_objects(seed=0):
    """Two textured stacks of 9 x 61 x 61 whose every voxel is its own object, numbered in raster order: 2 x 33489 rows."""
    shape = STRIDE_OBJECTS_SHAPE
    rng = np.random.default_rng(7500 + seed)
    n = int(np.prod(shape))
    lab = np.arange(1, n + 1, dtype=np.uint16).reshape(shape)
    vol = np.stack([lab, lab[::-1, ::-1, ::-1]])
    px = np.stack([textured(rng, shape), textured(rng, shape)])[:, None]
    return vol, px, [n, n], dict(STRIDE_OBJECTS_KW)


SMALL = {
    **{f"nondyadic-{k}": (lambda seed=0, k=k: nondyadic(k, seed)) for k in NONDYADIC},
    "flat_background": flat_background, "corridor": corridor, "batch": batch, "faces": faces,
}
BUILDERS = {**SMALL, "stride_voxels": stride_voxels, "stride_voxels_coarse": stride_voxels_coarse, "stride_objects": stride_objects}


@functools.lru_cache(maxsize=None)
def case(name):
    """the case `name` at seed 0, built once and shared (read-only)"""
    vol, px, counts, kw = BUILDERS[name]()
    vol.setflags(write=False)
    px.setflags(write=False)
    return vol, px, tuple(counts), kw


@functools.lru_cache(maxsize=None)
def reference(name, channel=0):
    """-> (the restatement's rows for `channel` of case `name`, its sweeps [stack][step], the seconds it took), computed once"""
    vol, px, counts, kw = case(name)
    stats = {}
    t0 = time.perf_counter()
    want = expected(vol, px, channel, counts, stats=stats, **kw)
    seconds = time.perf_counter() - t0
    want.setflags(write=False)
    return want, stats["sweeps"], seconds


def tolerance_bound(volume, pixels, counts):
    """100 * 2^-53 * (2 * area_max + 260) * (max pixel / min start), over the present objects that are not all-zero (those are exact
    on both sides), every channel and every stack.

    The argument is granularity_cases.tolerance_bound's, with the terms counted for three axes.  Both sides work in float64 and take
    the same decisions (the same floor, the same inside test on the same quotient i / size; min, max and the clamp are exact and do
    not expand an error), so they differ only in the order of the sums and of the interpolation's products.  With u = 2^-53 and M
    the largest pixel, which bounds every intermediate image:
      * one trilinear value: SciPy sums eight products of three weights and a voxel, the kernel nests three blends; either is within
        about 12 u M of the exact value, the two within 24 u M of each other;
      * a voxel of a resized reconstruction has been through the subsampling (24), the background's resampling, its resize back and
        the subtraction (24 + 24 + 2), and the resize to the stack (24): under 128 u M;
      * a mean of `area` such terms carries at most area u M more from the sum in any order: (area + 128) u M per mean, two means in
        a granularity, and 4 u M for the subtraction, the product and the quotient;
      * times 100 / start.
    An absolute bound on the difference of the two sides; the tests' ATOL must stay above it."""
    worst = 0.0
    for f, n in enumerate(counts):
        lab = np.where(volume[f] <= n, volume[f], 0).astype(np.int64).ravel()
        if not lab.any():
            continue
        area = np.bincount(lab, minlength=n + 1)[1:]
        for c in range(pixels.shape[1]):
            px = pixels[f, c].astype(np.float64)
            start = np.bincount(lab, weights=px.ravel(), minlength=n + 1)[1:][area > 0] / area[area > 0]
            start = start[start > 0]
            if len(start):
                worst = max(worst, (2 * int(area.max()) + 260) * float(px.max()) / float(start.min()))
    return 100 * 2.0 ** -53 * worst
