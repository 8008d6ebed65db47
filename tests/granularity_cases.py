"""
Edge cases for the granularity kernels (aliby_amd/csrc/feat_granularity.hip), shared by tests/test_cpu_granularity_cases.py
(which checks, without a GPU, that every case really is the edge it claims to be) and tests/test_gpu_granularity.py.

Every builder takes a seed, is deterministic and returns

    labels uint16 [F, Y, X],  planes [F, C, Y, X] (uint16, or float32 in [0, 1]),  kwargs of oracle.granularity_restated.get_granularity

The kwargs hold the geometry only (subsample_size, image_sample_size, element_size, granular_spectrum_length); the image mask
is the test's choice.

The cases:

    nondyadic(name)   sample sizes of 0.7, where i / 0.7 and i * (1 / 0.7) differ in the last place and, at the frame's far edge,
                      land on different sides of n - 1: bilinear sampling returns the pixel on one side and 0 on the other.
                      NONDYADIC[name] = (shape, kwargs, axes of the first sampling that are critical, axes of the second).
    overshoot(name)   shapes at which the up-resize coordinate (n - 1) * ((m - 1) / (n - 1)) rounds above m - 1, so that the
                      last frame row or column of the resized image reads 0.  The oracle and the kernel share this quirk.
    serpentine()      a 48 x 48 maze in which the reconstruction has to carry a value along a path of about half the image's
                      pixels, one pixel per Jacobi sweep.
    matrix()          three float32 frames with three channels, the middle frame without labels, shapes no multiple of 4.
    degenerate()      flat and two-level planes, all-zero objects, one-pixel objects, an absent label.
    whole_frame()     one object that is the whole frame (tests/pixel_patterns.full_frame).
    label_65535()     a frame whose only objects are labels 2 and 65535.
    stride()          17 frames of 512 x 512 with 4096 objects each: more elements than one pass of the capped image grids
                      covers (16384 x 256) and more objects than the capped object grid has blocks (65535).

`tolerance_bound` is the figure under which the GPU tests' tolerance (RTOL, ATOL) is justified, see its docstring.
"""
import numpy as np
from scipy import ndimage as ndi

from aliby_amd import synth
from tests import pixel_patterns as pp

RTOL = ATOL = 1e-9

# name: (frame shape, kwargs, critical axes of the frame -> subsampled sampling, critical axes of subsampled -> background)
NONDYADIC = {
    "sub_both": ((61, 121), dict(subsample_size=0.7, image_sample_size=0.5, element_size=3, granular_spectrum_length=4), (0, 1), ()),
    "back_both": ((62, 122), dict(subsample_size=0.5, image_sample_size=0.7, element_size=3, granular_spectrum_length=4), (), (0, 1)),
    "sub_x": ((64, 121), dict(subsample_size=0.7, image_sample_size=0.5, element_size=3, granular_spectrum_length=4), (1,), ()),
    "sub_y": ((61, 124), dict(subsample_size=0.7, image_sample_size=0.5, element_size=3, granular_spectrum_length=4), (0,), ()),
    "control": ((96, 120), dict(subsample_size=0.5, image_sample_size=0.7, element_size=3, granular_spectrum_length=4), (), ()),
}
# name: (frame shape, kwargs, axes on which frame <- subsampled overshoots, axes on which subsampled <- background overshoots)
OVERSHOOT = {
    "sub_0.2": ((80, 140), dict(subsample_size=0.2, image_sample_size=0.5, element_size=2, granular_spectrum_length=3), (0, 1), ()),
    "sub_0.1": ((160, 158), dict(subsample_size=0.1, image_sample_size=1.0, element_size=2, granular_spectrum_length=3), (0, 1), ()),
    "back_0.3": ((26, 84), dict(subsample_size=1.0, image_sample_size=0.3, element_size=2, granular_spectrum_length=3), (), (0, 1)),
}


def sampled_shape(shape, size):
    """numpy's mgrid[0 : n * size] has ceil(n * size) points"""
    return tuple(int(np.ceil(n * size)) if size < 1 else int(n) for n in shape)


def geometry(shape, kw):
    """-> (frame shape, subsampled shape, background shape)"""
    sub = sampled_shape(shape, kw.get("subsample_size", 0.25))
    return tuple(shape), sub, sampled_shape(sub, kw.get("image_sample_size", 0.25))


def textured(rng, shape):
    """Smoothed noise around 3000 with specks of up to 6000 on 2 % of the pixels: uint16 in [1000, 12000]."""
    smooth = ndi.gaussian_filter(rng.standard_normal(shape), 2.0)
    img = 3000.0 + 800.0 * smooth / smooth.std()
    specks = rng.random(shape) < 0.02
    img[specks] += rng.uniform(1000.0, 6000.0, int(specks.sum()))
    return np.clip(np.rint(img), 1000, 12000).astype(np.uint16)


def paint_border_objects(labels, first):
    """Objects on the last 6 rows and the last 5 columns of one frame (overwriting what is there): two blocks that touch the last
    row, two that touch the last column, one in the corner, one that lies on the last row only.  -> the next free label"""
    Y, X = labels.shape
    boxes = [
        (slice(Y - 6, Y), slice(4, 16)), (slice(Y - 3, Y), slice(X // 2, X // 2 + 9)),
        (slice(3, 14), slice(X - 5, X)), (slice(Y // 2, Y // 2 + 7), slice(X - 2, X)),
        (slice(Y - 6, Y), slice(X - 5, X)), (slice(Y - 1, Y), slice(20, 31)),
    ]
    for k, box in enumerate(boxes):
        labels[box] = first + k
    return first + len(boxes)


def _relabel(lab):
    """labels 1..n without gaps, in the order of the old labels"""
    old = np.unique(lab)
    old = old[old > 0]
    lut = np.zeros(int(lab.max()) + 1, np.uint16)
    lut[old] = np.arange(1, len(old) + 1)
    return lut[lab]


def nondyadic(name, seed=0):
    """Two frames of synth.make_fov (nuclei, both channels, uint16) with border objects whose pixels are brightened by a seeded
    texture, so that a last row or column that wrongly reads the pixel (or wrongly 0) moves their means.  One more, larger block
    touches the last row: with the objects as image mask the background is 0 wherever the erosion by disk(element_size) finds
    a pixel outside the mask, so only a large object at the edge lets the second sampling's last row matter."""
    shape, kw, _, _ = NONDYADIC[name]
    rng = np.random.default_rng(1000 + seed)
    labels, planes = [], []
    for f in range(2):
        fov = synth.make_fov(1, 300 + 10 * seed + f, shape=shape, n_target=8)
        lab = fov["nuclei"].copy()
        px = fov["pixels"][:, 0].copy()
        before = lab.copy()
        big = int(lab.max()) + 1
        lab[shape[0] - 22:, 36:76] = big  # wide enough to survive the background's erosion in the objects-masked variant
        paint_border_objects(lab, big + 1)
        painted = lab != before
        for c in range(px.shape[0]):
            px[c][painted] = textured(rng, shape)[painted]
        labels.append(_relabel(lab))
        planes.append(px)
    return np.stack(labels), np.stack(planes), dict(kw)


def overshoot(name, seed=0):
    """One textured uint16 frame, C = 1; border objects as in `nondyadic` plus three interior blocks."""
    shape, kw, _, _ = OVERSHOOT[name]
    rng = np.random.default_rng(2000 + seed)
    Y, X = shape
    lab = np.zeros(shape, np.uint16)
    lab[2:9, 3:12] = 1
    lab[Y // 2 - 4:Y // 2 + 3, X // 3:X // 3 + 11] = 2
    lab[5:8, X // 2:X // 2 + 20] = 3
    paint_border_objects(lab, 4)
    return _relabel(lab)[None], textured(rng, shape)[None, None], dict(kw)


SERPENTINE_KW = dict(subsample_size=1.0, image_sample_size=1.0, element_size=10, granular_spectrum_length=4)
SERPENTINE_FAR_END = 4  # label of the object at the path's far end


def serpentine(seed=0):
    """48 x 48.  Even rows hold 1000, odd rows 0 but for one joining pixel at alternating ends: a single path of 1000 through the
    whole frame.  A 5 x 5 blob of 3000 at its start survives the erosion; three one-pixel-high bumps do not.  Objects: the blob,
    and a stretch of rows 8, 24 and 46.  The reconstruction has to carry 1000 from the blob to row 46."""
    del seed  # (nothing is random here)
    n = 48
    px = np.zeros((n, n), np.uint16)
    px[0::2] = 1000
    for k, y in enumerate(range(1, n, 2)):
        px[y, n - 1 if k % 2 == 0 else 0] = 1000
    px[2:7, 2:7] = 3000
    px[8, 15] = 1500
    px[24, 20:22] = 1700
    px[46, 30] = 1400
    lab = np.zeros((n, n), np.uint16)
    lab[2:7, 2:7] = 1
    lab[8, 10:40] = 2
    lab[24, 10:40] = 3
    lab[46, 10:40] = 4
    return lab[None], px[None, None], dict(SERPENTINE_KW)


def ordinary_frame(shape, seed):
    """-> (labels, pixels [Y, X]) of an ordinary textured frame with a few blocks, for batches around a special frame"""
    rng = np.random.default_rng(3000 + seed)
    Y, X = shape
    lab = np.zeros(shape, np.uint16)
    lab[4:12, 5:17] = 1
    lab[Y // 2:Y // 2 + 9, X // 2:X // 2 + 6] = 2
    lab[Y - 9:Y - 2, 3:10] = 3
    return lab, textured(rng, shape)


MATRIX_SAMPLES = ((1.0, 1.0), (0.5, 1.0), (1.0, 0.5), (0.25, 0.25))


def matrix(seed=0):
    """Three frames of 90 x 117, three channels, float32 in [0, 1]; the middle frame has no label.  The pixels are the square root
    of synth.make_fov's (as a fraction of 65535): a dim nucleus beside a bright one would otherwise put the frame's largest pixel
    at 50 times the smallest object mean, beyond what `tolerance_bound` allows for objects of this size.  The kwargs
    carry no sample sizes: the test runs MATRIX_SAMPLES."""
    shape = (90, 117)
    labels, planes = [], []
    for f in range(3):
        fov = synth.make_fov(2, 500 + 10 * seed + f, shape=shape, n_channels=3, n_target=8)
        lab = fov["nuclei"].copy()
        if f == 1:
            lab[:] = 0
        else:
            lab[shape[0] - 4:, 30:41] = lab.max() + 1  # on the last rows
            lab = _relabel(lab)
        labels.append(lab)
        planes.append(np.sqrt(fov["pixels"][:, 0] / 65535.0).astype(np.float32))
    return np.stack(labels), np.stack(planes), dict(element_size=3, granular_spectrum_length=4)


DEGENERATE_KW = dict(subsample_size=1.0, image_sample_size=0.5, element_size=2, granular_spectrum_length=3)
DEGENERATE_ABSENT = 4  # frame 0 has no label 4
DEGENERATE_DARK = ((1, 1), (1, 2))  # (frame, label) of the all-zero objects


def degenerate(seed=0):
    """Two frames of 45 x 54, two channels, uint16.  The sample size of the frame is 1, so that an all-zero object is exactly 0
    in every reconstruction and its granularity exactly 0 (0 * 100 / eps).
    Frame 0: channel 0 is flat (1234), channel 1 holds two levels, 100 and 300, in 2 x 3 bricks.  Labels 1-3 blocks, label 4
    absent, labels 5-7 single pixels (first pixel, interior, last pixel), label 8 a block on the last column.
    Frame 1: background 777; labels 1 and 2 are all-zero objects (interior, and in the last corner), label 3 a block with the two
    levels 700 and 900, label 4 a single bright pixel."""
    del seed
    Y, X = 45, 54
    yy, xx = np.mgrid[0:Y, 0:X]
    lab = np.zeros((2, Y, X), np.uint16)
    px = np.zeros((2, 2, Y, X), np.uint16)
    px[0, 0] = 1234
    px[0, 1] = np.where((yy // 2 + xx // 3) % 2 == 0, 300, 100)
    lab[0, 3:11, 4:15] = 1
    lab[0, 20:27, 20:33] = 2
    lab[0, 30:41, 6:9] = 3
    lab[0, 0, 0] = 5
    lab[0, 17, 40] = 6
    lab[0, Y - 1, X - 1] = 7
    lab[0, 8:19, X - 3:X] = 8
    px[1] = 777
    lab[1, 10:19, 12:22] = 1
    lab[1, Y - 7:Y, X - 8:X] = 2
    px[1][:, lab[1] > 0] = 0
    lab[1, 25:35, 30:44] = 3
    px[1, 0][lab[1] == 3] = np.where((yy + xx) % 2 == 0, 900, 700)[lab[1] == 3]
    px[1, 1][lab[1] == 3] = np.where(xx < 37, 900, 700)[lab[1] == 3]
    lab[1, 5, 47] = 4
    px[1, :, 5, 47] = 5000
    return lab, px, dict(DEGENERATE_KW)


def whole_frame(seed=0):
    """One object equal to the whole 12 x 16 frame, three channels (tests/pixel_patterns.full_frame)."""
    del seed
    lab, px, _ = pp.full_frame()
    return lab, px, dict(subsample_size=0.5, image_sample_size=0.5, element_size=1, granular_spectrum_length=3)


def label_65535(seed=0):
    """A 12 x 16 textured frame whose objects are labels 2 and 65535: a table of 65535 rows, all but two of them absent."""
    rng = np.random.default_rng(4000 + seed)
    lab = np.zeros((12, 16), np.uint16)
    lab[2:6, 3:9] = 2
    lab[8:12, 10:16] = 65535
    return lab[None], textured(rng, (12, 16))[None, None], dict(subsample_size=1.0, image_sample_size=0.5, element_size=1,
                                                                 granular_spectrum_length=1)


STRIDE_FRAMES, STRIDE_SIDE, STRIDE_BLOCK = 17, 512, 8
STRIDE_KW = dict(subsample_size=1.0, image_sample_size=0.5, element_size=3, granular_spectrum_length=2)
STRIDE_ORACLE_FRAMES = (0, 16)


def stride(seed=0):
    """17 frames of 512 x 512, uint16, C = 1.  Every frame's labels are its 4096 blocks of 8 x 8, numbered in raster order.
    The pixels are three seeded textured planes, rolled by another amount in every frame, so that no two frames are equal."""
    rng = np.random.default_rng(5000 + seed)
    n, b = STRIDE_SIDE, STRIDE_BLOCK
    base = [textured(rng, (n, n)) for _ in range(3)]
    by, bx = np.mgrid[0:n, 0:n] // b
    lab = (by * (n // b) + bx + 1).astype(np.uint16)
    labels = np.broadcast_to(lab, (STRIDE_FRAMES, n, n)).copy()
    planes = np.stack([np.roll(base[f % 3], (7 * f + 3, 11 * f + 5), axis=(0, 1)) for f in range(STRIDE_FRAMES)])[:, None]
    return labels, planes, dict(STRIDE_KW)


def stride_subset(seed=0, count=256):
    """-> sorted block labels of `stride` that the oracle is run for (it loops over every label of a full-frame mask, which for
    4096 labels of 512 x 512 takes a quarter of a minute per frame; with the whole frame as image mask an object's result does
    not depend on the other labels): the four corner blocks, the blocks around them, and a seeded draw of the others."""
    side = STRIDE_SIDE // STRIDE_BLOCK
    fixed = {1, 2, side - 1, side, side + 1, 2 * side, side * (side - 2) + 1, side * (side - 1) + 1, side * (side - 1) + 2,
             side * side - 1, side * side, side * (side - 1), side * (side - 1) - 1, side * side - side + 32}
    rng = np.random.default_rng(6000 + seed)
    rest = [int(v) for v in rng.permutation(np.arange(1, side * side + 1)) if int(v) not in fixed]
    return sorted(fixed | set(rest[:count - len(fixed)]))


def subset_labels(lab, keep):
    """a frame's labels with only `keep` (sorted) left, renumbered 1..len(keep) in that order"""
    lut = np.zeros(int(lab.max()) + 1, np.uint16)
    lut[np.asarray(keep)] = np.arange(1, len(keep) + 1)
    return lut[lab]


BUILDERS = {
    **{f"nondyadic-{k}": (lambda seed=0, k=k: nondyadic(k, seed)) for k in NONDYADIC},
    **{f"overshoot-{k}": (lambda seed=0, k=k: overshoot(k, seed)) for k in OVERSHOOT},
    "serpentine": serpentine, "matrix": matrix, "degenerate": degenerate, "whole_frame": whole_frame, "label_65535": label_65535,
    "stride": stride,
}


def tolerance_bound(labels, planes, frames=None):
    """4 * 100 * area_max * 2^-53 * (max pixel / min start), over the present objects that are not all-zero (those are compared
    exactly), every channel, and the given frames (all by default).

    Both sides work in float64 and differ only in the order of sums and of the interpolation's products.  A mean of `area` terms
    of at most `max pixel` carries an error of at most area * 2^-53 * max pixel in any order; a granularity is the difference of
    two such means times 100 / start, and the factor 4 covers the two means and the bilinear products behind their terms."""
    worst_area, worst_ratio = 0, 0.0
    for f in (range(labels.shape[0]) if frames is None else frames):
        lab = labels[f]
        if not lab.any():
            continue
        area = np.bincount(lab.ravel())[1:]
        for c in range(planes.shape[1]):
            px = planes[f, c].astype(np.float64)
            start = np.bincount(lab.ravel(), weights=px.ravel())[1:][area > 0] / area[area > 0]
            start = start[start > 0]
            if len(start):
                worst_ratio = max(worst_ratio, float(px.max()) / float(start.min()))
        worst_area = max(worst_area, int(area.max()))
    return 4 * 100 * worst_area * 2.0 ** -53 * worst_ratio
