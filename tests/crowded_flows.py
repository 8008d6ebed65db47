"""
Crowded inputs for the mask dynamics (aliby_amd/csrc/dynamics.hip): grids of small squares (cubes) with distinct labels, one
pixel apart, turned into network-scale flows by synth.analytic_flows / analytic_flows_3d.  Every pattern is built to put one
kernel of the dynamics past a capacity above which it works in several passes; tests/test_cpu_crowded_flows.py holds that the
CPU restatement alone gives the count each pattern is named for, tests/test_gpu_dynamics_crowded.py compares the kernels with
it.  The restatement's outputs are cached per pattern and read-only.
"""

from __future__ import annotations

import functools
from unittest import mock

import numpy as np

from aliby_amd import synth
from oracle import cellpose_restated as cr
from tests import cellpose3d_ref as ref3

BACKGROUND = np.float32(-6.0)


# ------------------------------------------------------------------------------------------------ label grids
def _starts(length, side, pitch, offset):
    return list(range(offset, length - side + 1, pitch))


def grid_labels(shape, side, pitch, offset=(1, 1), small=None, n_max=None, skip=None):
    """Squares of `side` at `pitch` from `offset`, whole inside the frame, numbered in raster order.
    small = (every, at, side2): square number k (0-based) with k % every == at has side2 instead;
    n_max: only the first n_max squares; skip: boolean [Y,X], squares touching it are left out."""
    Y, X = shape
    gt = np.zeros(shape, np.int32)
    k = n = 0
    for y in _starts(Y, side, pitch, offset[0]):
        for x in _starts(X, side, pitch, offset[1]):
            s = small[2] if small and k % small[0] == small[1] else side
            k += 1
            if skip is not None and skip[y : y + side, x : x + side].any():
                continue
            if n_max is not None and n >= n_max:
                return gt
            n += 1
            gt[y : y + s, x : x + s] = n
    return gt


def quad_grid_labels(shape, big_every, big_at):
    """Cells of pitch 12: one 11 x 11 square where cell number % big_every == big_at, else four 5 x 5 squares at pitch 6."""
    Y, X = shape
    gt = np.zeros(shape, np.int32)
    c = n = 0
    for y in _starts(Y, 11, 12, 1):
        for x in _starts(X, 11, 12, 1):
            if c % big_every == big_at:
                n += 1
                gt[y : y + 11, x : x + 11] = n
            else:
                for dy in (0, 6):
                    for dx in (0, 6):
                        n += 1
                        gt[y + dy : y + dy + 5, x + dx : x + dx + 5] = n
            c += 1
    return gt


def grid_labels_3d(shape, n_max=None, big=None):
    """Cubes of side 3 at pitch 4 from offset 1.  big = (every, at): the 2 x 2 block of cubes number c (in-plane blocks of pitch
    8, counted per layer) with c % every == at is one 3 x 7 x 7 box instead."""
    Z, Y, X = shape
    gt = np.zeros(shape, np.int32)
    n = 0
    if big is None:
        for z in _starts(Z, 3, 4, 1):
            for y in _starts(Y, 3, 4, 1):
                for x in _starts(X, 3, 4, 1):
                    if n_max is not None and n >= n_max:
                        return gt
                    n += 1
                    gt[z : z + 3, y : y + 3, x : x + 3] = n
        return gt
    c = 0
    for z in _starts(Z, 3, 4, 1):
        for y in _starts(Y, 7, 8, 1):
            for x in _starts(X, 7, 8, 1):
                if c % big[0] == big[1]:
                    n += 1
                    gt[z : z + 3, y : y + 7, x : x + 7] = n
                else:
                    for dy in (0, 4):
                        for dx in (0, 4):
                            n += 1
                            gt[z : z + 3, y + dy : y + dy + 3, x + dx : x + dx + 3] = n
                c += 1
    return gt


def disc(shape, cy, cx, r):
    yy, xx = np.mgrid[0 : shape[0], 0 : shape[1]]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def with_holes(gt, prob, every):
    """A one-pixel background hole at the interior pixel (+1, +1) of every `every`-th square (off the centre, where the points
    of the square gather)."""
    prob = prob.copy()
    for lab, sl in enumerate(_find_objects(gt), start=1):
        if lab % every == 0:
            prob[sl[0].start + 1, sl[1].start + 1] = BACKGROUND
    return prob


def _find_objects(gt):
    from scipy import ndimage as ndi

    return ndi.find_objects(gt)


# ------------------------------------------------------------------------------------------------ patterns
# name -> (builder of (gt, dP, prob), keywords of compute_masks, masks the restatement gives).  The counts are the restatement's
# (tests/test_cpu_crowded_flows.py), not derived from the geometry.
def _plain(gt):
    return (gt, *synth.analytic_flows(gt))


def _noisy(gt, every):
    """The flows of every `every`-th square replaced by N(0, 4) noise: the flow QC has something to remove."""
    gt, dP, prob = _plain(gt)
    rng = np.random.default_rng(7)
    bad = (gt > 0) & (gt % every == 0)
    dP = dP.copy()
    dP[:, bad] = rng.normal(0, 4, size=(2, int(bad.sum()))).astype(np.float32)
    return gt, dP, prob


def _qc_crowd():
    """One disc whose padded box (95 x 95 cells x 17 bytes = 153 KB) passes the LDS of the diffusion, with a one-pixel hole,
    beside 360 squares, every third with a one-pixel hole."""
    shape = (120, 216)
    big = disc(shape, 60, 160, 46)
    gt = grid_labels((120, 110), 5, 6)
    gt = np.pad(gt, ((0, 0), (0, shape[1] - gt.shape[1])))
    n_small = int(gt.max())
    gt[big] = n_small + 1
    dP, prob = synth.analytic_flows(gt)
    prob = with_holes(np.where(big, 0, gt), prob, 3)
    prob[40, 180] = BACKGROUND  # (one pixel: a wider hole stops the points behind it, and their streak opens it to the outside)
    return gt, dP, prob


def _fill_crowd():
    """One disc of radius 180 (box 361 x 361, 363 x 363 = 131 769 padded cells: past the 131 072 the hole fill keeps in LDS),
    with a one-pixel hole, and squares of side 6 at pitch 7 outside it, every third with a one-pixel hole."""
    shape = (366, 424)
    big = disc(shape, 182, 182, 180)
    gt = grid_labels(shape, 6, 7, skip=disc(shape, 182, 182, 182))
    n_small = int(gt.max())
    gt[big] = n_small + 1
    dP, prob = synth.analytic_flows(gt)
    prob = with_holes(np.where(big, 0, gt), prob, 3)
    prob[150, 200] = BACKGROUND
    return gt, dP, prob


def _one_square(shape):
    gt = np.zeros(shape, np.int32)
    gt[100:105, 90:95] = 1
    return gt


TILE256 = ((1, 1), (2, 4), (4, 2))  # offsets of the three 256 x 256 tilings

PATTERNS_2D = {
    # seeds per frame around 256 and above 1024
    "g256": (lambda: _plain(grid_labels((96, 96), 5, 6)), {}, 256),
    "g259": (lambda: _plain(grid_labels((102, 96), 5, 6, n_max=259)), {}, 259),
    "g361": (lambda: _plain(grid_labels((96, 96), 4, 5)), {}, 361),
    "g440": (lambda: _plain(grid_labels((120, 136), 5, 6)), {}, 440),
    "g1156": (lambda: _plain(grid_labels((208, 208), 5, 6)), {}, 1156),
    "g1681": (lambda: _plain(grid_labels((208, 208), 4, 5)), {}, 1681),
    # frames of very different counts, one shape
    "empty208": (lambda: _plain(np.zeros((208, 208), np.int32)), {}, 0),
    "one208": (lambda: _plain(_one_square((208, 208))), {}, 1),
    "g300_208": (lambda: _plain(grid_labels((208, 208), 5, 6, n_max=300)), {}, 300),
    # rows dropped in the middle of a long table
    "mixed1156": (lambda: _plain(grid_labels((208, 208), 5, 6, small=(3, 1, 4))), dict(min_size=20), 771),
    "noisy1156_qc": (lambda: _noisy(grid_labels((208, 208), 5, 6), 7), {}, 909),
    "noisy1156_noqc": (lambda: _noisy(grid_labels((208, 208), 5, 6), 7), dict(flow_threshold=0.0), 1016),
    "quad1102": (lambda: _plain(quad_grid_labels((208, 208), 16, 5)), dict(max_size_fraction=0.001), 1084),
    # global-scratch forms that walk several masks per workgroup
    "qc_crowd": (_qc_crowd, {}, 361),
    "fill_crowd": (_fill_crowd, dict(flow_threshold=0.0, max_size_fraction=0.9), 933),
    # more than 4 194 304 foreground pixels and 8192 masks in one call: 80 frames of these
    "t256_0": (lambda: _plain(grid_labels((256, 256), 11, 12, TILE256[0])), {}, 441),
    "t256_1": (lambda: _plain(grid_labels((256, 256), 11, 12, TILE256[1])), {}, 441),
    "t256_2": (lambda: _plain(grid_labels((256, 256), 11, 12, TILE256[2])), {}, 441),
}

PATTERNS_3D = {
    "v450": (lambda: grid_labels_3d((11, 60, 60)), {}, 450),
    "v1156": (lambda: grid_labels_3d((7, 136, 136)), {}, 1156),
    "v450_of_1156": (lambda: grid_labels_3d((7, 136, 136), n_max=450), {}, 450),
    "vmixed": (lambda: grid_labels_3d((7, 136, 136), big=(12, 5)), dict(min_size=28), 24),
}

# one frame with more seeds than uint16 labels: 256 x 257 squares.  Only ever built, never restated.
OVERFLOW_SHAPE, OVERFLOW_SIDE, OVERFLOW_PITCH = (1280, 1285), 4, 5


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(ground truth int32, dP float32, prob float32) of a pattern, read-only."""
    if name in PATTERNS_2D:
        return _frozen(*PATTERNS_2D[name][0]())
    gt = PATTERNS_3D[name][0]()
    return _frozen(gt, *synth.analytic_flows_3d(gt))


def keywords(name):
    return dict((PATTERNS_2D.get(name) or PATTERNS_3D[name])[1])


def count(name):
    return (PATTERNS_2D.get(name) or PATTERNS_3D[name])[2]


def restate_2d(dP, prob, **kw):
    """cr.compute_masks -> (labels, end points [2,Y,X], zero off the foreground): the end points are the ones its own call of
    follow_flows returned."""
    seen = []
    follow = cr.follow_flows

    def keep(*a, **k):
        seen.append(follow(*a, **k))
        return seen[-1]

    with mock.patch.object(cr, "follow_flows", keep):
        labels = cr.compute_masks(dP, prob, **kw)
    pf = np.zeros((2, *prob.shape), np.float32)
    if seen:
        (p,) = seen
        pf[(slice(None), *np.nonzero(prob > kw.get("cellprob_threshold", 0.0)))] = p
    return labels, pf


@functools.lru_cache(maxsize=None)
def restated(name, **override):
    """The restatement's (labels, end points) of a pattern with its keywords (and `override`), read-only."""
    _, dP, prob = inputs(name)
    kw = {**keywords(name), **override}
    if name in PATTERNS_2D:
        return _frozen(*restate_2d(dP, prob, **kw))
    labels, _, pf = ref3.compute_masks_3d(dP, prob, **kw)
    return _frozen(labels, pf)


def dropped_rows(before, after):
    """before: labels 1..n of a table; after: the same image with some masks removed (and the rest renumbered).  -> bool [n],
    True where mask k + 1 of `before` is gone from `after`."""
    n = int(before.max())
    alive = np.zeros(n + 1, bool)
    alive[np.unique(before[(after > 0) & (before > 0)])] = True
    return ~alive[1:]


def largest_padded_box(labels):
    """(h + 2) * (w + 2) of the largest bounding box of a label image: the cells the per-mask kernels stage."""
    return max((sl[0].stop - sl[0].start + 2) * (sl[1].stop - sl[1].start + 2) for sl in _find_objects(labels.astype(np.int64)) if sl)


def on_both_sides(dropped, row=1024):
    """Something dropped and something kept below `row` and from `row` on."""
    return bool(dropped[:row].any() and dropped[row:].any() and (~dropped[:row]).any() and (~dropped[row:]).any())


def holes(name):
    """Background pixels inside the pattern's ground truth: not followed, to be filled back by the hole fill."""
    gt, _, prob = inputs(name)
    return (gt > 0) & ~(prob > 0)
