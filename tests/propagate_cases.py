"""Scenes for the `propagate` tests (tests/test_cpu_propagate_ref.py, tests/test_gpu_propagate.py): seeds plus a stain."""

from __future__ import annotations

import numpy as np


def scene(shape, n_seeds, seed, noise=800, islands=0):
    """(primary uint16 [F,Y,X], image uint16 [F,Y,X]): small seeds of mixed labels, a Gaussian blob of stain around each, noise;
    `islands` more blobs per tile that hold no seed, far from the seeds (under a threshold: passable pixels that nothing reaches)."""
    rng = np.random.default_rng(seed)
    F, Y, X = shape
    primary = np.zeros(shape, np.uint16)
    image = np.zeros(shape, np.float64)
    yy, xx = np.mgrid[0:Y, 0:X]
    pool = np.concatenate([np.arange(1, 30), [255, 256, 4097, 65534, 65535]])
    for _ in range(n_seeds):
        f, y, x = rng.integers(0, F), rng.integers(0, Y), rng.integers(0, X)
        h, w = rng.integers(1, 4, 2)
        primary[f, y:y + h, x:x + w] = rng.choice(pool)
        s = rng.uniform(3, 9)
        image[f] += rng.uniform(8000, 30000) * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s))
    for f in range(F):  # each island where the tile is farthest from its seeds and from the islands before it
        far = np.full((Y, X), np.inf)
        for y, x in zip(*np.nonzero(primary[f])):
            far = np.minimum(far, (yy - y) ** 2 + (xx - x) ** 2)
        for _ in range(islands):
            y, x = np.unravel_index(np.argmax(far), far.shape)
            image[f] += 20000 * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * 2.0 * 2.0))
            far = np.minimum(far, (yy - y) ** 2 + (xx - x) ** 2)
    image += rng.uniform(0, noise, shape)
    return primary, np.clip(image, 0, 65535).astype(np.uint16)


def flat(shape, value=1000):
    return np.full(shape, value, np.uint16)


def at(shape, *pixels):
    lab = np.zeros(shape, np.uint16)
    for (y, x), v in pixels:
        lab[0, y, x] = v
    return lab


def serpentine(Y, X, pitch, label=5, high=20000):
    """A corridor of `pitch - 1` rows that runs the whole width, turns at the end and comes back, down the whole tile: walls of 0
    under a threshold of 1, the seed in the top left corner.  The one path to the last row is about (Y / pitch) * X steps long."""
    image = np.full((1, Y, X), high, np.uint16)
    for k, y in enumerate(range(pitch - 1, Y, pitch)):
        image[0, y, :] = 0
        if k % 2 == 0:
            image[0, y, X - 2:] = high  # the gap: right, then left, ...
        else:
            image[0, y, :2] = high
    return at((1, Y, X), ((0, 0), label)), image


def ridge(Y=21, X=40, col=12):
    """Two seeds at either end of the middle row, a bright vertical ridge at column `col`, off the midline."""
    image = flat((1, Y, X), 2000)
    image[0, :, col] = 30000
    return at((1, Y, X), ((Y // 2, 0), 4), ((Y // 2, X - 1), 9)), image


def wall(Y=40, X=70):
    """A seed on the left, a dark wall at column 30 from top to bottom, a bright island right of it with no seed."""
    image = flat((1, Y, X), 5000)
    image[0, :, 30] = 10
    image[0, :, 50:] = 10
    image[0, 10:20, 55:65] = 9000  # the island: above the threshold, beyond two dark bands
    return at((1, Y, X), ((20, 5), 3)), image


def checkerboard(Y=37, X=53):
    yy, xx = np.mgrid[0:Y, 0:X]
    image = (((yy + xx) % 2) * 65535).astype(np.uint16)[None]
    return at((1, Y, X), ((3, 4), 8), ((30, 40), 2), ((18, 50), 65535)), image


def gradient(Y=37, X=53):
    """A stain that rises into every edge of the tile (the clamp decides the border weights), seeds in the corners and the middle."""
    yy, xx = np.mgrid[0:Y, 0:X]
    image = (np.abs(yy - Y // 2) * 900 + np.abs(xx - X // 2) * 700 + (yy * xx) % 97).astype(np.uint16)[None]
    return at((1, Y, X), ((0, 0), 3), ((0, X - 1), 1), ((Y - 1, 0), 65535), ((Y - 1, X - 1), 2), ((Y // 2, X // 2), 7)), image
