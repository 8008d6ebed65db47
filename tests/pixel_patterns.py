"""
Pixel-value edge cases for the 2-D per-channel feature kernels (k_intensity, k_texture, k_radial_stats, the weighted Zernike
kernel, k_ranks, k_coloc, k_coloc_pairs): objects whose pixels are all zero, flat, saturated, two-valued, tied, or only 1 to 5
in number.  The shapes are ordinary; what is degenerate here is the values.  Shared by tests/test_cpu_intensity_ref.py (which
checks the preconditions stated below without a GPU) and tests/test_gpu_pixel_patterns.py.

`tiles()`: two tiles of 64 x 96, three channels, uint16.  Channel 2 is a copy of channel 0, so the pair (0, 2) is a pair of
identical channels (Pearson 1, slope 1, RWC equal to Manders).  No object is larger than 20 x 20.  Background pixels hold 777, a
value no object has in that place, so a kernel that reads a pixel outside its object shows.

Tile 0: eight ellipses of 187 pixels (radii 7.3 x 8.1, a box of 15 x 17), `ELLIPSES[k]` is label k + 1:

    zero          0 in every channel
    flat          1234 in every channel
    saturated     65535 in every channel
    two_level     channel 0: 100 left of column cx - 2, else 300; channel 1: 7 above row cy + 1, else 9
    one_bright    0, but one pixel of 500 in channel 0 and ANOTHER pixel of 40 in channel 1 (bright in disjoint pixels)
    plateau       channel 0: 1000 with a 3 x 5 block of 2000 off-centre (rows cy - 3 .. cy - 1, columns cx + 1 .. cx + 5: several
                  maxima, none in the box's last row); channel 1: a ramp, 10 + 3 * raster rank
    ramp          channel 0: 1 + raster rank (all distinct); channel 1: the same values in reverse (Pearson -1)
    checkerboard  channel 0: 0 / 65535 by the parity of y + x; channel 1: the complement

Tile 1: the tiny objects of `TINY` (label = position + 1; value lists are in raster order), label 9, which is absent (its row is
NaN everywhere), an object in the frame's last corner (label 10), and "block" (label 11): 20 x 20, flat 3000 in channel 0, and
100 - (raster rank mod 256) // 16 in channel 1.  Areas 1 to 5 put every quartile index N q on both sides of the `qi < N - 1`
branch with a fractional part of 0, .25, .5 and .75.  The block's box has more pixels than the largest workgroup has threads
(256), and its maxima sit at box positions i and i + 256: a thread that walks the box with a stride of 64, 128 or 256 meets two
tied maxima itself, where in the ellipses (a box of 255 pixels) a 256-thread workgroup leaves every tie to the reduction.
"""
import functools

import numpy as np

SHAPE = (64, 96)
BACKGROUND = 777
RY, RX = 7.3, 8.1
ELLIPSES = ("zero", "flat", "saturated", "two_level", "one_bright", "plateau", "ramp", "checkerboard")
# name, top-left corner (y, x), shape, channel 0 values, channel 1 values (raster order)
TINY = (
    ("one_zero", (3, 3), (1, 1), (0,), (0,)),
    ("one_pixel", (3, 8), (1, 1), (321,), (45,)),
    ("pair", (8, 3), (1, 2), (5, 9), (3, 4)),
    ("triple", (12, 3), (1, 3), (5, 5, 9), (1, 2, 3)),
    ("four", (16, 3), (1, 4), (7, 1, 12, 4), (2, 8, 3, 5)),
    ("five", (20, 3), (1, 5), (1, 2, 3, 4, 5), (5, 4, 3, 2, 1)),
    ("square", (24, 3), (2, 2), (4, 4, 4, 8), (0, 0, 0, 1)),
)
PLUS = ("plus", (30, 10), (11, 13, 40, 17, 19), (5, 4, 9, 2, 7))  # centre (y, x); top, left, centre, right, bottom
ABSENT_LABEL = 9
CORNER_LABEL = 10
BLOCK_LABEL = 11
BLOCK = (slice(2, 22), slice(40, 60))
COUNTS = (len(ELLIPSES), BLOCK_LABEL)


def ellipse_centre(k):
    return 14 + 30 * (k // 4), 12 + 24 * (k % 4)


def label_of(name):
    """-> (tile, label) of a named object"""
    if name in ELLIPSES:
        return 0, ELLIPSES.index(name) + 1
    names = [t[0] for t in TINY] + [PLUS[0]]
    if name in names:
        return 1, names.index(name) + 1
    assert name in ("corner", "block"), name
    return 1, CORNER_LABEL if name == "corner" else BLOCK_LABEL


def row_of(name):
    """-> the object's row in a table of both tiles, tile after tile"""
    tile, label = label_of(name)
    return (COUNTS[0] if tile else 0) + label - 1


@functools.lru_cache(maxsize=None)
def tiles():
    """-> labels uint16 [2, 64, 96], pixels uint16 [2, 3, 64, 96], rows per tile.  Read-only."""
    lab = np.zeros((2, *SHAPE), np.uint16)
    px = np.full((2, 3, *SHAPE), BACKGROUND, np.uint16)
    yy, xx = np.mgrid[0:SHAPE[0], 0:SHAPE[1]]
    for k, name in enumerate(ELLIPSES):
        cy, cx = ellipse_centre(k)
        m = ((yy - cy) / RY) ** 2 + ((xx - cx) / RX) ** 2 <= 1.0
        lab[0][m] = k + 1
        n = int(m.sum())
        rank = np.arange(n)
        y, x = yy[m], xx[m]
        if name == "zero":
            c0 = c1 = np.zeros(n, int)
        elif name == "flat":
            c0 = c1 = np.full(n, 1234)
        elif name == "saturated":
            c0 = c1 = np.full(n, 65535)
        elif name == "two_level":
            c0, c1 = np.where(x < cx - 2, 100, 300), np.where(y < cy + 1, 7, 9)
        elif name == "one_bright":
            c0, c1 = np.where((y == cy - 2) & (x == cx + 3), 500, 0), np.where((y == cy + 1) & (x == cx - 2), 40, 0)
        elif name == "plateau":
            c0 = np.where((y >= cy - 3) & (y <= cy - 1) & (x >= cx + 1) & (x <= cx + 5), 2000, 1000)
            c1 = 10 + 3 * rank
        elif name == "ramp":
            c0, c1 = 1 + rank, n - rank
        else:
            assert name == "checkerboard"
            c0 = np.where((y + x) & 1, 65535, 0)
            c1 = 65535 - c0
        px[0, 0][m], px[0, 1][m] = c0, c1
    for k, (name, (y0, x0), (h, w), c0, c1) in enumerate(TINY):
        lab[1, y0:y0 + h, x0:x0 + w] = k + 1
        px[1, 0, y0:y0 + h, x0:x0 + w] = np.reshape(c0, (h, w))
        px[1, 1, y0:y0 + h, x0:x0 + w] = np.reshape(c1, (h, w))
    _, (cy, cx), c0, c1 = PLUS
    for j, (dy, dx) in enumerate(((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))):
        lab[1, cy + dy, cx + dx] = len(TINY) + 1
        px[1, 0, cy + dy, cx + dx], px[1, 1, cy + dy, cx + dx] = c0[j], c1[j]
    assert len(TINY) + 1 == ABSENT_LABEL - 1
    corner = (slice(SHAPE[0] - 3, SHAPE[0]), slice(SHAPE[1] - 4, SHAPE[1]))  # 3 x 4, the frame's last pixel included
    lab[1][corner] = CORNER_LABEL
    rank = np.arange(12)
    px[1, 0][corner] = (50 + rank * 37 % 101).reshape(3, 4)
    px[1, 1][corner] = (20 + rank * 53 % 97).reshape(3, 4)
    lab[1][BLOCK] = BLOCK_LABEL
    px[1, 0][BLOCK] = 3000
    px[1, 1][BLOCK] = (100 - (np.arange(400) % 256) // 16).reshape(20, 20)
    px[:, 2] = px[:, 0]
    assert [int(lab[f].max()) for f in range(2)] == list(COUNTS) and not (lab[1] == ABSENT_LABEL).any()
    for a in (lab, px):
        a.setflags(write=False)
    return lab, px, COUNTS


@functools.lru_cache(maxsize=None)
def full_frame():
    """-> labels uint16 [1, 12, 16] (all 1), pixels uint16 [1, 3, 12, 16], rows per tile.  Read-only."""
    lab = np.ones((1, 12, 16), np.uint16)
    rank = np.arange(12 * 16).reshape(12, 16)
    px = np.stack([1 + 7 * rank, 40000 - 11 * rank, 1 + 7 * rank]).astype(np.uint16)[None]
    for a in (lab, px):
        a.setflags(write=False)
    return lab, px, (1,)


SCENES = {"tiles": tiles, "full_frame": full_frame}
MODES = ("u16", "f32")


@functools.lru_cache(maxsize=None)
def planes(name, mode):
    """The pixels of scene `name` as uint16 or as float32 in [0, 1] (u16 / 65535, CellProfiler's scaling).  Read-only."""
    px = SCENES[name]()[1]
    if mode == "f32":
        px = (px.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
        px.setflags(write=False)
    else:
        assert mode == "u16"
    return px
