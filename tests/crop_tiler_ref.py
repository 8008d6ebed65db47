"""
NumPy restatement of the crop tiler (aliby_amd/csrc/tile_crop.hip, aliby_amd.tile.tiler.CropTiler) and the seeded scenes its
tests share.  Written from the formulas, through the per-channel histogram as the kernels go:

    h[v]      = number of voxels of grey level v in the channel's [Z,Y,X] frame, n = sum h
    rank r    -> the smallest v with cum[v] > r (cum = inclusive prefix sum of h): the r-th order statistic
    p(q)      = NumPy's percentile, method="linear": index = (n - 1) (q / 100), lo = floor(index), t = index - lo,
                a, b = order statistics lo and min(lo + 1, n - 1); a + (b - a) t for t < 0.5, else b - (b - a) (1 - t)
    clip      x = (v - pmin) / (pmax - pmin) clipped to [0, 1], pmin = p(0.5), pmax = p(99.5)        (NaN stays NaN)
    8-bit     trunc(255 x) as uint8 (NaN -> 0) after clip; on raw integers (255 v) mod 256: NumPy multiplies in the source's
              integer type, which wraps, and then narrows
    scale     (x - mean) / std, mean = sum h g / n, std = sqrt(sum h (g - mean)^2 / n), g = the value after the stages before
    tiles     n_th = (Y - ts) // ts + 1 by n_tw = (X - ts) // ts + 1 squares in row-major order, the remainder dropped

tests/test_cpu_crop_tiler.py pins it to what the reference's own CropTiler returned (tests/golden/reference_crop_tiler.npz,
written by tests/golden/make_crop_tiler_golden.py); the GPU tests compare the kernels with it.
"""
import itertools
import math

import numpy as np

BINS = 65536
CLIP = 0.5  # clip_outliers' default, the only value CropTiler uses
COMBOS = list(itertools.product((False, True), repeat=3))  # (clip_outliers, convert_8bit, standard_scale)


def combo_name(clip, bit8, std):
    return f"clip{int(clip)}_bit{int(bit8)}_std{int(std)}"


def histogram(channel):
    return np.bincount(np.asarray(channel).ravel().astype(np.int64), minlength=BINS)


def order_statistic(cum, rank):
    return int(np.searchsorted(cum, rank, side="right"))


def percentile(h, q):
    n = int(h.sum())
    cum = np.cumsum(h)
    index = (n - 1) * (q / 100)
    lo = math.floor(index)
    t = index - lo
    a = float(order_statistic(cum, min(lo, n - 1)))
    b = float(order_statistic(cum, min(lo + 1, n - 1)))
    return a + (b - a) * t if t < 0.5 else b - (b - a) * (1 - t)


def channel_levels(h, clip, bit8, std, clip_percent=CLIP):
    """-> (value of every grey level after the stages that are on [65536], (pmin, pmax, mean, std), NaN where a stage is off)"""
    v = np.arange(BINS, dtype=np.float64)
    n = float(h.sum())
    pmin = pmax = mean = sd = np.nan
    with np.errstate(all="ignore"):
        if clip:
            if clip_percent > 0:
                pmin, pmax = percentile(h, clip_percent), percentile(h, 100 - clip_percent)
            else:
                present = np.flatnonzero(h)
                pmin, pmax = float(present[0]), float(present[-1])
            g = (v - pmin) / (pmax - pmin)
            g = np.where(g < 0, 0.0, np.where(g > 1, 1.0, g))
            if bit8:
                g = np.trunc(np.where(np.isnan(g), 0.0, g * 255))
        elif bit8:
            g = ((np.arange(BINS, dtype=np.int64) * 255) % 256).astype(np.float64)
        else:
            g = v
        if std:
            nz = np.flatnonzero(h)
            mean = float(np.sum(h[nz] * g[nz]) / n)
            sd = float(np.sqrt(np.sum(h[nz] * (g[nz] - mean) ** 2) / n))
            g = (g - mean) / sd
    return g, (pmin, pmax, mean, sd)


def out_dtype(source_dtype, clip, bit8, std):
    if std or (clip and not bit8):
        return np.dtype(np.float64)
    return np.dtype(np.uint8) if bit8 else np.dtype(source_dtype)


def normalise(pixels, clip, bit8, std, clip_percent=CLIP):
    """pixels [C,Z,Y,X] of an unsigned integer type -> (the normalised frame in the reference's dtype, stats [C,4])"""
    pixels = np.asarray(pixels)
    stats = np.empty((pixels.shape[0], 4))
    out = np.empty(pixels.shape, out_dtype(pixels.dtype, clip, bit8, std))
    for c in range(pixels.shape[0]):
        g, stats[c] = channel_levels(histogram(pixels[c]), clip, bit8, std, clip_percent)
        out[c] = g[pixels[c]]  # (integer outputs hold whole numbers in range: the cast is exact)
    return out, stats


def cut(frame, ts):
    C, Z, Y, X = frame.shape
    n_th = (Y - ts) // ts + 1 if Y >= ts else 0
    n_tw = (X - ts) // ts + 1 if X >= ts else 0
    tiles = np.empty((n_th * n_tw, C, Z, ts, ts), frame.dtype)
    for i in range(n_th):
        for j in range(n_tw):
            tiles[i * n_tw + j] = frame[:, :, i * ts:(i + 1) * ts, j * ts:(j + 1) * ts]
    return tiles


def crop_tiles(pixels, ts, standard_scale=True, convert_8bit=False, clip_outliers=False):
    frame, _ = normalise(pixels, clip_outliers, convert_8bit, standard_scale)
    return cut(frame, ts)


def rel_err(got, want, floor=1.0):
    """Largest |got - want| / max(|want|, floor) over the finite entries; NaN / inf positions must coincide (checked by the
    caller through `same_nonfinite`).  The floor: the float outputs are unit-variance or lie in [0, 1], and a value near 0 after
    the standard scale is a difference of two numbers of that size, so its error is absolute on that scale."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), floor)))


def same_nonfinite(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = ~np.isfinite(want)
    return np.array_equal(~np.isfinite(got), bad) and np.array_equal(got[bad], want[bad], equal_nan=True)


# ------------------------------------------------------------------------------------------------ scenes
def _narrow(rng, shape, lo, levels):
    return (lo + rng.integers(0, levels, shape)).astype(np.uint16)


def _two_valued(shape, low, high, n_low):
    flat = np.full(int(np.prod(shape)), high, np.uint16)
    flat[:n_low] = low
    return np.random.default_rng(n_low).permutation(flat).reshape(shape)


_SCENES = None


def scenes():
    """name -> {"pixels": [C,Z,Y,X], "ts": tile size}; built once, never modified (the arrays are read-only)."""
    global _SCENES
    if _SCENES is not None:
        return _SCENES
    out = {}
    rng = np.random.default_rng(20240611)
    # remainders dropped on both axes; neither ts nor X allows 16-byte groups
    out["ragged"] = dict(ts=16, pixels=np.stack([_narrow(rng, (2, 37, 53), 1000, 64), _narrow(rng, (2, 37, 53), 300, 200),
                                                 _narrow(rng, (2, 37, 53), 30000, 256)]))
    out["vector"] = dict(ts=32, pixels=np.stack([_narrow(rng, (1, 64, 96), 500, 150), _narrow(rng, (1, 64, 96), 40000, 100)]))
    out["exact_fit"] = dict(ts=24, pixels=_narrow(rng, (1, 1, 24, 24), 100, 300))
    out["oversized"] = dict(ts=16, pixels=_narrow(rng, (2, 1, 10, 12), 100, 300))
    # n = 1280 voxels per channel: (n - 1) 0.005 = 6.395 (t < 0.5), (n - 1) 0.995 = 1272.605 (t >= 0.5); with 7 low voxels the
    # lower percentile falls between the two values, with 7 high voxels the upper one does
    full = rng.integers(0, 65536, (1, 32, 40)).astype(np.uint16)
    full.flat[3], full.flat[77] = 0, 65535
    out["special"] = dict(ts=16, pixels=np.stack([full, np.full((1, 32, 40), 777, np.uint16),
                                                  _two_valued((1, 32, 40), 100, 900, 7), _two_valued((1, 32, 40), 100, 900, 1273)]))
    out["eight_bit"] = dict(ts=8, pixels=np.stack([rng.integers(0, 256, (2, 20, 28)), rng.integers(10, 60, (2, 20, 28))]).astype(np.uint8))
    for s in out.values():
        s["pixels"].flags.writeable = False
    _SCENES = out
    return out
