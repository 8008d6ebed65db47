"""Restatement of the automatic threshold (include/aliby_hip.h, csrc/feat_threshold.hip): Otsu's threshold of one uint16 tile, with
two or three classes, a correction factor and bounds.  The definition is stated twice — `otsu_loop`, a plain Python loop over the
candidates in Python ints and floats, and `otsu_numpy`, vectorised — and tests/test_cpu_threshold_ref.py holds the two against each
other bit for bit.  Every float64 operation is written out one by one, in the order the kernel uses: squares, then the quotients, then
the sums from the left.  Nothing here imports the package."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

LEVELS = 65536
BINS = 256


class Otsu(NamedTuple):
    threshold: int  # after correction and bounds
    lo: int
    hi: int
    t1: int  # raw; with two classes t1 == t2
    t2: int

    @property
    def details(self) -> tuple:
        return (self.lo, self.hi, self.t1, self.t2)


def histogram(tile) -> np.ndarray:
    """h[v] of one uint16 tile of any shape, int64 [65536]."""
    tile = np.asarray(tile)
    assert tile.dtype == np.uint16, tile.dtype
    return np.bincount(tile.reshape(-1), minlength=LEVELS).astype(np.int64)


def finish(t: int, correction=1.0, bounds=(0, 65535)) -> int:
    """T = min(max(rint(min(t * correction, 65535.0)), bound_lo), bound_hi): the product in float64, the rounding half to even."""
    scaled = min(float(t) * float(correction), 65535.0)
    return int(min(max(int(np.rint(scaled)), int(bounds[0])), int(bounds[1])))


# ------------------------------------------------------------------------------------------------ the plain loop
def _two_loop(h, lo, hi) -> int:
    if lo == hi:
        return lo
    total_n = sum(int(c) for c in h)
    total_s = sum(v * int(c) for v, c in enumerate(h))
    best_j, best_t = -1.0, None
    n0 = s0 = 0
    for t in range(lo + 1, hi + 1):  # class 0 = {v < t}
        n0 += int(h[t - 1])
        s0 += (t - 1) * int(h[t - 1])
        n1, s1 = total_n - n0, total_s - s0
        j = float(s0) * float(s0) / float(n0) + float(s1) * float(s1) / float(n1)
        if j > best_j:  # (strictly: the smallest t that attains the maximum)
            best_j, best_t = j, t
    return best_t


def _three_loop(h, lo, hi):
    width = hi - lo + 1
    bin_n, bin_s = [0] * BINS, [0] * BINS
    for v in range(lo, hi + 1):
        b = ((v - lo) * BINS) // width
        bin_n[b] += int(h[v])
        bin_s[b] += v * int(h[v])
    total_n, total_s = sum(bin_n), sum(bin_s)
    best_j, best = -1.0, None
    n0 = s0 = 0
    for k1 in range(0, BINS - 2):
        n0 += bin_n[k1]
        s0 += bin_s[k1]
        n01, s01 = n0, s0
        for k2 in range(k1 + 1, BINS - 1):
            n01 += bin_n[k2]
            s01 += bin_s[k2]
            n1, s1, n2, s2 = n01 - n0, s01 - s0, total_n - n01, total_s - s01
            if n0 == 0 or n1 == 0 or n2 == 0:
                continue
            j = float(s0) * float(s0) / float(n0) + float(s1) * float(s1) / float(n1) + float(s2) * float(s2) / float(n2)
            if j > best_j:  # (k1 ascending, then k2 ascending: the first to attain the maximum)
                best_j, best = j, (k1, k2)
    if best is None:
        return None
    return tuple(lo + -((-(k + 1) * width) // BINS) for k in best)  # lo + ceil((k + 1) W / 256)


def otsu_loop(h, classes=2, middle="foreground", correction=1.0, bounds=(0, 65535)) -> Otsu:
    h = [int(c) for c in h]
    occupied = [v for v, c in enumerate(h) if c]
    lo, hi = occupied[0], occupied[-1]
    t1 = t2 = _two_loop(h, lo, hi)
    if classes == 3:
        pair = _three_loop(h, lo, hi)
        if pair is not None:
            t1, t2 = pair
    raw = t1 if (classes == 2 or middle == "foreground") else t2
    return Otsu(finish(raw, correction, bounds), lo, hi, t1, t2)


# ------------------------------------------------------------------------------------------------ the vectorised form
def _quotient(s, n):
    s, n = s.astype(np.float64), n.astype(np.float64)  # (exact: both below 2^53)
    return s * s / n


def _two_numpy(h, lo, hi) -> int:
    if lo == hi:
        return lo
    v = np.arange(LEVELS, dtype=np.int64)
    cum_n, cum_s = np.cumsum(h), np.cumsum(h * v)
    t = np.arange(lo + 1, hi + 1)
    n0, s0 = cum_n[t - 1], cum_s[t - 1]
    j = _quotient(s0, n0) + _quotient(cum_s[-1] - s0, cum_n[-1] - n0)
    return int(t[np.argmax(j)])  # (argmax: the first index of the maximum)


def _three_numpy(h, lo, hi):
    width = hi - lo + 1
    v = np.arange(lo, hi + 1, dtype=np.int64)
    b = ((v - lo) * BINS) // width
    bin_n = np.zeros(BINS, np.int64)
    np.add.at(bin_n, b, h[lo:hi + 1])
    bin_s = np.zeros(BINS, np.int64)
    np.add.at(bin_s, b, h[lo:hi + 1] * v)
    cum_n, cum_s = np.cumsum(bin_n), np.cumsum(bin_s)
    k1, k2 = np.meshgrid(np.arange(BINS - 1), np.arange(BINS - 1), indexing="ij")
    n0, s0 = cum_n[k1], cum_s[k1]
    n1, s1 = cum_n[k2] - n0, cum_s[k2] - s0
    n2, s2 = cum_n[-1] - cum_n[k2], cum_s[-1] - cum_s[k2]
    valid = (k1 < k2) & (n0 > 0) & (n1 > 0) & (n2 > 0)
    if not valid.any():
        return None
    one = np.int64(1)
    j = _quotient(s0, np.where(valid, n0, one)) + _quotient(s1, np.where(valid, n1, one)) + _quotient(s2, np.where(valid, n2, one))
    j = np.where(valid, j, -1.0)
    a, c = np.unravel_index(np.argmax(j), j.shape)  # (row-major argmax: the smallest k1, then the smallest k2)
    return tuple(int(lo + ((k + 1) * width + BINS - 1) // BINS) for k in (a, c))


def otsu_numpy(h, classes=2, middle="foreground", correction=1.0, bounds=(0, 65535)) -> Otsu:
    h = np.asarray(h, dtype=np.int64)
    occupied = np.flatnonzero(h)
    lo, hi = int(occupied[0]), int(occupied[-1])
    t1 = t2 = _two_numpy(h, lo, hi)
    if classes == 3:
        pair = _three_numpy(h, lo, hi)
        if pair is not None:
            t1, t2 = pair
    raw = t1 if (classes == 2 or middle == "foreground") else t2
    return Otsu(finish(raw, correction, bounds), lo, hi, t1, t2)


def otsu(tile, classes=2, middle="foreground", correction=1.0, bounds=(0, 65535)) -> Otsu:
    """The threshold of one uint16 tile (the vectorised statement)."""
    return otsu_numpy(histogram(tile), classes, middle, correction, bounds)


def otsu_batch(image, **options):
    """image uint16 [F,Y,X] -> (thresholds int32 [F], details int32 [F,4])."""
    rows = [otsu(tile, **options) for tile in np.asarray(image)]
    return (np.array([r.threshold for r in rows], np.int32).reshape(-1),
            np.array([r.details for r in rows], np.int32).reshape(-1, 4))
