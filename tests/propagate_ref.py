"""Restatement of the `propagate` definition (include/aliby_hip.h, csrc/feat_propagate.hip): CellProfiler's IdentifySecondaryObjects,
method "Propagation", on an exact integer metric.

  passable(p)   primary[p] != 0, or image[p] >= threshold and (distance is None or secondary_labels(primary, distance)[p] != 0)
  P(p,q)        sum over o in {-1,0,1}^2 of |image[clamp(p+o)] - image[clamp(q+o)]|, each coordinate clamped to the tile
  W(p,q)        isqrt(256 (P^2 + m L)), m = |dy| + |dx|, for passable 8-neighbours p, q
  D[p]          min over paths from labelled pixels of the sum of W; out[p] the smallest label that arrives at D[p]
  labelled p    out = primary, D = 0: a source only
  no path       out = 0, D = 2^64 - 1

`propagate_tile` is the definition itself: a heap Dijkstra in Python integers on the lexicographic key (D, label), math.isqrt for the
root.  `propagate_labels` is a vectorised NumPy Jacobi iteration on packed uint64 keys (D << 16) | label with its own root (float
sqrt and a correction), for the larger cases; tests/test_cpu_propagate_ref.py holds the two against each other bit for bit.
"""

from __future__ import annotations

import heapq
import math

import numpy as np

from tests import secondary_ref

NONE = (1 << 64) - 1
NOEDGE = (1 << 32) - 1
_STEPS = ((0, 1), (1, -1), (1, 0), (1, 1))  # E, SW, S, SE: the other four are these seen from the far end


def lambda2(regularization=0.05, image_max=65535):
    """L = llrint((regularization * image_max)^2) in float64, half to even."""
    scaled = float(regularization) * float(image_max)
    return int(round(scaled * scaled))


def passable(primary, image, threshold=0, distance=None):
    primary, image = np.asarray(primary), np.asarray(image)
    ok = image.astype(np.int64) >= int(threshold)
    if distance is not None:
        ok &= secondary_ref.secondary_tile(primary, int(distance))[0] != 0
    return ok | (primary != 0)


def _clamped(image, y, x):
    Y, X = image.shape
    return int(image[min(max(y, 0), Y - 1), min(max(x, 0), X - 1)])


def pair_difference(image, p, q):
    """P(p, q) by the definition, in Python integers."""
    return sum(abs(_clamped(image, p[0] + oy, p[1] + ox) - _clamped(image, q[0] + oy, q[1] + ox)) for oy in (-1, 0, 1) for ox in (-1, 0, 1))


def weight(image, p, q, lam2):
    m = abs(p[0] - q[0]) + abs(p[1] - q[1])
    assert m in (1, 2) and max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1
    P = pair_difference(image, p, q)
    return math.isqrt(256 * (P * P + m * lam2))


def propagate_tile(primary, image, threshold=0, regularization=0.05, distance=None, image_max=65535):
    """One tile [Y,X] -> (out uint16 [Y,X], D uint64 [Y,X]) by Dijkstra on the key (D, label)."""
    primary, image = np.asarray(primary), np.asarray(image)
    assert primary.ndim == 2 and primary.shape == image.shape
    Y, X = primary.shape
    lam2 = lambda2(regularization, image_max)
    ok = passable(primary, image, threshold, distance)
    best = {}
    heap = []
    for y, x in zip(*np.nonzero(primary)):
        best[(int(y), int(x))] = (0, int(primary[y, x]))
        heap.append((0, int(primary[y, x]), int(y), int(x)))
    heapq.heapify(heap)
    while heap:
        d, lab, y, x = heapq.heappop(heap)
        if best[(y, x)] != (d, lab):
            continue
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                qy, qx = y + dy, x + dx
                if (dy or dx) and 0 <= qy < Y and 0 <= qx < X and ok[qy, qx] and primary[qy, qx] == 0:  # (labelled: a source only)
                    cand = (d + weight(image, (y, x), (qy, qx), lam2), lab)
                    if cand < best.get((qy, qx), (NONE, 0)):
                        best[(qy, qx)] = cand
                        heapq.heappush(heap, (*cand, qy, qx))
    out = np.zeros((Y, X), np.uint16)
    D = np.full((Y, X), NONE, np.uint64)
    for (y, x), (d, lab) in best.items():
        out[y, x], D[y, x] = lab, d
    return out, D


def _isqrt(v):
    """floor(sqrt(v)) of an int64 array below 2^52: the float root, one step down, one step up."""
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    return r


def edge_weights(image, ok, lam2):
    """uint64 [4,Y,X]: the weight of the edge from (y, x) to its E, SW, S, SE neighbour, NOEDGE where there is none."""
    image = np.asarray(image).astype(np.int64)
    Y, X = image.shape
    ys, xs = np.arange(Y), np.arange(X)

    def fetch(dy, dx):
        return image[np.clip(ys + dy, 0, Y - 1)][:, np.clip(xs + dx, 0, X - 1)]

    w = np.full((4, Y, X), NOEDGE, np.uint64)
    for k, (dy, dx) in enumerate(_STEPS):
        P = np.zeros((Y, X), np.int64)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                P += np.abs(fetch(oy, ox) - fetch(oy + dy, ox + dx))
        cost = _isqrt(256 * (P * P + (abs(dy) + abs(dx)) * lam2))
        far = np.zeros((Y, X), bool)  # the far end is in the tile and passable
        y1, x0, x1 = Y - dy, max(0, -dx), X - max(0, dx)
        far[:y1, x0:x1] = ok[dy:, x0 + dx:x1 + dx]
        w[k] = np.where(ok & far, cost, NOEDGE).astype(np.uint64)
    return w


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside."""
    Y, X = a.shape
    b = np.full_like(a, fill)
    b[max(0, -dy):Y - max(0, dy), max(0, -dx):X - max(0, dx)] = a[max(0, dy):Y + min(0, dy), max(0, dx):X + min(0, dx)]
    return b


def propagate_jacobi(primary, image, threshold=0, regularization=0.05, distance=None, image_max=65535):
    """One tile [Y,X] -> (out uint16, D uint64, sweeps): Jacobi sweeps of the packed keys to the fixed point."""
    primary, image = np.asarray(primary), np.asarray(image)
    assert primary.ndim == 2 and primary.shape == image.shape and primary.size <= 1 << 23
    w = edge_weights(image, passable(primary, image, threshold, distance), lambda2(regularization, image_max))
    none, noedge = np.uint64(NONE), np.uint64(NOEDGE)
    keys = np.where(primary != 0, primary.astype(np.uint64), none)
    # the eight ways into a pixel: from (y + dy, x + dx) over its own edge, from (y - dy, x - dx) over that pixel's edge
    ways = []
    for k, (dy, dx) in enumerate(_STEPS):
        for sy, sx, wk in ((dy, dx, w[k]), (-dy, -dx, _shift(w[k], -dy, -dx, noedge))):
            ways.append((sy, sx, wk != noedge, np.where(wk != noedge, wk, 0).astype(np.uint64) << np.uint64(16)))
    sweeps = 0
    while True:
        new = keys
        for sy, sx, edge, cost in ways:
            nk = _shift(keys, sy, sx, none)
            valid = edge & (nk != none)
            new = np.minimum(new, np.where(valid, np.where(valid, nk, 0) + cost, none))
        new = np.where(primary != 0, keys, new)  # a labelled pixel is a source only
        if (new == keys).all():
            break
        keys = new
        sweeps += 1
    out = np.where(keys == none, 0, keys & np.uint64(0xFFFF)).astype(np.uint16)
    D = np.where(keys == none, none, keys >> np.uint64(16))
    return out, D, sweeps


def propagate_labels(primary, image, threshold=0, regularization=0.05, distance=None, image_max=65535):
    """[F,Y,X] -> (uint16 [F,Y,X], uint64 [F,Y,X]), every tile on its own."""
    primary, image = np.asarray(primary), np.asarray(image)
    assert primary.ndim == 3 and primary.shape == image.shape
    out = np.zeros(primary.shape, np.uint16)
    D = np.full(primary.shape, NONE, np.uint64)
    for f in range(primary.shape[0]):
        out[f], D[f], _ = propagate_jacobi(primary[f], image[f], threshold, regularization, distance, image_max)
    return out, D
