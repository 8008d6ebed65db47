"""Brute-force restatement of the `secondary` definition (include/aliby_hip.h, csrc/feat_secondary.hip): CellProfiler's
IdentifySecondaryObjects, method "Distance - N".  No transform, no sweep: every background pixel against every labelled pixel of its
tile, integer squared distances, the key d2 * 65536 + label, one minimum.

  labels[p] != 0                    out[p] = labels[p]
  else m = min |p - q|^2 over the labelled q of the tile
    no such q, or m > N^2           out[p] = 0
    else                            out[p] = min{ labels[q] : |p - q|^2 = m }
"""

from __future__ import annotations

import numpy as np

_PAIRS = 1 << 22  # pairs per chunk


def secondary_tile(labels, distance):
    """One [Y,X] label image -> (out uint16 [Y,X], ties bool [Y,X]): `ties` marks the expanded pixels with more than one distinct label
    at the minimum distance m (where SciPy's index is a matter of its sweep order)."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and isinstance(distance, int) and distance >= 1
    out = labels.astype(np.uint16).copy()
    ties = np.zeros(labels.shape, dtype=bool)
    qy, qx = np.nonzero(labels)
    py, px = np.nonzero(labels == 0)
    if qy.size == 0 or py.size == 0:
        return out, ties
    qlab = labels[qy, qx].astype(np.int64)
    qy, qx = qy.astype(np.int64), qx.astype(np.int64)
    step = max(1, _PAIRS // qy.size)
    for s in range(0, py.size, step):
        y, x = py[s:s + step].astype(np.int64), px[s:s + step].astype(np.int64)
        d2 = (y[:, None] - qy[None, :]) ** 2 + (x[:, None] - qx[None, :]) ** 2
        key = (d2 * 65536 + qlab[None, :]).min(axis=1)
        m, lab = key >> 16, key & 0xFFFF
        at_m = d2 == m[:, None]
        largest = np.where(at_m, qlab[None, :], 0).max(axis=1)
        grown = m <= distance * distance
        out[y[grown], x[grown]] = lab[grown].astype(np.uint16)
        ties[y[grown], x[grown]] = largest[grown] != lab[grown]
    return out, ties


def secondary_labels(labels, distance):
    """[F,Y,X] -> uint16 [F,Y,X], every tile on its own."""
    labels = np.asarray(labels)
    assert labels.ndim == 3
    out = np.zeros(labels.shape, dtype=np.uint16)
    for f in range(labels.shape[0]):
        out[f] = secondary_tile(labels[f], distance)[0]
    return out
