"""Brute-force restatement of the `secondary` definition on volume labels (include/aliby_hip.h, csrc/feat_secondary3d.hip):
tests/secondary_ref.py with a z axis and an integer spacing.  No transform, no sweep: every background voxel against every labelled
voxel of its stack, integer squared distances on the lattice, the key d2 * 65536 + label, one minimum.

  vol[p] != 0                       out[p] = vol[p]
  else m = min over the labelled q of the stack of (sz dz)^2 + (sy dy)^2 + (sx dx)^2
    no such q, or m > N^2           out[p] = 0
    else                            out[p] = min{ vol[q] : d2(p, q) = m }
"""

from __future__ import annotations

import numpy as np

_PAIRS = 1 << 22  # pairs per chunk


def secondary_stack(vol, distance, spacing=(1, 1, 1)):
    """One [Z,Y,X] label stack -> (out uint16 [Z,Y,X], ties bool [Z,Y,X]): `ties` marks the grown voxels with more than one distinct
    label at the minimum distance m (where SciPy's index is a matter of its sweep order)."""
    vol = np.asarray(vol)
    assert vol.ndim == 3 and isinstance(distance, int) and distance >= 1
    sz, sy, sx = (int(s) for s in spacing)
    assert (sz, sy, sx) == tuple(spacing) and min(sz, sy, sx) >= 1
    out = vol.astype(np.uint16).copy()
    ties = np.zeros(vol.shape, dtype=bool)
    q = [c.astype(np.int64) for c in np.nonzero(vol)]
    p = [c.astype(np.int64) for c in np.nonzero(vol == 0)]
    if q[0].size == 0 or p[0].size == 0:
        return out, ties
    qlab = vol[tuple(q)].astype(np.int64)
    step = max(1, _PAIRS // q[0].size)
    for s in range(0, p[0].size, step):
        z, y, x = (c[s:s + step] for c in p)
        d2 = ((sz * (z[:, None] - q[0][None, :])) ** 2 + (sy * (y[:, None] - q[1][None, :])) ** 2
              + (sx * (x[:, None] - q[2][None, :])) ** 2)
        key = (d2 * 65536 + qlab[None, :]).min(axis=1)
        m, lab = key >> 16, key & 0xFFFF
        largest = np.where(d2 == m[:, None], qlab[None, :], 0).max(axis=1)
        grown = m <= distance * distance
        out[z[grown], y[grown], x[grown]] = lab[grown].astype(np.uint16)
        ties[z[grown], y[grown], x[grown]] = largest[grown] != lab[grown]
    return out, ties


def secondary_volume(volumes, distance, spacing=(1, 1, 1)):
    """[F,Z,Y,X] -> uint16 [F,Z,Y,X], every stack on its own."""
    volumes = np.asarray(volumes)
    assert volumes.ndim == 4
    out = np.zeros(volumes.shape, dtype=np.uint16)
    for f in range(volumes.shape[0]):
        out[f] = secondary_stack(volumes[f], distance, spacing)[0]
    return out
