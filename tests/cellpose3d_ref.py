"""
Float32 restatement of cellpose's 3-D dynamics (compute_masks on a [3,Z,Y,X] flow field, do_3D=True), the yardstick of
aliby_amd/csrc/dynamics.hip.  Every float32 operation is written out in the order the kernels use, so labels compare bit for
bit; where cellpose leaves an order to an unstable sort (overlapping seeds) the restatement fixes it as the 2-D one does
(oracle/cellpose_restated.py): seed priority = (points in the bin, raster position), a later seed overwrites an earlier one.

  follow    cellpose's steps_interp with grid_sample in 3-D (trilinear, align_corners=False, zero padding): positions
            p_d = idx_d / (L_d-1) * 2 - 1, field im_d = dP_d * fg / 5 * 2/(L_d-1), per step i_d = ((p_d+1)*L_d - 1)/2, taps in
            PyTorch's order tnw, tne, tsw, tse, bnw, bne, bsw, bse with weights (wx*wy)*wz summed from 0, p = clamp(p + delta, -1, 1);
            end points (p+1)*0.5*(L_d-1);
  seeds     histogram of the end cells trunc(clamp(end + 20, 0, L + 19)) on the volume padded by 20, bins equal to the maximum
            of their 5x5x5 neighbourhood (constant -1 outside) with more than 10 points;
  growth    per seed, in priority order: 5 x (3x3x3 dilation AND window > 2) inside an 11x11x11 window, rank + 1 written;
  labels    voxel = owner of its end cell; labels with more than max_size_fraction * Z*Y*X voxels removed; renumbered by first
            appearance in (z,y,x) raster order;
  fill      masks below min_size voxels dropped, each remaining mask's 6-connected 3-D holes filled inside its bounding box,
            kept masks numbered 1..n in label order, a voxel inside the holes of several masks going to the highest label.
No flow-error QC: cellpose documents flow_threshold as "not used for 3D".
"""

from __future__ import annotations

import numpy as np
from scipy import ndimage as ndi

f32 = np.float32

# PyTorch grid_sample's tap order: (dz, dy, dx) offsets of tnw, tne, tsw, tse, bnw, bne, bsw, bse
TAPS = ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))


def follow_flows_3d(dPs, inds, niter=200):
    """dPs float32 [3,Z,Y,X] = dP * fg / 5; inds = (zs, ys, xs) of the foreground voxels -> end points float32 [3, n] (z, y, x)."""
    L = dPs.shape[1:]
    s = [f32(n - 1) for n in L]
    im = [dPs[d] * (f32(2.0) / s[d]) for d in range(3)]
    p = [inds[d].astype(f32) / s[d] * f32(2.0) - f32(1.0) for d in range(3)]
    Lf = [f32(n) for n in L]

    def tap(field, zz, yy, xx):
        ok = (zz >= 0) & (zz < L[0]) & (yy >= 0) & (yy < L[1]) & (xx >= 0) & (xx < L[2])
        v = np.zeros(len(zz), f32)
        v[ok] = field[zz[ok], yy[ok], xx[ok]]
        return v

    for _ in range(niter):
        i = [((p[d] + f32(1.0)) * Lf[d] - f32(1.0)) / f32(2.0) for d in range(3)]
        lo = [np.floor(i[d]) for d in range(3)]
        hi = [lo[d] + f32(1.0) for d in range(3)]
        wlo = [hi[d] - i[d] for d in range(3)]  # weight of the low tap along axis d
        whi = [i[d] - lo[d] for d in range(3)]
        li = [lo[d].astype(np.int64) for d in range(3)]
        delta = []
        for d in range(3):
            acc = None
            for dz, dy, dx in TAPS:
                wx = whi[2] if dx else wlo[2]
                wy = whi[1] if dy else wlo[1]
                wz = whi[0] if dz else wlo[0]
                term = tap(im[d], li[0] + dz, li[1] + dy, li[2] + dx) * ((wx * wy) * wz)
                acc = (f32(0.0) + term) if acc is None else acc + term
            delta.append(acc)
        p = [np.minimum(np.maximum(p[d] + delta[d], f32(-1.0)), f32(1.0)) for d in range(3)]
    return np.stack([(p[d] + f32(1.0)) * f32(0.5) * s[d] for d in range(3)]).astype(f32)


def seed_mask(h1):
    """Bins equal to the maximum of their 5x5x5 neighbourhood (constant -1 outside) with more than 10 points."""
    hmax = ndi.maximum_filter(h1, size=5, mode="constant", cval=-1)
    return (h1 >= hmax) & (h1 > 10)


def get_masks_3d(p_final, inds, shape0, rpad=20, max_size_fraction=0.4):
    """End points [3, n] -> labels uint32 [Z,Y,X] before hole filling, renumbered by first raster appearance."""
    shape = tuple(n + 2 * rpad for n in shape0)
    pt = []
    for d in range(3):
        q = np.clip(p_final[d] + f32(rpad), 0, None)
        pt.append(np.minimum(q, f32(shape0[d] + rpad - 1)).astype(np.int64))  # torch's cast to long: truncation
    pt = tuple(pt)
    h1 = np.zeros(shape, np.int64)
    np.add.at(h1, pt, 1)
    seeds = np.nonzero(seed_mask(h1))
    M0 = np.zeros(shape0, np.uint32)
    if len(seeds[0]) == 0:
        return M0
    flat = np.ravel_multi_index(seeds, shape)
    prio = h1[seeds].astype(np.int64) * int(np.prod(shape)) + flat  # ascending: later (larger) overwrite earlier
    order = np.argsort(prio, kind="stable")
    M1 = np.zeros(shape, np.int64)
    cube = np.ones((3, 3, 3), bool)
    for rank, k in enumerate(order):
        c = [int(seeds[d][k]) for d in range(3)]
        sl = tuple(slice(c[d] - 5, c[d] + 6) for d in range(3))
        win = h1[sl]
        sm = np.zeros((11, 11, 11), bool)
        sm[5, 5, 5] = True
        for _ in range(5):
            sm = ndi.binary_dilation(sm, cube) & (win > 2)
        M1[sl][sm] = rank + 1
    M0[inds] = M1[pt]
    uniq, counts = np.unique(M0, return_counts=True)
    # (the C entry takes max_size_fraction as a float32)
    big = float(np.prod(shape0)) * float(f32(max_size_fraction))
    drop = uniq[(counts > big) & (uniq != 0)]
    if len(drop):
        M0[np.isin(M0, drop)] = 0
    return renumber_first_appearance(M0)


def renumber_first_appearance(M):
    """1..n in the order labels are first met in a raster scan; 0 stays 0."""
    flat = M.ravel()
    uniq, first = np.unique(flat, return_index=True)
    keep = uniq != 0
    uniq, first = uniq[keep], first[keep]
    fwd = np.zeros(int(flat.max()) + 1 if flat.size else 1, np.uint32)
    fwd[uniq[np.argsort(first, kind="stable")]] = np.arange(1, len(uniq) + 1, dtype=np.uint32)
    return fwd[M]


def fill_holes_3d(mask):
    """Holes of a boolean box: background voxels not 6-connected to the box's outside (the box is ringed by one voxel of
    outside) -> the filled mask.  Written as a flood of the background, independently of scipy's binary_fill_holes."""
    ring = np.pad(~mask, 1, constant_values=True)
    comp, _ = ndi.label(ring, structure=ndi.generate_binary_structure(3, 1))
    outside = np.unique(np.concatenate([comp[0].ravel(), comp[-1].ravel(), comp[:, 0].ravel(), comp[:, -1].ravel(),
                                        comp[:, :, 0].ravel(), comp[:, :, -1].ravel()]))
    reach = np.isin(comp, outside[outside != 0])
    return ~reach[1:-1, 1:-1, 1:-1]


def fill_holes_and_remove_small_masks_3d(masks, min_size=15):
    out = np.zeros(masks.shape, np.uint16)
    j = 0
    for i, slc in enumerate(ndi.find_objects(masks.astype(np.int64))):
        if slc is None:
            continue
        msk = masks[slc] == (i + 1)
        if min_size > 0 and msk.sum() < min_size:
            continue
        j += 1
        out[slc][fill_holes_3d(msk)] = j  # (label order: a later, higher label overwrites)
    return out


def compute_masks_3d(dP, cellprob, niter=200, cellprob_threshold=0.0, min_size=15, max_size_fraction=0.4):
    """dP float32 [3,Z,Y,X] (network scale), cellprob float32 [Z,Y,X] -> (labels uint16 [Z,Y,X], n, end points float32
    [3,Z,Y,X], zero off the foreground)."""
    fg = cellprob > f32(cellprob_threshold)
    shape0 = cellprob.shape
    pf = np.zeros((3, *shape0), f32)
    if not fg.any():
        return np.zeros(shape0, np.uint16), 0, pf
    inds = np.nonzero(fg)
    dPs = np.where(fg[None], dP, f32(0.0)).astype(f32) / f32(5.0)
    p_final = follow_flows_3d(dPs, inds, niter=niter)
    pf[(slice(None), *inds)] = p_final
    masks = get_masks_3d(p_final, inds, shape0, max_size_fraction=max_size_fraction)
    masks = fill_holes_and_remove_small_masks_3d(masks, min_size=min_size)
    return masks, int(masks.max()), pf
