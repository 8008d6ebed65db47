"""
TEST INFRASTRUCTURE — plain NumPy references for csrc/stager.hip (crop + median pad, reduce_z) and csrc/objects.hip (the object
table), written from the definitions and not from the kernels.  Held against independent code (np.pad, ufunc.reduce,
scipy.ndimage.find_objects) in tests/test_cpu_stager_ref.py; the GPU suites compare the kernels with these bit for bit.
"""

from __future__ import annotations

import numpy as np

OBJECT_ROW = np.dtype([("tile", "<i4"), ("label", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("area", "<i4")])


def round_half_even_mean(a, b):
    """The median of an even count as np.pad(mode="median") leaves it in an integer array: the float64 mean of the two middle
    values, rounded half to even."""
    return np.rint((np.asarray(a, np.float64) + np.asarray(b, np.float64)) / 2.0)


def _line_median(block, axis):
    """One median per line of `block` along `axis` (kept as a length-1 axis), rounded as above, in the block's dtype."""
    s = np.sort(block, axis=axis)
    n = s.shape[axis]
    mid = np.take(s, [n // 2], axis=axis)
    if n % 2:
        return mid
    return round_half_even_mean(np.take(s, [n // 2 - 1], axis=axis), mid).astype(block.dtype)


def nan_rule(Y, X, rect):
    """(is a NaN tile, (pad before y, after y, before x, after x)).  if_out_of_bounds_pad compares `padding / 0.25` — rows (y, x),
    columns (before, after) — with tile_shape = (h, w) broadcast over the LAST axis: before-pads meet h, after-pads meet w."""
    y0, x0, h, w = (int(v) for v in rect)
    pyb, pya = max(0, -y0), max(0, y0 + h - Y)
    pxb, pxa = max(0, -x0), max(0, x0 + w - X)
    nan = pyb * 4 > h or pya * 4 > w or pxb * 4 > h or pxa * 4 > w
    return nan, (pyb, pya, pxb, pxa)


def crop_pad(stack_czyx, rect):
    """The window rect = (y0, x0, h, w) of stack [..., Y, X] as if_out_of_bounds_pad gives it for every leading index: the
    overlap copied, then one median per column over the inside rows, then one median per row over the inside columns of ALL
    rows, the ones the first pass made included.  None for a NaN tile; ValueError for a window without overlap that the NaN
    rule lets through (where np.pad refuses an empty axis; a window that ends left of or above pixel 0 gives the restated
    reference a negative slice stop, which Python counts from the far edge: here it is judged by the same rule)."""
    stack = np.asarray(stack_czyx)
    Y, X = stack.shape[-2:]
    y0, x0, h, w = (int(v) for v in rect)
    nan, (pyb, pya, pxb, pxa) = nan_rule(Y, X, rect)
    if nan:
        return None
    ny, nx = h - pyb - pya, w - pxb - pxa  # inside rows / columns
    if ny <= 0 or nx <= 0:
        raise ValueError(f"window {(y0, x0, h, w)} does not overlap the {Y} x {X} frame and is not a NaN tile")
    out = np.zeros(stack.shape[:-2] + (h, w), stack.dtype)
    out[..., pyb:pyb + ny, pxb:pxb + nx] = stack[..., y0 + pyb:y0 + pyb + ny, x0 + pxb:x0 + pxb + nx]
    if pyb or pya:
        m = _line_median(out[..., pyb:pyb + ny, pxb:pxb + nx], axis=-2)  # [..., 1, nx]
        out[..., :pyb, pxb:pxb + nx] = m
        out[..., pyb + ny:, pxb:pxb + nx] = m
    if pxb or pxa:
        m = _line_median(out[..., :, pxb:pxb + nx], axis=-1)  # [..., h, 1]: every row
        out[..., :, :pxb] = m
        out[..., :, pxb + nx:] = m
    return out


def reduce_fold(a, op, axis):
    """ufunc.reduce(a, axis) for op in ("max", "add", "div") as an explicit left fold, plane by plane, in NumPy's result dtype:
    u16 max -> u16, u16 add -> u64, u16 divide -> f64, f32 anything -> f32.  (np.add.reduce over a contiguous last axis sums
    pairwise, which is not the fold the kernel and the header promise.)  f32 max is np.maximum: a NaN comes through."""
    a = np.moveaxis(np.asarray(a), axis, 0)
    if a.dtype == np.uint16:
        acc_dtype = {"max": np.uint16, "add": np.uint64, "div": np.float64}[op]
    elif a.dtype == np.float32:
        acc_dtype = np.float32
    else:
        raise TypeError(a.dtype)
    step = {"max": np.maximum, "add": np.add, "div": np.divide}[op]
    acc = a[0].astype(acc_dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for z in range(1, a.shape[0]):
            acc = step(acc, a[z].astype(acc_dtype))
            assert acc.dtype == acc_dtype
    return acc


def object_rows(labels_fyx, max_labels=None):
    """(rows, offsets): one row per frame f and label 1..max_labels[f] (default: the frame's largest label) with the bounding
    box (y1, x1 exclusive) and the pixel count.  A label without pixels has area 0 and the box (-1, -1, -1, -1); pixels of
    labels above max_labels[f] are counted nowhere."""
    labels = np.asarray(labels_fyx)
    F = labels.shape[0]
    mx = [int(labels[f].max()) if labels[f].size else 0 for f in range(F)] if max_labels is None else [int(m) for m in max_labels]
    offsets = np.zeros(F + 1, np.int32)
    offsets[1:] = np.cumsum(mx)
    rows = np.zeros(int(offsets[-1]), OBJECT_ROW)
    for f in range(F):
        r = rows[offsets[f]:offsets[f + 1]]
        r["tile"] = f
        r["label"] = np.arange(1, mx[f] + 1)
        for k in ("y0", "x0", "y1", "x1"):
            r[k] = -1
        if mx[f] == 0:
            continue
        area = np.bincount(labels[f].ravel(), minlength=mx[f] + 1)[1:mx[f] + 1]
        r["area"] = area
        yy, xx = np.nonzero((labels[f] > 0) & (labels[f] <= mx[f]))
        ll = labels[f][yy, xx].astype(np.int64) - 1
        for name, coord, fn, init in (("y0", yy, np.minimum, np.iinfo(np.int64).max), ("x0", xx, np.minimum, np.iinfo(np.int64).max),
                                      ("y1", yy + 1, np.maximum, -1), ("x1", xx + 1, np.maximum, -1)):
            acc = np.full(mx[f], init, np.int64)
            fn.at(acc, ll, coord)
            r[name] = np.where(area > 0, acc, -1)
    return rows, offsets
