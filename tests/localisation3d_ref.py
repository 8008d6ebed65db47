"""
nuc_conv_3d of the reference (src/extraction/core/functions/custom/localisation.py:123-140, filter gauss3D 31-44), restated in
float64 from its definition, and the seeded inputs it is pinned and the kernel is tested on.

The restatement has a structure of its own: two explicit 1-D filters (in plane and along z), three direct 1-D correlations in the
order x, y, z (the kernel goes z, x, y) and the closed-form normaliser sum(h^2) = (sum gx^2)^2 sum gz^2 / ((sum gx)^2 sum gz)^2,
where the reference builds the (2 hw + 1)^3 filter, zeroes its entries below eps * max and lets scipy.signal.convolve pick a
method.  tests/test_cpu_localisation3d_ref.py pins it to the values the reference's own function returned
(tests/golden/reference_nuc_conv_3d.json).

  v     = the stack's voxels under the 2-D mask repeated on every plane
  N     = number of NON-ZERO values in v                 med = np.median(v)
  chi   = chi2.ppf(0.95, 2)                               r   = sqrt(0.085 N / pi)
  sd    = r / sqrt(chi)                                   hw  = ceil(2 r)             ratio = z_spacing / pixel_size
  gx[k] = exp(-k^2 / (2 sd)), gz[k] = exp(-k^2 / (2 sd ratio)), k = -hw .. hw   (sd, not sd^2: the reference's gauss3D)
  J     = stack - med under the mask, 0 elsewhere (uint16 -> float64, float32 stays float32: NumPy's arithmetic)
  value = max over the stack of correlate(J, gx gx gz / ((sum gx)^2 sum gz), "same") / (sum(h^2) 0.95 pi chi sd^2)
"""
import functools

import numpy as np
from scipy import signal, stats

ALPHA = 0.95
VOLUME = 0.085


def parts(cell_mask, trap_image, pixel_size=0.23, z_spacing=0.6):
    """-> (J float64 [Z,Y,X], gx, gz: the 1-D filters normalised to sum 1, denominator, hw) or None where the value is NaN"""
    mask = np.asarray(cell_mask, bool)
    image = np.asarray(trap_image)
    if image.ndim != 3 or mask.shape != image.shape[1:]:
        raise ValueError((mask.shape, image.shape))
    inside = image[:, mask]  # [Z, area]
    if inside.size == 0:
        return None  # the median of nothing
    n_nonzero = int(np.count_nonzero(inside))
    if n_nonzero == 0:
        return None  # sd = 0: the filter is exp(-0 / 0)
    med = np.median(inside)  # float64 for uint16 voxels, float32 for float32 voxels
    chi = stats.chi2.ppf(ALPHA, df=2)
    radius = np.sqrt(VOLUME * n_nonzero / np.pi)
    sd = float(radius / np.sqrt(chi))
    hw = int(np.ceil(2 * radius))
    k = np.arange(-hw, hw + 1, dtype=np.float64)
    gx = np.exp(-(k * k) / (2.0 * sd))
    gz = np.exp(-(k * k) / (2.0 * sd * (z_spacing / pixel_size)))
    sum_h2 = np.sum(gx * gx) ** 2 * np.sum(gz * gz) / (np.sum(gx) ** 2 * np.sum(gz)) ** 2
    if image.dtype == np.float32:
        diff = (image - np.float32(med)).astype(np.float64)  # rounded to float32, as NumPy subtracts two float32
    else:
        diff = image.astype(np.float64) - float(med)
    return np.where(mask[None], diff, 0.0), gx / np.sum(gx), gz / np.sum(gz), sum_h2 * ALPHA * np.pi * chi * sd**2, hw


def nuc_conv_3d(cell_mask, trap_image, pixel_size=0.23, z_spacing=0.6):
    p = parts(cell_mask, trap_image, pixel_size, z_spacing)
    if p is None:
        return float("nan")
    J, gx, gz, denominator, hw = p
    along_x = signal.correlate(J, gx[None, None, :], mode="same", method="direct")
    along_y = signal.correlate(along_x, gx[None, :, None], mode="same", method="direct")
    # along z the filter may be longer than the stack: pad the stack to the filter's reach, so that "valid" returns exactly the
    # stack's planes whichever of the two is longer
    padded = np.pad(along_y, ((hw, hw), (0, 0), (0, 0)))
    resp = signal.correlate(padded, gz[:, None, None], mode="valid", method="direct")
    assert resp.shape == J.shape
    return float(np.max(resp) / denominator)


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _ellipse(shape, cy, cx, ry, rx):
    yy, xx = np.mgrid[0 : shape[0], 0 : shape[1]]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def _noise(seed, shape, lo=300, hi=900):
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.int64)


def _spot(shape, cz, cy, cx, s, amp):
    """a 3-D Gaussian spot in a [Z,Y,X] stack, twice as narrow along z"""
    zz, yy, xx = np.mgrid[0 : shape[0], 0 : shape[1], 0 : shape[2]]
    return amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2 + 4.0 * (zz - cz) ** 2) / (2.0 * s * s))


def _scene(lab, img, **kwargs):
    """one tile, one channel"""
    assert img.min() >= 0 and img.max() <= 65535
    return dict(labels=lab[None].astype(np.uint16), stack=img.astype(np.uint16)[None, None], channel=0, kwargs=kwargs)


def tiny_labels():
    lab = np.zeros((24, 24), np.uint16)
    lab[5, 5] = 1
    lab[10, 8:11] = 2
    lab[15:17, 15:17] = 3
    return lab


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(labels uint16 [F,Y,X], stack [F,C,Z,Y,X] uint16 or float32, channel, kwargs).  Rows are (tile, label) for every
    label 1..max of every tile, the order of the object table.  Treat as read-only."""
    from aliby_amd import synth

    out = {}
    # 1. mixed batch: two synthetic tiles of 96 x 96 with three planes, the `cells` labels, channel 1 of 2
    fovs = [synth.make_fov(2, k, shape=(96, 96), n_channels=2, n_z=3, n_target=8) for k in (0, 1)]
    lab = np.stack([f["cells"] for f in fovs]).astype(np.uint16)
    px = np.stack([f["pixels"] for f in fovs]).astype(np.uint16)  # [F,C,Z,Y,X]
    assert px.shape == (2, 2, 3, 96, 96)
    out["mixed_u16"] = dict(labels=lab, stack=px, channel=1, kwargs={})
    out["mixed_f32"] = dict(labels=lab, stack=(px.astype(np.float32) / np.float32(65535.0)).astype(np.float32), channel=1, kwargs={})
    # 8. pixel_size / z_spacing, on the same input
    out["kw_flat"] = dict(labels=lab, stack=px, channel=1, kwargs=dict(pixel_size=0.1, z_spacing=1.0))
    out["kw_cubic"] = dict(labels=lab, stack=px, channel=1, kwargs=dict(pixel_size=0.5, z_spacing=0.5))
    # 2. corner objects: the "same" crop on Y and X; bright spots against the corners, on the first and the last plane
    shape = (5, 48, 56)
    lab = np.zeros(shape[1:], np.uint16)
    lab[_ellipse(shape[1:], 2, 3, 9.0, 7.0)] = 1
    lab[_ellipse(shape[1:], 47, 55, 8.0, 11.0)] = 2
    out["corner"] = _scene(lab, _noise(31, shape) + _spot(shape, 0, 1, 1, 2.0, 6000) + _spot(shape, 4, 46, 54, 2.5, 9000))
    # 3. tiny objects (1, 3 and 4 pixels), on one plane and on nine
    out["tiny_z1"] = _scene(tiny_labels(), _noise(32, (1, 24, 24)))
    out["tiny_z9"] = _scene(tiny_labels(), _noise(33, (9, 24, 24)))
    # 4. an object that nearly fills its tile: the dilated box is the whole stack, no outside 0 takes part.  Its brightest voxels
    # sit at the border, so that the response of a centred blob does not hide the question
    shape = (2, 12, 12)
    lab = np.zeros(shape[1:], np.uint16)
    lab[0:12, 0:11] = 1
    lab[0, 0] = 0
    out["fill"] = _scene(lab, _noise(34, shape) + _spot(shape, 0, 11, 10, 1.5, 4000))
    # 5. zeros inside the cell: alternate columns on alternate planes, so N is neither area * Z nor a multiple of the area
    shape = (5, 40, 40)
    lab = _ellipse(shape[1:], 20, 19, 11.0, 13.0).astype(np.uint16)
    img = _noise(35, shape) + _spot(shape, 3, 17, 22, 2.5, 5000)
    img[1::2, :, 1::2] = np.where(lab[None, :, 1::2] > 0, 0, img[1::2, :, 1::2])
    img[0, 20, 19] = 0
    area, n = int(lab.sum()), int(np.count_nonzero(img[:, lab > 0]))
    assert n < area * 5 and n % area != 0
    out["zeros_inside"] = _scene(lab, img)
    # 6. undefined and degenerate: 1 = all-zero voxels, 2 = absent, 3 = uniform, 4 = an ordinary blob
    shape = (3, 40, 48)
    lab = np.zeros(shape[1:], np.uint16)
    lab[_ellipse(shape[1:], 9, 10, 6.0, 7.0)] = 1
    lab[_ellipse(shape[1:], 28, 12, 7.0, 6.0)] = 3
    lab[_ellipse(shape[1:], 20, 34, 9.0, 8.0)] = 4
    img = _noise(36, shape) + _spot(shape, 1, 22, 33, 2.0, 4000)
    img[:, lab == 1] = 0
    img[:, lab == 3] = 1234
    out["degenerate"] = _scene(lab, img)
    # 7. neighbours: two touching objects, the second 50 000 counts brighter; the same with the second's voxels zeroed; and the
    # first object alone
    shape = (3, 40, 44)
    lab = np.zeros(shape[1:], np.uint16)
    both = _ellipse(shape[1:], 20, 22, 12.0, 15.0)
    lab[both] = 1
    lab[both & (np.mgrid[0:40, 0:44][1] >= 22)] = 2
    img = _noise(37, shape) + _spot(shape, 1, 18, 18, 2.0, 3000)
    out["neighbours"] = _scene(lab, img + 50000 * (lab == 2)[None])
    out["neighbours_zeroed"] = _scene(lab, np.where((lab == 2)[None], 0, img))
    out["neighbours_alone"] = _scene(np.where(lab == 1, 1, 0), img)
    # 9. one large object: a disc of radius 40 in a 120 x 120 tile, five planes (hw = 56)
    shape = (5, 120, 120)
    lab = _ellipse(shape[1:], 60, 60, 40.0, 40.0).astype(np.uint16)
    out["disc40"] = _scene(lab, _noise(38, shape) + _spot(shape, 2, 50, 72, 12.0, 7000))
    # 10. float32 in plain LDS: the corner scene (odd voxel counts) and the filled tile (262 voxels: the mean of two middle values)
    for name in ("corner", "fill"):
        src = out[name]
        out[name + "_f32"] = dict(labels=src["labels"], stack=(src["stack"].astype(np.float32) / np.float32(65535.0)).astype(np.float32),
                                  channel=0, kwargs={})
    for s in out.values():
        s["labels"].setflags(write=False)
        s["stack"].setflags(write=False)
    return out


def rows(scene):
    """[(tile, label)] of a scene, in table order"""
    return [(f, l) for f in range(scene["labels"].shape[0]) for l in range(1, int(scene["labels"][f].max()) + 1)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement on every row of a scene -> float64 [n_rows]; computed once"""
    s = scenes()[name]
    res = np.array([nuc_conv_3d(s["labels"][f] == l, s["stack"][f, s["channel"]], **s["kwargs"]) for f, l in rows(s)], np.float64)
    res.setflags(write=False)
    return res
