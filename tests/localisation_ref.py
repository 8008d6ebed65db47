"""
nuc_est_conv of the reference (src/extraction/core/functions/custom/localisation.py:75-120), restated in float64 from its
definition, and the seeded inputs it is pinned and the kernel is tested on.

The restatement has a structure of its own: one explicit 1-D Gaussian g, two direct 1-D correlations (rows, then columns) and the
separable normaliser sum(h^2) = (sum g^2)^2 / (sum g)^4, where the reference builds the 2-D filter, zeroes its entries below
eps * max and lets scipy.signal.convolve pick a method.  tests/test_cpu_localisation_ref.py pins it to the values the
reference's own function returned (tests/golden/reference_nuc_est_conv.json).

  N     = number of NON-ZERO pixels of the cell          med = np.median(pixels of the cell)
  chi   = chi2.ppf(alpha, 2)                              r   = sqrt(object_radius_estimation N / pi)
  sigma = gaussian_sigma or r / sqrt(chi)                 hw  = ceil(2 r)
  J     = image - med inside the cell, 0 outside (uint16 -> float64, float32 stays float32: NumPy's arithmetic)
  value = max over the tile of correlate(J, g g^T / (sum g)^2, "same") / (sum(h^2) alpha pi chi sigma^2)
"""
import functools

import numpy as np
from scipy import signal, stats


def parts(cell_mask, trap_image, alpha=0.95, object_radius_estimation=0.085, gaussian_filter_shape=None, gaussian_sigma=None):
    """-> (J float64 [Y,X], g: the 1-D filter normalised to sum 1, denominator) or None where the value is NaN.
    gaussian_filter_shape is ignored, as the reference overwrites it."""
    alpha = 0.95 if alpha is None else alpha
    ore = 0.085 if object_radius_estimation is None else object_radius_estimation
    mask = np.asarray(cell_mask, bool)
    image = np.asarray(trap_image)
    inside = image[mask]
    if inside.size == 0:
        return None  # the median of nothing
    n_nonzero = int(np.count_nonzero(inside))
    med = np.median(inside)  # float64 for uint16 pixels, float32 for float32 pixels
    chi = stats.chi2.ppf(alpha, df=2)
    radius = np.sqrt(ore * n_nonzero / np.pi)
    if gaussian_sigma is None:
        if n_nonzero == 0:
            return None  # sigma = 0: the filter is exp(-0 / 0)
        sigma = float(radius / np.sqrt(chi))
    else:
        sigma = float(gaussian_sigma)
    hw = int(np.ceil(2 * radius))
    k = np.arange(-hw, hw + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    sum_h2 = np.sum(g * g) ** 2 / np.sum(g) ** 4
    g = g / np.sum(g)
    if image.dtype == np.float32:
        diff = (image - np.float32(med)).astype(np.float64)  # rounded to float32, as NumPy subtracts two float32
    else:
        diff = image.astype(np.float64) - float(med)
    return np.where(mask, diff, 0.0), g, sum_h2 * alpha * np.pi * chi * sigma**2


def nuc_est_conv(cell_mask, trap_image, **kwargs):
    p = parts(cell_mask, trap_image, **kwargs)
    if p is None:
        return float("nan")
    J, g, denominator = p
    rows = signal.correlate(J, g[None, :], mode="same", method="direct")
    resp = signal.correlate(rows, g[:, None], mode="same", method="direct")
    return float(np.max(resp) / denominator)


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _ellipse(shape, cy, cx, ry, rx):
    yy, xx = np.mgrid[0 : shape[0], 0 : shape[1]]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def _noise(seed, shape, lo=300, hi=900):
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.int64)


def _spot(shape, cy, cx, s, amp):
    yy, xx = np.mgrid[0 : shape[0], 0 : shape[1]]
    return amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(labels uint16 [F,Y,X], planes [F,C,Y,X] uint16 or float32, channel, kwargs).  Rows are (tile, label) for every
    label 1..max of every tile, the order of the object table.  Treat as read-only."""
    from aliby_amd import synth

    out = {}
    # 1. mixed batch: two synthetic tiles of 96 x 96, the `cells` labels, channel 1 of 2
    fovs = [synth.make_fov(2, k, shape=(96, 96), n_channels=2, n_z=1, n_target=8) for k in (0, 1)]
    lab = np.stack([f["cells"] for f in fovs]).astype(np.uint16)
    px = np.stack([f["pixels"][:, 0] for f in fovs]).astype(np.uint16)
    out["mixed_u16"] = dict(labels=lab, planes=px, channel=1, kwargs={})
    out["mixed_f32"] = dict(labels=lab, planes=(px.astype(np.float32) / np.float32(65535.0)).astype(np.float32), channel=1, kwargs={})
    # 7. keyword forms, on the same input
    out["kw_alpha_ore"] = dict(labels=lab, planes=px, channel=1, kwargs=dict(alpha=0.9, object_radius_estimation=0.2))
    out["kw_sigma"] = dict(labels=lab, planes=px, channel=1, kwargs=dict(gaussian_sigma=2.0))
    # 2. tile border: the "same" crop
    shape = (48, 56)
    lab = np.zeros(shape, np.uint16)
    lab[_ellipse(shape, 2, 3, 9.0, 7.0)] = 1
    lab[_ellipse(shape, 47, 55, 8.0, 11.0)] = 2
    img = _noise(21, shape) + _spot(shape, 1, 1, 2.0, 6000) + _spot(shape, 46, 54, 2.5, 9000)
    out["border"] = dict(labels=lab[None], planes=img.astype(np.uint16)[None, None], channel=0, kwargs={})
    # 3. tiny objects
    shape = (24, 24)
    lab = np.zeros(shape, np.uint16)
    lab[5, 5] = 1
    lab[10, 8:11] = 2
    lab[15:17, 15:17] = 3
    out["tiny"] = dict(labels=lab[None], planes=_noise(22, shape).astype(np.uint16)[None, None], channel=0, kwargs={})
    # 4. zeros inside the cell: N is half the area
    shape = (40, 40)
    lab = _ellipse(shape, 20, 19, 11.0, 13.0).astype(np.uint16)
    img = _noise(23, shape) + _spot(shape, 17, 22, 2.5, 5000)
    img[:, 1::2] = np.where(lab[:, 1::2] > 0, 0, img[:, 1::2])
    assert np.count_nonzero(img[lab > 0]) < 0.6 * int(lab.sum())
    out["zeros_inside"] = dict(labels=lab[None], planes=img.astype(np.uint16)[None, None], channel=0, kwargs={})
    # 5. undefined and degenerate: 1 = all-zero pixels, 2 = absent, 3 = uniform, 4 = an ordinary blob
    shape = (40, 48)
    lab = np.zeros(shape, np.uint16)
    lab[_ellipse(shape, 9, 10, 6.0, 7.0)] = 1
    lab[_ellipse(shape, 28, 12, 7.0, 6.0)] = 3
    lab[_ellipse(shape, 20, 34, 9.0, 8.0)] = 4
    img = _noise(24, shape) + _spot(shape, 22, 33, 2.0, 4000)
    img[lab == 1] = 0
    img[lab == 3] = 1234
    out["degenerate"] = dict(labels=lab[None], planes=img.astype(np.uint16)[None, None], channel=0, kwargs={})
    # 6. neighbours: two touching objects, the second 50 000 counts brighter; and the same with the second's pixels zeroed
    shape = (40, 44)
    lab = np.zeros(shape, np.uint16)
    both = _ellipse(shape, 20, 22, 12.0, 15.0)
    lab[both] = 1
    lab[both & (np.mgrid[0:40, 0:44][1] >= 22)] = 2
    img = _noise(25, shape) + _spot(shape, 18, 18, 2.0, 3000)
    bright = img + 50000 * (lab == 2)
    out["neighbours"] = dict(labels=lab[None], planes=bright.astype(np.uint16)[None, None], channel=0, kwargs={})
    out["neighbours_zeroed"] = dict(labels=lab[None], planes=np.where(lab == 2, 0, img).astype(np.uint16)[None, None], channel=0, kwargs={})
    # 8. one large object: a disc of radius 90 in a 200 x 200 tile
    shape = (200, 200)
    lab = _ellipse(shape, 100, 100, 90.0, 90.0).astype(np.uint16)
    img = _noise(26, shape) + _spot(shape, 80, 120, 25.0, 7000)
    out["disc90"] = dict(labels=lab[None], planes=img.astype(np.uint16)[None, None], channel=0, kwargs={})
    for s in out.values():
        s["labels"].setflags(write=False)
        s["planes"].setflags(write=False)
    return out


def rows(scene):
    """[(tile, label)] of a scene, in table order"""
    return [(f, l) for f in range(scene["labels"].shape[0]) for l in range(1, int(scene["labels"][f].max()) + 1)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement on every row of a scene -> float64 [n_rows]; computed once"""
    s = scenes()[name]
    res = np.array([nuc_est_conv(s["labels"][f] == l, s["planes"][f, s["channel"]], **s["kwargs"]) for f, l in rows(s)], np.float64)
    res.setflags(write=False)
    return res
