"""
Float64 reference of `FeatureEngine.coloc3d` (aliby_amd/csrc/feat_coloc3d.hip) and the inputs of its tests.

The reference drives oracle/cp_measure_restated.py the way the reference pipeline drives cp_measure and the 2-D GPU test does:
one binary mask per object, each of the four functions called on (pixels[c0], pixels[c1], mask).  Those functions index with a
boolean mask, so they take [Z,Y,X] arrays unchanged and see the object's voxels in raster order (z, y, x).
tests/test_cpu_coloc3d_ref.py pins this file to numpy.corrcoef / polyfit, closed forms and the oracle's own 2-D numbers.
Parity with cp_measure / CellProfiler on volumes is unpinned.

Costes' columns come out of a discrete search: every probe goes left or right on the sign of a Pearson value.  `costes_probes`
records that value for every probe of the reference's bisection, so that the CPU test can show that no input of the GPU tests
sits within rounding of a sign change (`cases()` lists those inputs; CPU and GPU tests build them from here).
"""
import contextlib

import numpy as np

from oracle import cp_measure_restated as cpm

METRICS = ("pearson", "manders_fold", "rwc", "costes")
COLUMNS = {"pearson": ["Correlation_Pearson", "Correlation_Slope"], "manders_fold": ["Correlation_Manders_1", "Correlation_Manders_2"],
           "rwc": ["Correlation_RWC_1", "Correlation_RWC_2"], "costes": ["Correlation_Costes_1", "Correlation_Costes_2"]}
NAMES = [n for m in METRICS for n in COLUMNS[m]]
PROBE_MARGIN = 1e-8  # three orders above eps * N = 2e-11, the rounding of a float64 correlation over 1e5 voxels


def _call(metric, p0, p1, mask, thr, scale_max):
    fn = cpm.get_correlation_measurements()[metric]
    if metric in ("manders_fold", "rwc"):
        return fn(p0, p1, mask, thr=thr)
    if metric == "costes":
        return fn(p0, p1, mask, scale_max=scale_max)
    return fn(p0, p1, mask)


def coloc3d(volume, p0, p1, n=None, metrics=METRICS, thr=15, scale_max=255) -> np.ndarray:
    """volume int [Z,Y,X] with labels 1..n, p0 / p1 [Z,Y,X] -> float64 [n, 2 * len(metrics)], row = label - 1; a label without
    voxels gives a row of NaN."""
    volume = np.asarray(volume)
    n = int(volume.max()) if n is None else int(n)
    out = np.full((n, 2 * len(metrics)), np.nan)
    for lab in range(1, n + 1):
        mask = volume == lab
        if not mask.any():
            continue
        one = mask.astype(np.uint16)
        for k, m in enumerate(metrics):
            res = _call(m, p0, p1, one, thr, scale_max)
            for j, name in enumerate(COLUMNS[m]):
                out[lab - 1, 2 * k + j] = np.asarray(res[name], float)[0]
    return out


def coloc3d_batch(vols, pixels, pairs, counts, metrics=METRICS, thr=15, scale_max=255) -> np.ndarray:
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] -> float64 [sum counts, 2 * len(metrics) * len(pairs)], pair-major columns."""
    rows = []
    for f, (v, c) in enumerate(zip(vols, counts)):
        rows.append(np.concatenate([coloc3d(v, pixels[f][a], pixels[f][b], c, metrics, thr, scale_max) for a, b in pairs], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 2 * len(metrics) * len(pairs)))


@contextlib.contextmanager
def _recorded_pearson(log):
    inner = cpm._pearsonr

    def recording(x, y):
        r = inner(x, y)
        log.append(float(r))
        return r

    cpm._pearsonr = recording
    try:
        yield
    finally:
        cpm._pearsonr = inner


def costes_probes(volume, p0, p1, n=None, scale_max=255):
    """-> one list per label: the Pearson value of every probe of the reference's Costes bisection for that object (NaN where a
    probe's voxels are constant in a channel; probes over two voxels or fewer evaluate none)."""
    volume = np.asarray(volume)
    n = int(volume.max()) if n is None else int(n)
    out = []
    for lab in range(1, n + 1):
        mask = volume == lab
        log = []
        if mask.any():
            with _recorded_pearson(log):
                cpm.get_correlation_costes(p0, p1, mask.astype(np.uint16), scale_max=scale_max)
        out.append(log)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def unit_float(pixels_u16) -> np.ndarray:
    """CellProfiler-style [0,1] floats of uint16 pixels: the case that exercises the Costes search properly."""
    return (np.asarray(pixels_u16).astype(np.float32) / np.float32(65535.0)).astype(np.float32)


def noise_pixels(seed, shape, n_channels=3) -> np.ndarray:
    """uint16 [C,Z,Y,X]: smoothed noise, every channel a mixture of a shared field and its own."""
    from scipy import ndimage as ndi

    rng = np.random.default_rng(1000 + seed)
    shared = ndi.gaussian_filter(rng.standard_normal(shape), (1.0, 2.0, 2.0))
    out = []
    for c in range(n_channels):
        own = ndi.gaussian_filter(rng.standard_normal(shape), (1.0, 1.5, 1.5))
        field = (0.7 - 0.2 * c) * shared / shared.std() + (0.5 + 0.2 * c) * own / own.std() + 0.05 * rng.standard_normal(shape)
        field = (field - field.min()) / (field.max() - field.min())
        out.append(np.round(500.0 + 40000.0 * field).astype(np.uint16))
    return np.stack(out)


def ellipsoids(n_z=12, shape=(128, 128), n_target=10):
    """-> (labels uint16 [Z,Y,X], n, pixels uint16 [3,Z,Y,X]): ellipsoids over the synthetic config-5 field of view."""
    from aliby_amd import synth

    f = synth.make_fov(5, 0, shape=shape, n_channels=3, n_z=n_z, n_target=n_target)
    vol = synth.ellipsoid_planes(f["nuclei"], n_z, seed=3).astype(np.uint16)
    return vol, int(vol.max()), f["pixels"]


def irregular(seed=1, shape=(32, 48, 56), n_seeds=12):
    """-> (labels, n, pixels uint16 [3,Z,Y,X]): touching irregular labels (tests/sizeshape3d_ref.random_labels), noise pixels."""
    from tests.sizeshape3d_ref import random_labels

    vol, n = random_labels(seed, shape, n_seeds=n_seeds)
    return vol, n, noise_pixels(seed, shape)


def budget_volume(lds_voxels=8192):
    """-> (labels, n, pixels uint16 [2,Z,Y,X], voxel counts): boxes of lds_voxels - 1000, exactly lds_voxels, lds_voxels + 1 and
    about 2.3 x lds_voxels voxels, and a small irregular piece: objects on both sides of the kernel's LDS budget, and at it."""
    side = int(round((lds_voxels / 8.0) ** (1.0 / 2.0)))  # lds_voxels = 8 * side * side for the default
    assert 8 * side * side == lds_voxels
    shape = (20, 2 * side + 8, 3 * side + 12)
    vol = np.zeros(shape, np.uint16)
    vol[1:9, 1:1 + side, 1:1 + side] = 1                      # exactly lds_voxels
    vol[1:9, 1:1 + side, 2 + side:2 + 2 * side] = 2           # lds_voxels + 1 (one voxel added below)
    vol[9, 1, 2 + side] = 2
    vol[11:19, 2 + side:2 + 2 * side, 1:1 + side] = 3         # lds_voxels - 1000 (a corner cut away below)
    vol[11:16, 2 + side:12 + side, 1:21] = 0
    vol[10:20, 2 + side:7 + 2 * side, 3 + side:3 + 3 * side] = 4  # 10 * (side + 5) * 2 side
    vol[0, -3:, -3:] = 5
    counts = np.bincount(vol.ravel())[1:]
    return vol, 5, noise_pixels(7, shape, 2), counts


def split_batch():
    """-> (vols [3][Z,Y,X], counts, pixels uint16 [3,2,Z,Y,X]): a stack with a label in two pieces, an empty stack, and a stack
    whose count announces two labels that have no voxels."""
    shape = (7, 61, 83)
    a, na, pa = irregular(11, shape)
    b, nb, pb = irregular(12, shape, n_seeds=9)
    centres = np.asarray([np.argwhere(a == k).mean(axis=0) for k in range(1, na + 1)])
    far = int(np.argmax(((centres - centres[0]) ** 2).sum(axis=1))) + 1
    split = a.copy()
    split[a == far] = 1
    split[a == na] = far if far != na else 1  # keep the labels sequential
    vols = [split, np.zeros(shape, np.uint16), b]
    counts = [na - 1, 0, nb + 2]
    return vols, counts, np.stack([pa[:2], noise_pixels(13, shape, 2), pb[:2]])


def edge_volume():
    """-> (labels, n, pixels uint16 [2,Z,Y,X]): label 1 a single voxel, label 2 an object inside which channel 0 is constant
    (one uint16 value, or its float32 quotient by 65535: every partial sum of at most 2^29 equal float32 values is exact in float64,
    so the mean is the value itself and every deviation exactly zero on both sides), label 3 an ordinary object."""
    shape = (6, 24, 40)
    vol = np.zeros(shape, np.uint16)
    vol[2, 3, 4] = 1
    vol[1:5, 8:20, 2:14] = 2
    vol[1:6, 6:22, 18:38] = 3
    px = noise_pixels(21, shape, 2)
    px[0][vol == 2] = 1234
    return vol, 3, px


def c_entry_case():
    """-> (labels uint16 [2,8,8], 1, pixels float32 [2,2,8,8] in [0,1]): the smallest call of the C entry, one object of 18 voxels."""
    vol = np.zeros((2, 8, 8), np.uint16)
    vol[:, 2:5, 2:5] = 1
    return vol, 1, unit_float(noise_pixels(41, (2, 8, 8), 2))


def segmenter_case():
    """-> (field of view, ground-truth labels [Z,Y,X], dP, prob): analytic 3-D flows for `dispatch_segmenter(volume_mode="flows3d")`."""
    from aliby_amd import synth

    f = synth.make_fov(5, 4, shape=(96, 112), n_channels=2, n_z=8, n_target=8)
    gt = synth.ellipsoid_planes(f["nuclei"], 8, seed=4)
    dP, prob = synth.analytic_flows_3d(gt)
    return f, gt, dP, prob


def cases():
    """Every (name, labels [Z,Y,X], n, pixels [C,Z,Y,X], pairs, scale_max, degenerate labels) the GPU tests compare on, except the
    segmenter's (its labels are computed: tests/test_cpu_coloc3d_ref.py builds them with tests/cellpose3d_ref.py).  `degenerate`
    names the labels built to have no defined correlation (one voxel, a constant channel)."""
    all3 = [(0, 1), (0, 2), (1, 2)]
    out = []
    vol, n, px = ellipsoids()
    out += [("ellipsoids u16", vol, n, px[:, :], all3, 255.0, ()), ("ellipsoids unit f32", vol, n, unit_float(px), all3, 255.0, ())]
    vol, n, px = irregular()
    out += [("irregular u16", vol, n, px, all3, 255.0, ()), ("irregular unit f32", vol, n, unit_float(px), all3, 255.0, ())]
    vol, n, px, _ = budget_volume()
    out += [("budget u16", vol, n, px, [(0, 1)], 255.0, ()), ("budget unit f32", vol, n, unit_float(px), [(0, 1)], 255.0, ())]
    vols, counts, px = split_batch()
    for f, (v, c) in enumerate(zip(vols, counts)):
        out.append((f"batch stack {f}", v, c, unit_float(px[f]), [(0, 1)], 255.0, ()))
    vol, n, px = irregular(21, (9, 50, 70))
    out.append(("reproducibility", vol, n, unit_float(px), [(0, 1), (2, 1)], 255.0, ()))
    vol, n, px = edge_volume()
    out += [("edges u16", vol, n, px, [(0, 1)], 255.0, (1, 2)), ("edges unit f32 scale 100", vol, n, unit_float(px), [(1, 0)], 100.0, (1, 2))]
    vol, n, px = irregular(31, (1, 64, 72), n_seeds=8)
    out.append(("one plane", vol, n, unit_float(px), [(0, 1)], 255.0, ()))
    vol, n, px = c_entry_case()
    out.append(("C entry", vol, n, px, [(0, 1)], 255.0, ()))
    return out
