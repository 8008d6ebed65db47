"""
The reference's in-repo functions that are not reached through the feature tree, with their own signatures:

  ratio(cell_mask, trap_image)            src/extraction/core/functions/cell.py:268-279
  nuc_est_conv(cell_mask, trap_image, ..) src/extraction/core/functions/custom/localisation.py:75-120
  nuc_conv_3d(cell_mask, trap_image, ..)  src/extraction/core/functions/custom/localisation.py:123-140
  imBackground(cell_masks, trap_image)    src/extraction/core/functions/trap.py:6-23
  background_max5(cell_masks, trap_image) src/extraction/core/functions/trap.py:26-43

  reduce_z(trap_image, fun, axis=0)       src/extraction/core/functions/distributors.py:6-24

Host arrays in, Python floats (reduce_z: a NumPy array of NumPy's own result dtype) out, the arithmetic in csrc/feat_extra.hip and
csrc/feat_localisation.hip (batched forms: FeatureEngine.cell_ratio / FeatureEngine.nuc_est_conv / FeatureEngine.nuc_conv_3d /
FeatureEngine.trap_background, which take a whole [F,Y,X] label stack).  No CPU fallback.
"""

from __future__ import annotations

import numpy as np
import torch

from aliby_amd.extraction.engine import FeatureEngine, to_device_planes, to_device_u16


def _as_pixels(a):
    """Float arrays that hold uint16-valued pixels go up as uint16: the kernels then divide / order them exactly as NumPy
    does in float64; anything else is float32 on the device."""
    a = np.asarray(a)
    if a.dtype.kind == "f" and a.size and np.isfinite(a).all() and a.min() >= 0 and a.max() <= 65535 and (a == np.rint(a)).all():
        return a.astype(np.uint16)
    return a


def ratio(cell_mask, trap_image) -> float:
    """Median ratio between two fluorescence channels of one cell; NaN unless trap_image is [Y, X, 2] (cell.py:270-279)."""
    trap_image = _as_pixels(trap_image)
    if not (trap_image.ndim == 3 and trap_image.shape[-1] == 2):
        return float("nan")
    eng = FeatureEngine()
    labels = to_device_u16(np.asarray(cell_mask, dtype=bool).astype(np.uint16)[None])
    planes, dt = to_device_planes(np.moveaxis(trap_image, -1, 0)[None])  # [1, 2, Y, X]
    table = eng.object_table(labels)
    if table.n_obj == 0:
        return float("nan")  # np.median of an empty selection
    return float(eng.cell_ratio(labels, planes, dt, 0, 1, table)[0])


def nuc_est_conv(cell_mask, trap_image, alpha=0.95, object_radius_estimation=0.085, gaussian_filter_shape=None, gaussian_sigma=None) -> float:
    """Nuclear localisation of one cell: the maximum of its median-subtracted pixels convolved with a Gaussian sized to the
    expected nucleus, normalised (localisation.py:75-120).  gaussian_filter_shape is accepted and ignored: the reference
    overwrites it with (2 ceil(2 r) + 1,) * 2.  NaN for an empty mask and for a cell without a non-zero pixel."""
    trap_image = _as_pixels(trap_image)
    if trap_image.ndim != 2:
        raise ValueError(f"trap_image must be [Y, X], got shape {trap_image.shape}")
    eng = FeatureEngine()
    labels = to_device_u16(np.asarray(cell_mask, dtype=bool).astype(np.uint16)[None])
    planes, dt = to_device_planes(trap_image[None, None])  # [1, 1, Y, X]
    table = eng.object_table(labels)
    if table.n_obj == 0:
        return float("nan")  # np.median of an empty selection
    out = eng.new_output(1, 1)
    eng.nuc_est_conv(labels, planes, dt, 0, table, out, 0, alpha=alpha, object_radius_estimation=object_radius_estimation,
                     gaussian_sigma=gaussian_sigma)
    return float(out[0, 0])


def nuc_conv_3d(cell_mask, trap_image, pixel_size=0.23, z_spacing=0.6) -> float:
    """Nuclear localisation of one cell over a Z stack: cell_mask [Y, X] is repeated on every plane of trap_image [Z, Y, X], and
    the maximum of the median-subtracted voxels convolved with the reference's 3-D Gaussian, sized to the expected nucleus, is
    normalised (localisation.py:123-140).  NaN for an empty mask and for a cell without a non-zero voxel."""
    trap_image = _as_pixels(trap_image)
    if trap_image.ndim != 3:
        raise ValueError(f"trap_image must be [Z, Y, X], got shape {trap_image.shape}")
    cell_mask = np.asarray(cell_mask, dtype=bool)
    if cell_mask.shape != trap_image.shape[1:]:
        raise ValueError(f"cell_mask {cell_mask.shape} does not match the planes of trap_image {trap_image.shape}")
    eng = FeatureEngine()
    labels = to_device_u16(cell_mask.astype(np.uint16)[None])
    stack, dt = to_device_planes(trap_image[None, None])  # [1, 1, Z, Y, X]
    table = eng.object_table(labels)
    if table.n_obj == 0:
        return float("nan")  # np.median of an empty selection
    out = eng.new_output(1, 1)
    eng.nuc_conv_3d(labels, stack, dt, 0, table, out, 0, pixel_size=pixel_size, z_spacing=z_spacing)
    return float(out[0, 0])


def _label_tile(name: str, labels):
    labels = np.asarray(labels)
    if labels.ndim != 2:
        raise ValueError(f"{name} must be one [Y, X] label image, got shape {labels.shape}")
    return to_device_u16(labels[None])


def relate_objects(child_labels, parent_labels):
    """Two label images [Y, X] of one tile (0 = background, labels 1..n) -> (children, parents), float64 [n, 5] each on the host: the
    rows of the first set relative to the second and of the second relative to the first, columns as `features.relate_names`
    (Parent, ParentOverlap, Children count, Distance_Centroid, Distance_Minimum; FeatureEngine.relate, csrc/feat_relate.hip).  Not in
    the reference: CellProfiler's RelateObjects, PARITY UNPINNED (include/aliby_hip.h)."""
    a, b = _label_tile("child_labels", child_labels), _label_tile("parent_labels", parent_labels)
    if a.shape != b.shape:
        raise ValueError(f"child_labels {tuple(a.shape[1:])} and parent_labels {tuple(b.shape[1:])} differ in shape")
    eng = FeatureEngine()
    rows_a, rows_b = eng.relate(a, eng.object_table(a), b, eng.object_table(b))
    return eng.to_host(rows_a), eng.to_host(rows_b)


def tertiary_objects(outer, inner, shrink_inner=True) -> np.ndarray:
    """Two label images [Y, X] of one tile -> uint16 [Y, X]: `outer`'s labels where `inner` is 0 or, with shrink_inner, on the outline
    of an inner object; 0 elsewhere (FeatureEngine.tertiary_labels, csrc/feat_relate.hip).  The cytoplasm is
    tertiary_objects(cells, nuclei).  Not in the reference: CellProfiler's IdentifyTertiaryObjects, PARITY UNPINNED."""
    a, b = _label_tile("outer", outer), _label_tile("inner", inner)
    if a.shape != b.shape:
        raise ValueError(f"outer {tuple(a.shape[1:])} and inner {tuple(b.shape[1:])} differ in shape")
    eng = FeatureEngine()
    return eng.tertiary_labels(a, b, shrink_inner=shrink_inner)[0].cpu().numpy()


def secondary_objects(primary_labels, distance) -> np.ndarray:
    """One label image [Y, X] -> uint16 [Y, X]: every object grown by up to `distance` pixels (an integer in 1..64) into the
    background, a grown pixel taking the label of the nearest labelled pixel, ties to the smaller label
    (FeatureEngine.secondary_labels, csrc/feat_secondary.hip).  The cell around a nucleus is secondary_objects(nuclei, 10), and the
    cytoplasm tertiary_objects(that, nuclei).  Not in the reference: CellProfiler's IdentifySecondaryObjects, method "Distance - N",
    equal to scipy's distance_transform_edt index gather except on ties (include/aliby_hip.h)."""
    return FeatureEngine().secondary_labels(_label_tile("primary_labels", primary_labels), distance)[0].cpu().numpy()


def auto_threshold(image, method="otsu", classes=2, middle=None, correction=1.0, bounds=(0, 65535)) -> int:
    """One uint16 image [Y, X] -> its automatic threshold, a Python int: Otsu's threshold with two or three classes over all the
    image's pixels, times `correction`, clamped to `bounds` (FeatureEngine.auto_threshold, csrc/feat_threshold.hip; the arguments are
    those of features.auto_threshold_args).  Not in the reference: CellProfiler's automatic threshold of IdentifySecondaryObjects,
    PARITY UNPINNED (the definition is in include/aliby_hip.h)."""
    image = np.asarray(image)
    if image.dtype != np.uint16 or image.ndim != 2:
        raise ValueError(f"image must be one uint16 [Y, X] image (float32 images are not built), got {image.dtype} {image.shape}")
    if image.size == 0:
        raise ValueError("image holds no pixel: it has no threshold")
    return int(FeatureEngine().auto_threshold(to_device_u16(image[None]), method, classes, middle, correction, bounds).cpu()[0])


def propagate_objects(primary_labels, image, threshold=0, regularization=0.05, distance=None, image_max=65535,
                      auto_threshold=None) -> np.ndarray:
    """One label image [Y, X] and one uint16 stain image [Y, X] -> uint16 [Y, X]: the labels grown along the stain, every passable
    pixel (labelled, or image >= threshold and, with `distance`, within that many pixels of a labelled one) taking the label of the
    cheapest path over the integer metric of include/aliby_hip.h, ties to the smaller label (FeatureEngine.propagate_labels,
    csrc/feat_propagate.hip).  The cell around a nucleus is propagate_objects(nuclei, cell_stain, threshold=t), and the cytoplasm
    tertiary_objects(that, nuclei).  Not in the reference: CellProfiler's IdentifySecondaryObjects, method "Propagation" (with a
    distance and threshold 0: "Distance - B"), PARITY UNPINNED.  `auto_threshold`: an option dict of features.auto_threshold_args
    ({} for two-class Otsu) — the threshold is then the image's own, computed and used on the device; together with a non-zero
    `threshold` it is a ValueError."""
    from aliby_amd.extraction.features import auto_threshold_options, propagate_args

    image = np.asarray(image)
    if image.dtype != np.uint16 or image.ndim != 2:
        raise ValueError(f"image must be one uint16 [Y, X] image (float32 images are not built), got {image.dtype} {image.shape}")
    checked = propagate_args(threshold, regularization, distance, image_max)
    auto = None if auto_threshold is None else auto_threshold_options(auto_threshold)
    if auto is not None and checked.threshold != 0:
        raise ValueError(f"give threshold or auto_threshold, not both (threshold={threshold!r})")
    engine, stain = FeatureEngine(), to_device_u16(image[None])
    thresholds = None if auto is None else engine.auto_threshold(stain, **auto._asdict())
    return engine.propagate_labels(_label_tile("primary_labels", primary_labels), stain, threshold, regularization, distance, image_max,
                                   thresholds=thresholds)[0].cpu().numpy()


def _label_stack(name: str, labels):
    labels = np.asarray(labels)
    if labels.ndim != 3:
        raise ValueError(f"{name} must be one [Z, Y, X] label stack, got shape {labels.shape}")
    return to_device_u16(labels[None]), int(labels.max()) if labels.size else 0


def relate_objects_3d(child_labels, parent_labels, spacing=(1.0, 1.0, 1.0)):
    """Two label stacks [Z, Y, X] of one shape (0 = background, labels 1..n) -> (children, parents), float64 [n, 5] each on the host:
    the volume form of `relate_objects` (FeatureEngine.relate3d, csrc/feat_relate3d.hip), overlaps in voxels and distances in the units
    of `spacing` = (dz, dy, dx).  Not in the reference: CellProfiler's RelateObjects, PARITY UNPINNED (include/aliby_hip.h)."""
    (a, na), (b, nb) = _label_stack("child_labels", child_labels), _label_stack("parent_labels", parent_labels)
    if a.shape != b.shape:
        raise ValueError(f"child_labels {tuple(a.shape[1:])} and parent_labels {tuple(b.shape[1:])} differ in shape")
    eng = FeatureEngine()
    rows_a, rows_b = eng.relate3d(a, [na], b, [nb], spacing=spacing)
    return eng.to_host(rows_a), eng.to_host(rows_b)


def tertiary_objects_3d(outer, inner, shrink_inner=True) -> np.ndarray:
    """Two label stacks [Z, Y, X] of one shape -> uint16 [Z, Y, X]: `outer`'s labels where `inner` is 0 or, with shrink_inner, on the
    plane-by-plane outline of an inner object; 0 elsewhere (FeatureEngine.tertiary_volume).  The cytoplasm of a stack is
    tertiary_objects_3d(cells, nuclei).  Not in the reference: CellProfiler's IdentifyTertiaryObjects, PARITY UNPINNED."""
    (a, _), (b, _) = _label_stack("outer", outer), _label_stack("inner", inner)
    if a.shape != b.shape:
        raise ValueError(f"outer {tuple(a.shape[1:])} and inner {tuple(b.shape[1:])} differ in shape")
    return FeatureEngine().tertiary_volume(a, b, shrink_inner=shrink_inner)[0].cpu().numpy()


def secondary_objects_3d(volume_labels, distance, spacing=(1, 1, 1)) -> np.ndarray:
    """One label stack [Z, Y, X] -> uint16 [Z, Y, X]: every object grown by up to `distance` into the background on the integer
    lattice `spacing` = (sz, sy, sx), a grown voxel taking the label of the nearest labelled voxel, ties to the smaller label
    (FeatureEngine.secondary_volume, csrc/feat_secondary3d.hip; the limits: features.secondary_volume_args).  The cell around a
    nucleus of a stack is secondary_objects_3d(nuclei, 10), and its cytoplasm tertiary_objects_3d(that, nuclei).  Not in the
    reference: the volume form of `secondary_objects`, equal to scipy's distance_transform_edt(sampling=) index gather except on ties
    (include/aliby_hip.h)."""
    return FeatureEngine().secondary_volume(_label_stack("volume_labels", volume_labels)[0], distance, spacing)[0].cpu().numpy()


def _background(cell_masks, trap_image):
    trap_image = _as_pixels(trap_image)
    if not len(cell_masks):
        covered = np.zeros(trap_image.shape, bool)  # "create cell_masks if none are given"
    else:
        covered = np.asarray(cell_masks).sum(axis=2).astype(bool)
    eng = FeatureEngine()
    labels = to_device_u16(covered.astype(np.uint16)[None])
    planes, dt = to_device_planes(trap_image[None, None])
    return eng.trap_background(labels, planes, dt, 0)[0]


def imBackground(cell_masks, trap_image) -> float:
    """Median of the pixels not comprising cells (cell_masks [Y, X, N], one mask per cell)."""
    return float(_background(cell_masks, trap_image)[0])


def background_max5(cell_masks, trap_image) -> float:
    """Mean of the maximum five pixels of the background."""
    return float(_background(cell_masks, trap_image)[1])


_UFUNCS = {"maximum": 0, "add": 1, "divide": 2, "true_divide": 2}


def reduce_z(trap_image, fun, axis: int = 0):
    """`fun.reduce(trap_image, axis=axis)` for the reducers the reference registers (loaders.py:110-127: np.maximum, np.add,
    np.divide) with NumPy's result dtypes — uint16 input: uint16 / uint64 / float64; float32 input: float32 — and the
    reference's error for anything that is not a ufunc (distributors.py:20-24).  A 2-D image comes back as it is."""
    from aliby_amd import _lib

    if isinstance(fun, np.ufunc):
        op = _UFUNCS.get(fun.__name__)
        if op is None:
            raise NotImplementedError(f"reduce_z: ufunc {fun.__name__} is not one of the reducers the pipeline registers (max / add / div)")
    else:
        raise Exception(f"Operator {fun} is an invalid reducer.")
    a = np.asarray(trap_image)
    if a.ndim <= 2:
        return a
    if a.dtype not in (np.uint16, np.float32):
        a = a.astype(np.uint16 if a.dtype in (np.uint8, np.bool_) else np.float32)
    moved = np.ascontiguousarray(np.moveaxis(a, axis, 0))  # [Z, ...]
    Z, rest = moved.shape[0], moved.shape[1:]
    dev = torch.from_numpy(moved).cuda()
    u16 = moved.dtype == np.uint16
    in_dt = _lib.U16 if u16 else _lib.F32
    out_dt = in_dt if op == 0 else _lib.F32 if not u16 else _lib.U64 if op == 1 else _lib.F64
    return FeatureEngine().reduce_z(dev.reshape(Z, 1, int(np.prod(rest, dtype=np.int64))), op, in_dt, out_dt).reshape(rest).cpu().numpy()
