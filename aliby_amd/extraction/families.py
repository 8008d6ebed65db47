"""
Metric registry: instruction -> HIP kernel launch(es) writing a block of columns.

Plays the role of the reference's CELL_FUNS / REDUCTION_FUNS registries
(src/extraction/core/functions/loaders.py:28-79,110-127): names are the cp_measure feature names
bound at loaders.py:71-77 plus the in-repo cell.py metrics (loaders.py:19-25).  A name that is not
registered raises KeyError, as `CELL_FUNS[metric]` does (extract.py:147-153).

`evaluate` is `plan` (pure: no engine, table or tensor) followed by one executor for the single-channel and one for the
channel-pair instructions; tests/test_cpu_feature_dispatch.py replays both on a recording engine.

The volume families (label-keyed measurements of Z-stacks kept as volumes) have a registry, a planner and an evaluator of their own
at the end of the module: `VOLUME`, `VOLUME_PAIRS`, `plan_volume`, `evaluate_volume` (tests/test_cpu_volume_tree.py).
"""

from __future__ import annotations

import os
from contextlib import nullcontext
from dataclasses import dataclass, field, replace
from typing import Callable

import torch

from aliby_amd import _lib
from aliby_amd.extraction import features as feat

_RED = {"max": _lib.RED_MAX, "add": _lib.RED_ADD, "div": _lib.RED_DIV}


class PlaneCache:
    """z-reduced planes [F,C,Y,X], one reduction per distinct red_z instead of one per call
    (the reference redoes it for every object x instruction, extract.py:105-107)."""

    def __init__(self, eng, planes):
        self.eng = eng
        self.tensor, self.dtype = planes  # [F,C,Z,Y,X]
        if self.tensor.ndim != 5:
            raise Exception(f"pixels must be [F,C,Z,Y,X], got {tuple(self.tensor.shape)}")
        self._cache = {}

    def get(self, red_z):
        if red_z in self._cache:
            return self._cache[red_z]
        if red_z not in _RED:
            # np.mean / np.median / None are not ufuncs: distributors.py:20-24 raises
            raise Exception(f"{red_z} is an invalid reducer.")
        F, C, Z, Y, X = self.tensor.shape
        op = _RED[red_z]
        if Z == 1 and op == _lib.RED_MAX:
            out, dt = self.tensor.reshape(F, C, Y, X), self.dtype
        else:
            # np.add.reduce(uint16) is exact uint64 and np.divide.reduce float64 (distributors.py:22-24); the feature kernels
            # read uint16 or float32 planes.  Sums of uint16 are exact in float32 while Z * 65535 < 2^24 (Z <= 256): beyond
            # that the plane would silently lose bits, so it is refused.  "div" results carry float32 rounding (6e-8
            # relative, three orders inside the 1e-4 feature tolerance).
            integer = self.dtype in (_lib.U16, _lib.U8W)
            if op == _lib.RED_ADD and integer and Z * 65535 >= (1 << 24):
                raise NotImplementedError(f"reduce_z 'add' over Z={Z} uint16 planes exceeds the exact float32 range (Z <= 256)")
            dt = self.dtype if op == _lib.RED_MAX else _lib.F32
            # (the maximum over z of 8-bit values is still 8-bit: the code U8W stays on the plane for the texture kernel)
            out = self.eng.reduce_z(self.tensor, op, _lib.U16 if integer else _lib.F32, _lib.U16 if dt != _lib.F32 else _lib.F32)
        self._cache[red_z] = (out, dt)
        return out, dt


# The [n_obj, 17] cell.py blocks of one evaluation: every metric of a (plane, channel) comes from ONE launch of k_cell
# (FeatureEngine.cell_metrics).  Handed to every launcher; the cell.py metrics and nuc_est_conv's median read it.
class _CellBlocks:
    def __init__(self, eng, labels, table):
        self.eng, self.labels, self.table = eng, labels, table
        self._blocks = {}

    def column(self, plane, dt, ch, metric):
        key = None if plane is None else (plane.data_ptr(), ch)
        if key not in self._blocks:
            self._blocks[key] = self.eng.cell_metrics(self.labels, plane, dt, ch, self.table)
        return self._blocks[key][:, self.eng.CELL_COLUMNS.index(metric)]


@dataclass(frozen=True)
class Family:  # one registered metric
    # names(kw) -> the keys of its columns, or None for a scalar (one column, named after the metric)
    names: Callable
    # launch(eng, labels, table, plane, dt, ch, out, col0, kw, cells) writes out[:, col0:...]; plane / dt / ch are None / 0 / None
    # for a family without pixels, kw holds keywords of BUILT_KWARGS only (`plan` refuses the rest), `cells` is the evaluation's
    # _CellBlocks.  None for the channel-pair metrics, which are launched in groups (`Plan.batches`).
    launch: Callable | None = None
    needs_pixels: bool = True
    # launched on the main stream after the fan-out has joined: the cell.py metrics share cached blocks, granularity iterates to a
    # fixed point and waits on its stream in between, large objects of nuc_conv_3d take the global-scratch form
    after_join: bool = False
    # handed the un-reduced [F,C,Z,Y,X] stack instead of one z-reduced plane; valid only under a channel with the reducer key
    # "None", ALIBY's spelling of "do not reduce" (the reference's reduce_z raises on it, and upstream reaches the function through
    # its custom loader).  Every other metric under "None" keeps raising "invalid reducer".
    stack: bool = False


def _scalar(kw):
    return None


def _launch_intensity(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.intensity(labels, plane, dt, ch, table, out, col0, **kw)


def _launch_sizeshape(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.sizeshape(labels, table, out, col0)


def _launch_feret(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.feret(labels, table, out, col0)


def _launch_neighbors(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    # (`plan` has refused every keyword but `distance`: the "expand" method and a second object set are not built)
    eng.neighbors(labels, table, out, col0, **kw)


def _launch_zernike(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.zernike(labels, None, 0, 0, table, out, col0, weighted=False)


def _launch_radial_zernikes(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.zernike(labels, plane, dt, ch, table, out, col0, weighted=True)


def _launch_texture(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.texture(labels, plane, dt, ch, table, out, col0, **kw)


def _launch_radial_distribution(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    eng.radial_distribution(labels, plane, dt, ch, table, out, col0, **kw)


def _launch_granularity(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    if kw.get("image_mask", "frame") != "frame":
        # the reference measures one object at a time on a single-object label image (extract.py:147-153): with the objects as
        # the image mask, every object would get its own background and spectrum images.  Not built.
        raise NotImplementedError("granularity(image_mask='objects') through the extraction tree is not built: the batched "
                                  "kernels share one image-level spectrum per tile (image_mask='frame', CellProfiler's default)")
    eng.granularity(labels, plane, dt, ch, table, out, col0, **kw)


def _make_cell_launch(metric):
    def launch(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
        out[:, col0] = cells.column(plane, dt, ch, metric)

    return launch


def _launch_nuc_est_conv(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    # custom/localisation.py, with its defaults (an entry of cp_measure_kwargs named after an in-repo function is not looked at).
    # The median it subtracts is a column of the (plane, channel)'s cell.py block, shared with the cell.py metrics.
    if plane is None:
        raise Exception("nuc_est_conv needs the pixels of a channel")
    eng.nuc_est_conv(labels, plane, dt, ch, table, out, col0, median=cells.column(plane, dt, ch, "median"))


def _launch_nuc_conv_3d(eng, labels, table, stack, dt, ch, out, col0, kw, cells):
    # custom/localisation.py:123-140, with its defaults.  `stack` is the un-reduced [F,C,Z,Y,X] block (Family.stack).
    eng.nuc_conv_3d(labels, stack, dt, ch, table, out, col0)


def _launch_ratio(eng, labels, table, plane, dt, ch, out, col0, kw, cells):
    # cell.ratio needs a [Y, X, 2] image (cell.py:270); the extraction path hands every metric ONE z-reduced plane, so the
    # reference returns NaN for every object here.  The two-channel form is FeatureEngine.cell_ratio / functions.ratio.
    out[:, col0] = float("nan")


MONO = {
    "intensity": Family(lambda kw: feat.intensity_names(kw.get("edge_measurements", True)), _launch_intensity),
    "sizeshape": Family(lambda kw: feat.sizeshape_names(), _launch_sizeshape, needs_pixels=False),
    "feret": Family(lambda kw: feat.feret_names(), _launch_feret, needs_pixels=False),
    "zernike": Family(lambda kw: feat.zernike_names(), _launch_zernike, needs_pixels=False),
    "radial_zernikes": Family(lambda kw: feat.radial_zernike_names(), _launch_radial_zernikes),
    "texture": Family(lambda kw: feat.texture_names(kw.get("scale", 3), kw.get("gray_levels", 256)), _launch_texture),
    "radial_distribution": Family(lambda kw: feat.radial_distribution_names(kw.get("bin_count", 4), kw.get("scaled", True)),
                                  _launch_radial_distribution),
    "granularity": Family(lambda kw: feat.granularity_names(kw.get("granular_spectrum_length", 16)), _launch_granularity,
                          after_join=True),
    "ratio": Family(_scalar, _launch_ratio),
    # extensions of this fork's registry: the reference reaches the two functions through its custom loader, not load_cellfuns_core
    "nuc_est_conv": Family(_scalar, _launch_nuc_est_conv, after_join=True),
    "nuc_conv_3d": Family(_scalar, _launch_nuc_conv_3d, after_join=True, stack=True),
    # cp_measure's multi-mask measurement of that name (CellProfiler's MeasureObjectNeighbors), with the objects as their own
    # neighbours; the reference's loader does not bind it.  Parity unpinned (features.neighbors_names)
    "neighbors": Family(lambda kw: feat.neighbors_names(kw.get("distance")), _launch_neighbors, needs_pixels=False),
}
# cell.py metrics (loaders.py:19-25): scalar results, one column each
for _m in ("area", "centroid_x", "centroid_y", "conical_volume", "eccentricity", "spherical_volume", "volume"):
    MONO[_m] = Family(_scalar, _make_cell_launch(_m), needs_pixels=False, after_join=True)
for _m in ("mean", "median", "std", "total", "total_squared", "max2p5pc", "max5px_median", "moment_of_inertia"):
    MONO[_m] = Family(_scalar, _make_cell_launch(_m), after_join=True)
MULTI = {name: Family(lambda kw, _n=name: list(feat.COLOC[_n])) for name in feat.COLOC}


def register_optional(eng_cls):
    """Does nothing: every family is registered when this module is imported.  Kept because the benchmark calls it."""


class _FanOut:
    """Per-object kernels are one small workgroup per object: latency-bound and far from filling 256 CUs, so
    independent instructions (different channels / families / channel pairs) go to a few side HIP streams and run
    concurrently.  fork(): side streams wait for the main stream; join(): the main stream waits for them.  Only
    taken when every object window is LDS-resident (ObjectTable.lds_resident): a global-scratch launch borrows the context's
    scratch, so only one may be in flight per context (the rule, and what this condition does and does not guarantee:
    aliby_amd/csrc/object_launch.h)."""

    def __init__(self, eng, table, out):
        n = int(os.environ.get("ALIBY_FEATURE_STREAMS", "4"))
        self.enabled = n > 1 and table.lds_resident and out.is_cuda
        self.out = out
        self.k = 0
        if self.enabled:
            pool = eng.__dict__.setdefault("_side_streams", [])
            while len(pool) < n:
                pool.append(torch.cuda.Stream())
            self.streams = pool[:n]
            self.used = set()

    def fork(self):
        if self.enabled:
            ev = torch.cuda.Event()
            ev.record()
            for st in self.streams:
                st.wait_event(ev)

    def next_stream(self):
        if not self.enabled:
            return nullcontext()
        i = self.k % len(self.streams)
        self.k += 1
        self.used.add(i)
        self.out.record_stream(self.streams[i])
        return torch.cuda.stream(self.streams[i])

    def join(self):
        if self.enabled:
            main = torch.cuda.current_stream()
            for i in sorted(self.used):
                ev = torch.cuda.Event()
                ev.record(self.streams[i])
                main.wait_event(ev)
            self.used.clear()


# the cp_measure functions: those the reference takes from it (get_core_measurements / get_correlation_measurements,
# loaders.py:71-77), and "neighbors", a cp_measure function the reference does not bind and this registry adds.  Only their entries
# of cp_measure_kwargs are ever looked at; an entry named after one of the in-repo functions is ignored
CP_MEASURE_NAMES = ("intensity", "sizeshape", "zernike", "feret", "texture", "radial_distribution", "radial_zernikes", "granularity",
                    "pearson", "manders_fold", "rwc", "costes", "neighbors")
# per-feature keywords (cp_measure_kwargs / cp_measure_feature_kwargs of the builder) that the kernels implement
BUILT_KWARGS = {
    "intensity": ("edge_measurements",),
    "texture": ("scale", "gray_levels"),
    "radial_distribution": ("bin_count", "scaled", "maximum_radius"),
    "granularity": ("subsample_size", "image_sample_size", "element_size", "granular_spectrum_length", "image_mask", "mask_order"),
    "manders_fold": ("thr",),
    "rwc": ("thr",),
    "costes": ("scale_max",),
    "neighbors": ("distance",),
}

LAUNCH, COPY, GROUP = "launch", "copy", "group"


@dataclass(frozen=True)
class Step:
    """One instruction of a plan: its registry entry, its keywords and its columns [col0, col0 + ncols)."""

    inst: tuple
    family: Family
    kw: dict
    col0: int
    ncols: int
    # single-channel plans: LAUNCH on its own; COPY, its columns are in `Plan.copies`; GROUP, a member of `Plan.zernike_groups`
    role: str = LAUNCH


@dataclass(frozen=True)
class Plan:
    blocks: list  # per instruction (first column, names | None): the second return value of `evaluate`
    n_cols: int
    steps: list
    # single-channel instructions
    copies: list = field(default_factory=list)  # (first column, source column, columns), after the join
    zernike_groups: dict = field(default_factory=dict)  # red_z -> [(channel, first column)]: channels of one plane block, one launch
    # channel pairs, in launch order
    prefetch: list = field(default_factory=list)  # (red_z, pair, whether its rank planes are needed) on the main stream
    batches: dict = field(default_factory=dict)  # (red_z, thr, scale_max) -> [(pair, {metric: first column})]: one launch each


def plan(instructions, cp_measure_kwargs, multi=False) -> Plan:
    """What `evaluate` will do for these instructions, and every refusal that depends on the names and keywords alone."""
    blocks, steps = [], []
    col = 0
    for inst in instructions:
        metric = inst[-1]
        kw = dict(cp_measure_kwargs.get(metric, {}))
        reg = MULTI if (multi and inst[1] == "None") else MONO
        if metric not in reg:
            raise KeyError(metric)
        # the reference forwards these to the cp_measure function of that name (loaders.py:71-77), where an unknown keyword is an
        # error; here a keyword the kernels do not implement must not be dropped either
        unbuilt = sorted(set(kw) - set(BUILT_KWARGS.get(metric, ()))) if metric in CP_MEASURE_NAMES else ()
        if unbuilt:
            raise NotImplementedError(f"cp_measure_kwargs[{metric!r}]: {unbuilt} not built (built: {sorted(BUILT_KWARGS.get(metric, ()))})")
        if reg[metric].stack and (inst[0] == "None" or inst[1] != "None"):
            raise Exception(f"{metric} needs the un-reduced stack of a channel: list it under a channel with the reducer key "
                            f"'None', not under {inst[0]!r} / {inst[1]!r}")
        names = reg[metric].names(kw)
        ncols = 1 if names is None else len(names)
        blocks.append((col, names))
        steps.append(Step(inst, reg[metric], kw, col, ncols))
        col += ncols
    return (_plan_multi if multi else _plan_mono)(blocks, col, steps)


def _plan_mono(blocks, n_cols, steps) -> Plan:
    done = {}  # (metric, kwargs) of pixel-independent families already launched -> first column
    copies, zernike_groups = [], {}
    sizeshape_col0 = next((s.col0 for s in steps if s.inst[-1] == "sizeshape"), None)
    for k, s in enumerate(steps):
        ch, red_z, metric = s.inst[0], s.inst[1], s.inst[-1]
        role = LAUNCH  # (also what a family that runs after the join keeps)
        if not s.family.after_join and (ch == "None" or not s.family.needs_pixels):
            key = (metric, tuple(sorted(s.kw.items())))
            if metric == "feret" and sizeshape_col0 is not None:
                # the two Feret diameters are columns of the sizeshape block (one hull kernel writes both): copy them
                ss = feat.sizeshape_names()
                copies.extend((s.col0 + j, sizeshape_col0 + ss.index(name), 1) for j, name in enumerate(feat.feret_names()))
                role = COPY
            elif key in done:
                # e.g. "feret"/"zernike" listed under every channel: same labels, same numbers
                copies.append((s.col0, done[key], s.ncols))
                role = COPY
            else:
                done[key] = s.col0
        elif not s.family.after_join and metric == "radial_zernikes":
            zernike_groups.setdefault(red_z, []).append((ch, s.col0))
            role = GROUP
        steps[k] = replace(s, role=role)
    return Plan(blocks, n_cols, steps, copies=copies, zernike_groups=zernike_groups)


def _plan_multi(blocks, n_cols, steps) -> Plan:
    groups = {}  # (pair, red_z) -> [(metric, first column, thr, scale_max)]: every requested metric of that pair together
    for s in steps:
        (ch0, ch1), red_ch, red_z, metric = s.inst[0], s.inst[1], s.inst[2], s.inst[3]
        if red_ch != "None":
            raise NotImplementedError("channel-combining multi instructions (extract.py:227-235) are not built; "
                                      "the builder only emits red_ch='None' (pipe_builder.py:33-43)")
        # kwargs are per feature name, as the reference bakes them into one partial per name (loaders.py:71-77):
        # manders_fold's thr must not leak into rwc.  The kernel takes one thr per launch, so metrics of a pair whose
        # thresholds differ go to separate launches.
        thr = float(s.kw.get("thr", 15.0)) if metric in ("manders_fold", "rwc") else None
        scale_max = float(s.kw.get("scale_max", 255.0)) if metric == "costes" else None
        groups.setdefault(((ch0, ch1), red_z), []).append((metric, s.col0, thr, scale_max))
    prefetch, batches = [], {}
    for (pair, red_z), entries in groups.items():
        thrs = sorted({t for _, _, t, _ in entries if t is not None}) or [15.0]
        scale_max = next((sm for _, _, _, sm in entries if sm is not None), 255.0)
        for k, thr in enumerate(thrs):  # threshold-free metrics ride with the first threshold's launch
            cols = {m: c for m, c, t, _ in entries if t == thr or (t is None and k == 0)}
            prefetch.append((red_z, pair, "rwc" in cols))
            # every pair that shares a z-reduction and its parameters goes into one launch (csrc/feat_coloc.hip, k_coloc_pairs)
            batches.setdefault((red_z, thr, scale_max), []).append((pair, cols))
    return Plan(blocks, n_cols, steps, prefetch=prefetch, batches=batches)


def evaluate(eng, labels, table, planes, instructions, cp_measure_kwargs, multi=False):
    """Run every instruction over every object; returns (matrix [n_obj, n_cols] on device, blocks)."""
    p = plan(instructions, cp_measure_kwargs, multi)
    out = eng.new_output(table.n_obj, p.n_cols)
    cache = PlaneCache(eng, planes) if planes is not None else None
    (_run_multi if multi else _run_mono)(eng, labels, table, cache, out, _FanOut(eng, table, out), p)
    return out, p.blocks


def _run_multi(eng, labels, table, cache, out, fan, p):
    if cache is None:
        raise Exception("pixels are required for colocalisation instructions")
    for red_z, pair, ranks in p.prefetch:  # shared inputs first, on the main stream: z-reduction, rank planes
        plane, dt = cache.get(red_z)
        if ranks:
            eng.rank_planes(labels, plane, dt, table, pair)
    left = []  # what goes pair by pair: single pairs, and what coloc_pairs declines
    for (red_z, thr, scale_max), pairs in p.batches.items():
        plane, dt = cache.get(red_z)
        if len(pairs) < 2 or not eng.coloc_pairs(labels, plane, dt, pairs, table, out, thr=thr, scale_max=scale_max):
            left.extend((pair, plane, dt, cols, thr, scale_max) for pair, cols in pairs)
    if left:
        fan.fork()
        for (ch0, ch1), plane, dt, cols, thr, scale_max in left:
            with fan.next_stream():
                eng.coloc(labels, plane, dt, ch0, ch1, table, out, cols, thr=thr, scale_max=scale_max)
        fan.join()


def _inputs(step, cache):  # -> (pixels, dtype code, channel) that the step's launcher is handed
    ch, red_z = step.inst[0], step.inst[1]
    if ch == "None" or not step.family.needs_pixels:
        if ch != "None" and cache is not None:
            cache.get(red_z)  # the reference would still reduce (and raise on a bad reducer)
        return None, 0, None
    if cache is None:
        raise Exception("pixels are required for this instruction")
    return (cache.tensor, cache.dtype, ch) if step.family.stack else (*cache.get(red_z), ch)


def _run_mono(eng, labels, table, cache, out, fan, p):
    # shared inputs first, on the main stream (the pixel-independent ones are cached on the object table)
    for s in p.steps:
        ch, red_z, metric = s.inst[0], s.inst[1], s.inst[-1]
        if ch != "None" and s.family.needs_pixels and cache is not None and red_z in _RED:
            cache.get(red_z)
        if metric in ("zernike", "radial_zernikes") and table.n_obj:
            eng.mec(labels, table)
        if metric == "radial_distribution" and table.n_obj:
            eng.radial_geometry(labels, table, s.kw.get("bin_count", 4), None if s.kw.get("scaled", True) else s.kw.get("maximum_radius", 100))
    cells = _CellBlocks(eng, labels, table)
    group = table.n_obj > 0  # without objects the Zernike channels are not grouped: each launches on its own
    fan.fork()
    for s in p.steps:
        if s.family.after_join:
            continue
        plane, dt, ch = _inputs(s, cache)
        if s.role == LAUNCH or (s.role == GROUP and not group):
            with fan.next_stream():
                s.family.launch(eng, labels, table, plane, dt, ch, out, s.col0, s.kw, cells)
    if group:
        for red_z, members in p.zernike_groups.items():
            plane, dt = cache.get(red_z)
            with fan.next_stream():
                eng.radial_zernikes_multi(labels, plane, dt, [c for c, _ in members], table, out, [c0 for _, c0 in members])
    fan.join()
    for col0, src, ncols in p.copies:
        out[:, col0 : col0 + ncols] = out[:, src : src + ncols]
    for s in p.steps:
        if s.family.after_join:
            s.family.launch(eng, labels, table, *_inputs(s, cache), out, s.col0, s.kw, cells)


# ------------------------------------------------------------------------------------------------
# volume families: label-keyed measurements of Z-stacks kept as volumes (FeatureEngine.*3d)
# ------------------------------------------------------------------------------------------------
# A volume tree has depth 3 throughout: {channel | "None" | (c0, c1): {"None": [names]}}.  The reducer key is always "None", ALIBY's
# "do not reduce" (as under nuc_conv_3d): a volume family reads the un-reduced stack.  Pixel-free families go under "None", the
# per-channel ones under their channel, the colocalisation names under a channel pair.  A column is "<key>/None/<name>/<column>".
@dataclass(frozen=True)
class VolumeFamily:  # one registered volume family; FeatureEngine's method of the same name measures it
    names: Callable  # names(kw) -> the keys of its columns
    needs_pixels: bool = True


VOLUME = {
    "intensity3d": VolumeFamily(lambda kw: feat.intensity3d_names()),
    "intensity3d_detail": VolumeFamily(lambda kw: feat.intensity3d_detail_names(kw.get("edge_measurements", True))),
    "texture3d": VolumeFamily(lambda kw: feat.texture3d_names(kw.get("scale", 3), kw.get("gray_levels", 256))),
    "granularity3d": VolumeFamily(lambda kw: feat.granularity3d_names(kw.get("granular_spectrum_length", 16))),
    "sizeshape3d": VolumeFamily(lambda kw: feat.sizeshape3d_names(kw.get("surface_area", False)), needs_pixels=False),
    "neighbors3d": VolumeFamily(lambda kw: feat.neighbors3d_names(kw.get("distance")), needs_pixels=False),
    "projection3d": VolumeFamily(lambda kw: feat.projection3d_names(), needs_pixels=False),
}
# the channel-pair names: groups of them become FeatureEngine.coloc3d calls
VOLUME_PAIRS = {name: VolumeFamily(lambda kw, _n=name: list(feat.COLOC[_n])) for name in feat.COLOC}
# per-name keywords of cp_measure_kwargs that the volume methods implement
VOLUME_KWARGS = {
    "sizeshape3d": ("spacing", "surface_area"),
    "intensity3d_detail": ("edge_measurements",),
    "texture3d": ("scale", "gray_levels"),
    "granularity3d": ("subsample_size", "image_sample_size", "element_size", "granular_spectrum_length"),
    "neighbors3d": ("distance",),
    "manders_fold": ("thr",),
    "rwc": ("thr",),
    "costes": ("scale_max",),
}
COLOC3D_MAX_PAIRS = 64  # per FeatureEngine.coloc3d call


@dataclass(frozen=True)
class VolumeCall:
    """One engine call of a volume plan: getattr(eng, method)(volume[, pixels, target], counts, **kw, out=matrix, col0=col0);
    target = the channel, for coloc3d the list of channel pairs, None for a pixel-free family."""

    method: str
    target: object
    kw: dict
    col0: int
    ncols: int


@dataclass(frozen=True)
class VolumePlan:
    blocks: list  # per instruction (first column, names): the second return value of `evaluate_volume`
    n_cols: int
    calls: list   # in launch order: ascending col0


def _is_channel(c) -> bool:
    return isinstance(c, int) and not isinstance(c, bool) and c >= 0


def plan_volume(instructions, cp_measure_kwargs) -> VolumePlan:
    """What `evaluate_volume` will do for the instructions of a volume tree, and every refusal that depends on the names and keywords
    alone.  Pure: no engine, no tensor.  Channel-pair metrics are grouped into coloc3d calls: consecutive metrics of a pair ride
    together while their parameters agree (manders_fold's thr does not leak into rwc: metrics whose thresholds differ are separate
    calls), and consecutive pairs that list the same metrics with the same parameters share one call."""
    cp_measure_kwargs = cp_measure_kwargs or {}
    blocks, calls = [], []
    col = 0
    group = None  # the open coloc3d group of the current pair: dict(pair, metrics, thr, scale_max, col0)

    def close():
        nonlocal group
        if group is None:
            return
        kw = dict(metrics=tuple(group["metrics"]), thr=15.0 if group["thr"] is None else group["thr"],
                  scale_max=255.0 if group["scale_max"] is None else group["scale_max"])
        ncols = 2 * len(group["metrics"])
        last = calls[-1] if calls else None
        if (last is not None and last.method == "coloc3d" and last.kw == kw and last.col0 + last.ncols == group["col0"]
                and len(last.target) < COLOC3D_MAX_PAIRS and group["pair"] not in last.target):
            calls[-1] = replace(last, target=[*last.target, group["pair"]], ncols=last.ncols + ncols)
        else:
            calls.append(VolumeCall("coloc3d", [group["pair"]], kw, group["col0"], ncols))
        group = None

    for inst in instructions:
        if len(inst) != 3:
            raise ValueError(f"a volume tree has depth 3, {{channel | 'None' | (c0, c1): {{'None': [names]}}}}, got the path {inst!r}")
        key, reducer, name = inst
        if name not in VOLUME and name not in VOLUME_PAIRS:
            raise KeyError(name)
        if reducer != "None":
            raise ValueError(f"{name}: a volume family reads the un-reduced stack: the reducer key must be 'None', got {reducer!r}")
        kw = dict(cp_measure_kwargs.get(name, {}))
        unbuilt = sorted(set(kw) - set(VOLUME_KWARGS.get(name, ())))
        if unbuilt:
            raise NotImplementedError(f"cp_measure_kwargs[{name!r}]: {unbuilt} not built (built: {sorted(VOLUME_KWARGS.get(name, ()))})")
        if isinstance(key, tuple):
            if len(key) != 2 or not all(_is_channel(c) for c in key) or key[0] == key[1]:
                raise ValueError(f"{name}: a channel-pair key is two distinct channels (c0, c1), got {key!r}")
            if name not in VOLUME_PAIRS:
                raise ValueError(f"{name} measures one channel (or none): list it under a channel or 'None', not under the pair {key!r}")
            names = VOLUME_PAIRS[name].names(kw)
            thr = float(kw["thr"]) if "thr" in kw else (15.0 if name in ("manders_fold", "rwc") else None)
            scale_max = float(kw["scale_max"]) if "scale_max" in kw else (255.0 if name == "costes" else None)
            fits = (group is not None and group["pair"] == key and name not in group["metrics"]
                    and (thr is None or group["thr"] in (None, thr)) and (scale_max is None or group["scale_max"] in (None, scale_max)))
            if not fits:
                close()
                group = dict(pair=key, metrics=[], thr=None, scale_max=None, col0=col)
            group["metrics"].append(name)
            group["thr"] = group["thr"] if thr is None else thr
            group["scale_max"] = group["scale_max"] if scale_max is None else scale_max
        else:
            close()
            if name in VOLUME_PAIRS:
                raise ValueError(f"{name} measures a channel pair: list it under a key (c0, c1), not under {key!r}")
            fam = VOLUME[name]
            if key == "None" and not isinstance(key, int):
                if fam.needs_pixels:
                    raise ValueError(f"{name} needs the pixels of a channel: list it under a channel, not under 'None'")
                target = None
            elif _is_channel(key):
                if not fam.needs_pixels:
                    raise ValueError(f"{name} reads labels only: list it under 'None', not under channel {key!r}")
                target = key
            else:
                raise ValueError(f"{name}: a volume tree's key is a channel, 'None' or a channel pair, got {key!r}")
            names = fam.names(kw)
            calls.append(VolumeCall(name, target, kw, col, len(names)))
        blocks.append((col, names))
        col += len(names)
    close()
    return VolumePlan(blocks, col, calls)


def evaluate_volume(eng, volume, pixels, counts, instructions, cp_measure_kwargs):
    """Run every instruction of a volume tree over every object of volume labels uint16 [F,Z,Y,X] with counts [F] objects per stack
    (pixels [F,C,Z,Y,X] on the device, or None for a pixel-free tree); returns (matrix [sum counts, n_cols] on the device, blocks).
    One matrix; every call writes its block in place, one after the other on the main stream: several volume families borrow the
    context's scratch, so there is no fan-out to side streams."""
    p = plan_volume(instructions, cp_measure_kwargs)
    rows = sum(int(c) for c in counts)
    out = eng.new_output(rows, p.n_cols)
    for call in p.calls:
        method = getattr(eng, call.method)
        if call.target is None:
            method(volume, counts, **call.kw, out=out, col0=call.col0)
        else:
            if pixels is None:
                raise Exception(f"pixels are required for {call.method}")
            method(volume, pixels, call.target, counts, **call.kw, out=out, col0=call.col0)
    return out, p.blocks
