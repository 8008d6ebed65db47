"""
Segmenter-agnostic pipeline engine with the reference's observable behaviour.

What the reference's engine does (src/aliby/pipe_core.py): steps are initialised lazily by an injected
`init_step_fn` (54-92, 182-183), each timepoint wires `passed_data` / `passed_methods` (188-215), runs the
step (147-154), writes the outputs listed in "save" every `save_interval` (219-228), appends to
`state["data"]` (230), drops tile pixels at the end of the tp (238-242) and trims histories per "retain"
(245-249); `validate_pipeline` (254-365) rejects malformed dicts; `_run_pipeline_and_post_impl` (381-450)
writes `profiles/<name>.parquet` and skips positions already done; `get_profiles_from_state` (453-512)
pivots every extract step's output, adds metadata columns, concatenates per step prefix and joins.

This module keeps those behaviours (same state layout `{"tps", "data", "fn"}`, same messages, same files)
behind a small `Engine` class.  Remote Nahual steps and trackastra global steps are out of scope
 and raise.
"""

from __future__ import annotations

import logging
import threading
from functools import partial
from pathlib import Path
from typing import Callable

import numpy
import pyarrow as pa
import pyarrow.parquet

from aliby_amd.extraction.extract import (
    extract_tree,
    extract_tree_multi,
    format_extraction,
    process_tree_masks,
    process_tree_masks_overlap,
    process_tree_volumes,
)
from aliby_amd.io.write import dispatch_write_fn, write_profiles
from aliby_amd.tile.tiler import dispatch_image, dispatch_tiler

logger = logging.getLogger("aliby")
_META_KEYS = ("tp", "tile", "object", "label")


def configure_logging(file):
    """DEBUG file sink like the reference's loguru one (pipe_core.py:37-46), on stdlib logging."""
    from logging.handlers import RotatingFileHandler

    Path(file).parent.mkdir(parents=True, exist_ok=True)
    sink = RotatingFileHandler(file, maxBytes=10 * 1024 * 1024, backupCount=5)
    sink.setFormatter(logging.Formatter("%(asctime)s | %(levelname)-8s | %(name)s:%(funcName)s:%(lineno)d - %(message)s"))
    logger.handlers = [sink]
    logger.setLevel(logging.DEBUG)


# ------------------------------------------------------------------------------------------------
# step initialisers shared by the pipelines' init_step dispatchers
# ------------------------------------------------------------------------------------------------
def _need(parameters: dict, key: str, step_name: str):
    if key not in parameters:
        raise ValueError(f"Step '{step_name}' is missing required '{key}'.")
    return parameters[key]


def _init_tile(step_name: str, parameters: dict) -> Callable:
    image_kwargs = parameters.pop("image_kwargs", None)
    if image_kwargs is None:
        raise ValueError(f"Step '{step_name}' is missing required 'image_kwargs'.")
    if "source" not in image_kwargs:
        raise ValueError(f"Step '{step_name}' 'image_kwargs' is missing required 'source'.")
    make_tiler = dispatch_tiler(parameters.pop("kind", None), parameters)
    return make_tiler(dispatch_image(source=image_kwargs["source"])(**image_kwargs))


def _init_extract(step_name: str, parameters: dict, *, overlap: bool) -> Callable:
    tree = _need(parameters, "tree", step_name)
    extra = parameters.get("kwargs", {})
    if overlap:
        return partial(process_tree_masks_overlap, measure_fn=partial(extract_tree, overlap=True), tree=tree, **extra)
    return partial(process_tree_masks, measure_fn=extract_tree, tree=tree, **extra)


def _init_extract_multi(step_name: str, parameters: dict) -> Callable:
    tree = _need(parameters, "tree", step_name)
    return partial(process_tree_masks, measure_fn=extract_tree_multi, tree=tree, **parameters.get("kwargs", {}))


_VOLUME_SOURCES = ("segment", "volumetertiary_", "volumesecondary_")  # the steps that keep volume labels in `last_volume`


def _kept_volume(step_name: str, key: str, source: str, other_steps: dict):
    """(volume uint16 [F,Z,Y,X] on the device, counts [F]) that the step `source` kept at this timepoint, or a ValueError that names
    the step `step_name`, its parameter `key` and the cause."""
    producer = other_steps.get(source)
    if producer is None or not hasattr(producer, "last_volume"):
        raise ValueError(f"Step '{step_name}': '{key}' = '{source}' is not a segment step or a volumetertiary step that ran before this one.")
    if producer.last_volume is None:
        raise ValueError(f"Step '{step_name}': '{source}' kept no volume labels: it ran without do_3D (set 'do_3D': True in its "
                         "segmenter_kwargs), or the stack has a single plane.")
    return producer.last_volume


def _volume_source(step_name: str, parameters: dict, key: str) -> str:
    source = _need(parameters, key, step_name)
    if not isinstance(source, str) or not source.startswith(_VOLUME_SOURCES):
        raise ValueError(f"Step '{step_name}': '{key}' must name a segment step (or a volumetertiary step), got {source!r}.")
    return source


def _init_volume(step_name: str, parameters: dict, other_steps: dict) -> Callable:
    """A `volume_<obj>` step: the volume families of `tree` (extraction.families.VOLUME / VOLUME_PAIRS) over the volume labels the
    segment step named by `volume_from` kept on the device (`segment.last_volume`, a 3-D segmentation: `do_3D` in its
    segmenter_kwargs) — or a `volumetertiary_` step (its tertiary volume) — with the tile's pixels.  `kwargs`: cp_measure_kwargs,
    ncores.  Its rows are keyed by the VOLUME label and go to their own table (get_volume_profiles_from_state), never into the join
    of the extract steps."""
    from aliby_amd.extraction import families
    from aliby_amd.extraction.extract import flatten, kv

    tree = _need(parameters, "tree", step_name)
    source = _volume_source(step_name, parameters, "volume_from")
    extra = dict(parameters.get("kwargs", {}))
    families.plan_volume(kv(flatten(tree)), extra.get("cp_measure_kwargs"))  # a tree or keyword that is refused fails here, not at tp 0

    def volume_step(pixels):
        volume, counts = _kept_volume(step_name, "volume_from", source, other_steps)
        shape = tuple(pixels.shape)
        if len(shape) != 5 or tuple(volume.shape) != (shape[0], *shape[2:]):
            raise ValueError(f"Step '{step_name}': the volume labels of '{source}' are {tuple(volume.shape)} [F,Z,Y,X], the pixels "
                             f"{shape} [F,C,Z,Y,X]: they do not match.")
        return process_tree_volumes(tree, volume, pixels, counts=counts, **extra)

    return volume_step


class _VolumeTertiary:
    """A `volumetertiary_<name>` step: the tertiary volume (FeatureEngine.tertiary_volume: the `outer` step's kept volume labels minus
    the objects of the `inner` step's, plane by plane; the cytoplasm of a stack) of two segment steps named in its parameters.  It
    keeps `last_volume` = (the tertiary volume on the device, outer's counts) for the `volume_<name>` and `volumerelate_` steps after
    it, and returns the labels on the host, one [Z,Y,X] uint16 array or a list of them for several tiles: listed under `save` they
    are written like a segment step's masks."""

    def __init__(self, step_name: str, parameters: dict, other_steps: dict):
        unknown = set(parameters) - {"outer", "inner", "shrink_inner"}
        if unknown:
            raise ValueError(f"Step '{step_name}': unknown parameters {sorted(unknown)}.")
        self.step_name, self.other_steps = step_name, other_steps
        self.outer, self.inner = _volume_source(step_name, parameters, "outer"), _volume_source(step_name, parameters, "inner")
        if self.outer == self.inner:
            raise ValueError(f"Step '{step_name}': 'outer' and 'inner' must name two different steps, got {self.outer!r} twice.")
        self.shrink = parameters.get("shrink_inner", True)
        if not isinstance(self.shrink, bool):
            raise ValueError(f"Step '{step_name}': 'shrink_inner' must be a bool, got {self.shrink!r}.")
        self.last_volume = None

    def __call__(self):
        from aliby_amd.extraction.engine import FeatureEngine

        self.last_volume = None
        outer, counts = _kept_volume(self.step_name, "outer", self.outer, self.other_steps)
        inner, _ = _kept_volume(self.step_name, "inner", self.inner, self.other_steps)
        if tuple(outer.shape) != tuple(inner.shape):
            raise ValueError(f"Step '{self.step_name}': the volume labels of '{self.outer}' are {tuple(outer.shape)} [F,Z,Y,X], those of "
                             f"'{self.inner}' {tuple(inner.shape)}: they do not match.")
        volume = FeatureEngine().tertiary_volume(outer, inner, shrink_inner=self.shrink)
        self.last_volume = (volume, counts)
        host = volume.cpu().numpy()
        return host[0] if host.shape[0] == 1 else [host[f] for f in range(host.shape[0])]


class _VolumeSecondary:
    """A `volumesecondary_<name>` step: the kept volume labels of the `primary` step grown by `distance` on the integer lattice
    `spacing` = (sz, sy, sx), default (1, 1, 1) (FeatureEngine.secondary_volume: CellProfiler's IdentifySecondaryObjects, method
    "Distance - N", on a stack; the cell around a nucleus).  It keeps `last_volume` = (the grown volume on the device, the primary's
    counts) — the numbering is kept and no object can vanish — for the `volume_<name>`, `volumetertiary_` and `volumerelate_` steps
    after it, and returns the labels on the host in `_VolumeTertiary`'s container: listed under `save` they are written like a
    segment step's masks."""

    def __init__(self, step_name: str, parameters: dict, other_steps: dict):
        from aliby_amd.extraction.features import secondary_volume_args

        unknown = set(parameters) - {"primary", "distance", "spacing"}
        if unknown:
            raise ValueError(f"Step '{step_name}': unknown parameters {sorted(unknown)}.")
        self.step_name, self.other_steps = step_name, other_steps
        self.primary = _volume_source(step_name, parameters, "primary")
        try:
            self.distance, self.spacing = secondary_volume_args(_need(parameters, "distance", step_name), parameters.get("spacing", (1, 1, 1)))
        except ValueError as e:
            raise ValueError(str(e) if str(e).startswith("Step ") else f"Step '{step_name}': {e}") from None
        self.last_volume = None

    def __call__(self):
        from aliby_amd.extraction.engine import FeatureEngine

        self.last_volume = None
        primary, counts = _kept_volume(self.step_name, "primary", self.primary, self.other_steps)
        volume = FeatureEngine().secondary_volume(primary, self.distance, self.spacing)
        self.last_volume = (volume, counts)
        host = volume.cpu().numpy()
        return host[0] if host.shape[0] == 1 else [host[f] for f in range(host.shape[0])]


def _volume_relate_others(step_name: str, parameters: dict) -> dict:
    """The `others` of a `volumerelate_<obj>` step: a non-empty {object-set name: the step that keeps its volume labels}."""
    from aliby_amd.extraction import features

    others = _need(parameters, "others", step_name)
    if not isinstance(others, dict) or not others:
        raise ValueError(f"Step '{step_name}': 'others' must be a non-empty dict {{object set: its segment or volumetertiary step}}, "
                         f"got {others!r}.")
    for other, source in others.items():
        features.relate3d_names(other)  # (refuses what cannot be told apart in a column or step name)
        _volume_source(step_name, {"others": source}, "others")
    return dict(others)


def _init_volume_relate(step_name: str, parameters: dict, other_steps: dict) -> Callable:
    """A `volumerelate_<obj>` step: the rows of <obj>'s volume objects relative to every object set of `others` (the `relate` family
    on volume labels; extraction.extract.relate_volumes), from the volumes the named steps kept.  `spacing` = (dz, dy, dx), default
    (1, 1, 1).  It returns (tileid_instructions, results) with the one instruction None/None/relate3d; the volume profile table joins
    the rows onto <obj>'s `volume_` rows."""
    from aliby_amd.extraction.engine import FeatureEngine
    from aliby_amd.extraction.extract import relate_volumes

    unknown = set(parameters) - {"volume_from", "others", "spacing"}
    if unknown:
        raise ValueError(f"Step '{step_name}': unknown parameters {sorted(unknown)}.")
    source = _volume_source(step_name, parameters, "volume_from")
    others = _volume_relate_others(step_name, parameters)
    try:
        spacing = tuple(float(v) for v in FeatureEngine._spacing3d(parameters.get("spacing", (1.0, 1.0, 1.0))))
    except (TypeError, ValueError) as e:
        raise ValueError(f"Step '{step_name}': {e}") from None

    def volume_relate_step():
        volume, counts = _kept_volume(step_name, "volume_from", source, other_steps)
        kept = {}
        for other, other_source in others.items():
            kept[other] = _kept_volume(step_name, "others", other_source, other_steps)
            if tuple(kept[other][0].shape) != tuple(volume.shape):
                raise ValueError(f"Step '{step_name}': the volume labels of '{source}' are {tuple(volume.shape)} [F,Z,Y,X], those of "
                                 f"'{other_source}' {tuple(kept[other][0].shape)}: they do not match.")
        return relate_volumes(volume, counts, kept, spacing=spacing)

    return volume_relate_step


def _relate_others(step_name: str, parameters: dict) -> list:
    """The `others` of an `extractrelate_<obj>` step: a non-empty sequence of distinct object-set names that make column names."""
    from aliby_amd.extraction import features

    others = _need(parameters, "others", step_name)
    if isinstance(others, str) or not isinstance(others, (list, tuple)) or not others or len(set(others)) != len(others):
        raise ValueError(f"Step '{step_name}': 'others' must be a non-empty sequence of distinct object-set names, got {others!r}.")
    for other in others:
        features.relate_names(other)  # (refuses what cannot be told apart in a column or step name)
    return list(others)


def _init_relate(step_name: str, parameters: dict) -> Callable:
    """An `extractrelate_<obj>` step: the rows of <obj>'s objects relative to every object set of `others` (CellProfiler's
    RelateObjects; extraction.extract.relate_masks).  Inputs: `masks` = <obj>'s segment result, `masks_<other>` = the other set's,
    through aliased `passed_data` entries.  It returns (tileid_instructions, results) with the one instruction None/None/relate; the
    profile table joins the rows onto <obj>'s extract rows."""
    from aliby_amd.extraction.extract import relate_masks

    others = _relate_others(step_name, parameters)  # (`kwargs`: the extract steps' ncores / cp_measure_kwargs; nothing here reads them)

    def relate_step(masks=None, **inputs):
        missing = [f"masks_{o}" for o in others if inputs.get(f"masks_{o}") is None]
        if masks is None or missing:
            raise ValueError(f"Step '{step_name}': no input for {['masks'] * (masks is None) + missing}: 'passed_data' must hand it "
                             "'masks' and one aliased 'masks_<other>' per entry of 'others', from steps that ran before it.")
        return relate_masks(masks, {o: inputs[f"masks_{o}"] for o in others}, who=f"Step '{step_name}'")

    return relate_step


def _init_tertiary(step_name: str, parameters: dict) -> Callable:
    """A `tertiary_<name>` step: the labels of the `outer` object set minus the objects of the `inner` one (CellProfiler's
    IdentifyTertiaryObjects: the cytoplasm; extraction.extract.tertiary_masks), in the container the outer segment step returned, so
    that `extract_<name>` / `extractmulti_<name>` steps measure it like a segment step's labels.  `shrink_inner` (default True)
    leaves the inner objects' outlines in."""
    from aliby_amd.extraction.extract import tertiary_masks

    unknown = set(parameters) - {"shrink_inner"}
    if unknown:
        raise ValueError(f"Step '{step_name}': unknown parameters {sorted(unknown)}.")
    shrink = parameters.get("shrink_inner", True)
    if not isinstance(shrink, bool):
        raise ValueError(f"Step '{step_name}': 'shrink_inner' must be a bool, got {shrink!r}.")

    def tertiary_step(outer=None, inner=None):
        if outer is None or inner is None:
            raise ValueError(f"Step '{step_name}': no input for {['outer'] * (outer is None) + ['inner'] * (inner is None)}: "
                             "'passed_data' must hand it the masks of two segment steps under the aliases 'outer' and 'inner'.")
        return tertiary_masks(outer, inner, shrink_inner=shrink, who=f"Step '{step_name}'")

    return tertiary_step


def _init_secondary(step_name: str, parameters: dict) -> Callable:
    """A `secondary_<name>` step: the labels of the `primary` object set grown by `distance` pixels (CellProfiler's
    IdentifySecondaryObjects, method "Distance - N": the cell around a nucleus; extraction.extract.secondary_masks), in the container
    the primary segment step returned, so that `extract_<name>` / `extractmulti_<name>` steps measure it like a segment step's labels
    and a `tertiary_` step may take it as its outer set.  `distance` is required: an integer in 1..64."""
    from aliby_amd.extraction.extract import secondary_masks
    from aliby_amd.extraction.features import secondary_distance

    unknown = set(parameters) - {"distance"}
    if unknown:
        raise ValueError(f"Step '{step_name}': unknown parameters {sorted(unknown)}.")
    if "distance" not in parameters:
        raise ValueError(f"Step '{step_name}' is missing required 'distance'.")
    try:
        distance = secondary_distance(parameters["distance"])
    except ValueError as e:
        raise ValueError(f"Step '{step_name}': {e}") from None

    def secondary_step(primary=None):
        if primary is None:
            raise ValueError(f"Step '{step_name}': no input for ['primary']: 'passed_data' must hand it the masks of a segment step "
                             "under the alias 'primary'.")
        return secondary_masks(primary, distance, who=f"Step '{step_name}'")

    return secondary_step


def _init_propagate(step_name: str, parameters: dict) -> Callable:
    """A `propagate_<name>` step: the labels of the `primary` object set grown along the stain in channel `channel` of the tile step's
    pixels, max-projected over Z (CellProfiler's IdentifySecondaryObjects, method "Propagation": the cell around a nucleus where the
    cell stain says it ends; extraction.extract.propagate_masks), in the container the primary segment step returned, so that
    `extract_<name>` / `extractmulti_<name>` steps measure it like a segment step's labels and a `tertiary_` step may take it as its
    outer set.  `channel` is required: a non-negative integer.  Optional: `threshold`, `regularization`, `distance`, `image_max`
    (features.propagate_args; a `distance` alone is "Distance - B"), and `auto_threshold`, an option dict of
    features.auto_threshold_args ("method", "classes", "middle", "correction", "bounds"; {} is two-class Otsu) in place of
    `threshold`: every tile is thresholded at its own Otsu level, computed on the device.  The callable keeps the last call's
    thresholds, one Python int per tile, in its attribute `thresholds`."""
    from aliby_amd.extraction.extract import propagate_masks
    from aliby_amd.extraction.features import PROPAGATE_OPTIONS, auto_threshold_options, propagate_args, propagate_channel

    unknown = set(parameters) - {"channel", "auto_threshold", *PROPAGATE_OPTIONS}
    if unknown:
        raise ValueError(f"Step '{step_name}': unknown parameters {sorted(unknown)}.")
    if "channel" not in parameters:
        raise ValueError(f"Step '{step_name}' is missing required 'channel'.")
    try:
        channel = propagate_channel(parameters["channel"])
        checked = propagate_args(**{key: parameters[key] for key in PROPAGATE_OPTIONS if key in parameters}).options()
        if "auto_threshold" in parameters:
            checked["auto_threshold"] = auto_threshold_options(parameters["auto_threshold"]).options()
            if checked["threshold"] != 0:
                raise ValueError(f"propagate: give threshold or auto_threshold, not both (threshold={parameters['threshold']!r})")
    except ValueError as e:
        raise ValueError(f"Step '{step_name}': {e}") from None

    def propagate_step(primary=None, pixels=None):
        missing = [key for key, value in (("primary", primary), ("pixels", pixels)) if value is None]
        if missing:
            raise ValueError(f"Step '{step_name}': no input for {missing}: 'passed_data' must hand it the masks of a segment step under "
                             "the alias 'primary' and the pixels of the tile step.")
        return propagate_masks(primary, pixels, channel, **checked, who=f"Step '{step_name}'", chosen=propagate_step.thresholds)

    propagate_step.thresholds = []  # the last call's threshold of every tile
    return propagate_step


def _check_volume_links(steps: dict) -> None:
    """The wiring of the volume steps that read another step's kept volume, before any timepoint: a `volumetertiary_`,
    `volumesecondary_` or `volumerelate_` step, and a `volume_` step fed by a `volumetertiary_` or `volumesecondary_` one, names steps
    of the pipeline that run before it and keep volume labels."""
    order = {name: k for k, name in enumerate(steps)}
    for name, params in steps.items():
        if not isinstance(params, dict):
            continue
        if name.startswith("volumetertiary_"):
            wanted = {"outer": params.get("outer"), "inner": params.get("inner")}
        elif name.startswith("volumesecondary_"):
            wanted = {"primary": params.get("primary")}
        elif name.startswith("volumerelate_"):
            wanted = {"volume_from": params.get("volume_from")}
            wanted.update({f"others[{o!r}]": src for o, src in _volume_relate_others(name, params).items()})
        elif name.startswith("volume_") and isinstance(params.get("volume_from"), str) and params["volume_from"].startswith(
                ("volumetertiary_", "volumesecondary_")):
            wanted = {"volume_from": params["volume_from"]}
        else:
            continue
        for key, source in wanted.items():
            if not isinstance(source, str) or not source.startswith(_VOLUME_SOURCES):
                raise ValueError(f"Step '{name}': '{key}' must name a segment step (or a volumetertiary step), got {source!r}.")
            if source not in steps or order[source] >= order[name]:
                raise ValueError(f"Step '{name}': '{key}' = '{source}' is not a step of the pipeline that runs before it.")
            kwargs = steps[source].get("segmenter_kwargs", {}) if isinstance(steps[source], dict) else {}
            if source.startswith("segment") and not (isinstance(kwargs, dict) and kwargs.get("do_3D")):
                raise ValueError(f"Step '{name}': '{key}' = '{source}' keeps no volume labels: set 'do_3D': True in its segmenter_kwargs.")


def _check_object_links(steps: dict, passed_data: dict) -> None:
    """The wiring of the two-object-set steps, before any timepoint: every input they need is an aliased `passed_data` entry."""
    _check_volume_links(steps)
    for name, params in steps.items():
        if name.startswith("extractrelate_") and isinstance(params, dict):
            wanted = ["masks"] + [f"masks_{o}" for o in _relate_others(name, params)]
        elif name.startswith("tertiary_"):
            wanted = ["outer", "inner"]
        elif name.startswith("secondary_"):
            wanted = ["primary"]
        elif name.startswith("propagate_"):
            wanted = ["primary", "pixels"]
        else:
            continue
        have = {dep[2] if len(dep) > 2 else dep[0] for dep in passed_data.get(name, ())}
        missing = [w for w in wanted if w not in have]
        if missing:
            raise ValueError(f"Step '{name}' needs the inputs {missing} in 'passed_data' (entries ('masks', <segment step>, <alias>)).")


def _init_nahual(step_name: str, parameters: dict) -> Callable:
    if parameters.get("address") is None:
        raise ValueError(f"If using Nahual you must have an address, currently it is None in step '{step_name}'")
    raise NotImplementedError(f"'{step_name}': Nahual remote steps are out of scope (SURVEY §2 rows 6/16)")


def run_step(step, *args, **kwargs):
    """Objects with `run_tp` get the time point; plain callables do not (pipe_core.py:147-154)."""
    runner = getattr(step, "run_tp", None)
    if runner is not None:
        return runner(*args, **kwargs)
    kwargs.pop("tp", None)
    return step(*args, **kwargs)


# ------------------------------------------------------------------------------------------------
# validation
# ------------------------------------------------------------------------------------------------
def _is_count(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def _check_links(pipeline: dict, steps: dict) -> dict:
    passed_data = pipeline.get("passed_data")
    if not isinstance(passed_data, dict):
        raise ValueError("Pipeline must contain a 'passed_data' dictionary.")
    for consumer, deps in passed_data.items():
        if not isinstance(deps, (list, tuple)):
            raise TypeError(f"'passed_data' dependencies for step '{consumer}' must be a sequence.")
        for dep in deps:
            if not isinstance(dep, (list, tuple)) or len(dep) < 2:
                raise ValueError(f"Invalid dependency format in 'passed_data' for '{consumer}': {dep}")
            if dep[1] not in steps:
                raise ValueError(f"Step '{consumer}' expects data from '{dep[1]}', but '{dep[1]}' is not defined in 'steps'.")
    methods = pipeline.get("passed_methods", {})
    if not isinstance(methods, dict):
        raise TypeError("'passed_methods' must be a dictionary.")
    for consumer, dep in methods.items():
        if not isinstance(dep, (list, tuple)) or len(dep) < 2:
            raise ValueError(f"Invalid method dependency format for '{consumer}': {dep}")
        if dep[0] not in steps:
            raise ValueError(f"Step '{consumer}' expects a method from '{dep[0]}', but '{dep[0]}' is not defined in 'steps'.")
    return passed_data


def _check_outputs(pipeline: dict, steps: dict, passed_data: dict) -> None:
    save = pipeline.get("save")
    if save is not None:
        if not isinstance(save, (list, tuple, set)):
            raise TypeError("'save' must be a sequence of step names.")
        known = set(steps) | set(pipeline.get("global_steps", {}))
        for name in save:
            if name not in known:
                raise ValueError(f"Step '{name}' listed in 'save' is not defined in the pipeline 'steps' or 'global_steps'.")
    if "save_interval" in pipeline and not (_is_count(pipeline["save_interval"]) and pipeline["save_interval"] >= 1):
        raise ValueError(f"'save_interval' must be a positive int, got {pipeline['save_interval']!r}.")
    retain = pipeline.get("retain", {})
    if not isinstance(retain, dict):
        raise TypeError("'retain' must be a dictionary mapping step name to int or 'all'.")
    tracked = {dep[1] for consumer, deps in passed_data.items() if consumer.startswith("track") for dep in deps}
    for name, keep in retain.items():
        if name not in steps:
            raise ValueError(f"'retain' references step '{name}' not defined in 'steps'.")
        if keep != "all" and not (_is_count(keep) and keep >= 0):
            raise ValueError(f"'retain[{name}]' must be a non-negative int or 'all', got {keep!r}.")
        if name in tracked and isinstance(keep, int) and keep < 2:
            raise ValueError(
                f"'retain[{name}]' = {keep} is too small; per-tp 'track' step reads the last 2 timepoints of '{name}'."
            )


def validate_pipeline(pipeline: dict) -> None:
    if not isinstance(pipeline, dict):
        raise TypeError("Pipeline configuration must be a dictionary.")
    steps = pipeline.get("steps")
    if not isinstance(steps, dict):
        raise ValueError("Pipeline must contain a 'steps' dictionary mapping step names to parameters.")
    passed_data = _check_links(pipeline, steps)
    _check_outputs(pipeline, steps, passed_data)
    for name, params in steps.items():
        if not isinstance(params, dict):
            raise TypeError(f"Parameters for step '{name}' must be a dictionary.")
        if name.startswith("nahual") and "address" not in params:
            raise ValueError(f"Nahual-deployed step '{name}' must provide an 'address' parameter.")
    _check_object_links(steps, passed_data)
    if pipeline.get("global_steps"):
        if "global_passed_data" not in pipeline:
            raise ValueError("Pipeline defines 'global_steps' but is missing 'global_passed_data'.")
        if not isinstance(pipeline["global_passed_data"], dict):
            raise TypeError("'global_passed_data' must be a dictionary.")
        # well-formed but out of scope here (trackastra via Nahual): refused before any timepoint is
        # processed, on the first run and on a resume alike
        raise NotImplementedError("global steps (trackastra via Nahual) are out of scope (SURVEY §2 row 16)")


# ------------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------------
class Engine:
    """Runs a pipeline dict one timepoint at a time; `state` has the reference's layout."""

    def __init__(self, pipeline: dict, steps_dir, init_step_fn: Callable):
        self.pipeline, self.steps_dir, self.init_step_fn = pipeline, steps_dir, init_step_fn

    @staticmethod
    def fresh_state(steps: dict) -> dict:
        return {"tps": {name: 0 for name in steps}, "data": {}, "fn": {}}

    def _inputs_for(self, step_name: str, state: dict) -> dict:
        kwargs = {}
        for kwd, producer, *alias in self.pipeline["passed_data"].get(step_name, ()):
            history = state["data"].get(producer, [])
            if not len(history):
                continue
            if step_name == "track" and kwd == "masks":
                # the tracker reads the last two timepoints, regrouped per tile
                value = [[tp_tiles[i] for tp_tiles in history[-2:]] for i in range(len(history[-1]))]
            else:
                value = history[-1]
                if isinstance(value, dict):
                    value = value[kwd]
            kwargs[alias[0] if alias else kwd] = value
        return kwargs

    def _method_args(self, step_name: str, state: dict, tp: int) -> tuple:
        spec = self.pipeline.get("passed_methods", {}).get(step_name)
        if spec is None or not step_name.startswith("segment"):
            return ()
        owner, method = spec
        return (getattr(state["fn"][owner], method)(tp),)

    def _maybe_save(self, step_name: str, result, tp: int) -> None:
        wanted = self.pipeline.get("save") or []
        every = self.pipeline.get("save_interval", 1)
        if wanted and every > 0 and tp % every == 0 and step_name in wanted:
            print(f"Saving {step_name} to {self.steps_dir}")
            dispatch_write_fn(step_name)(result, steps_dir=self.steps_dir, subpath=step_name, tp=tp)

    def _end_of_timepoint(self, state: dict) -> None:
        for name, history in state["data"].items():
            if name.startswith("tile") and history and isinstance(history[-1], dict):
                history[-1].pop("pixels", None)  # pixels are only consumed inside their own tp
        for name, history in state["data"].items():
            keep = self.pipeline.get("retain", {}).get(name, "all")
            if isinstance(keep, int) and keep >= 0 and len(history) > keep:
                del history[: len(history) - keep]

    def step(self, state: dict | None) -> dict:
        steps = self.pipeline["steps"]
        if not state:
            state = self.fresh_state(steps)
        tp = next(iter(state["tps"].values()))
        for name, parameters in steps.items():
            state["data"].setdefault(name, [])
            if name not in state["fn"]:
                state["fn"][name] = self.init_step_fn(name, parameters, state["fn"])
            result = run_step(state["fn"][name], *self._method_args(name, state, tp), tp=tp, **self._inputs_for(name, state))
            self._maybe_save(name, result, tp)
            state["data"][name].append(result)
            state["tps"][name] = tp + 1
        self._end_of_timepoint(state)
        return state


def pipeline_step(pipeline: dict, state: dict | None, steps_dir, init_step_fn: Callable) -> dict:
    """One timepoint (function form kept for callers of the reference's API)."""
    return Engine(pipeline, steps_dir, init_step_fn).step(state)


def run_pipeline_return_state(pipeline: dict, steps_dir, init_step_fn: Callable) -> dict:
    validate_pipeline(pipeline)
    engine, state = Engine(pipeline, steps_dir, init_step_fn), {}
    for _ in range(pipeline.get("ntps", 1)):
        state = engine.step(state)
    return state


# Pipelines of one process run one at a time on the device: a segmenter's model (weights, workspaces) is shared by every caller
# with the same parameters (segment/dispatch.py), and so are the dynamics' workspace and the runner's arenas.  Re-entrant: the
# position-batched runner holds it for a whole run_positions call and runs fallback steps under it.
DEVICE_LOCK = threading.RLock()


def _run_pipeline_and_post_impl(pipeline: dict, pipeline_name: str, output_path, overwrite: bool = True, *,
                                init_step_fn: Callable, post_state_hook: Callable | None = None):
    """One position: `profiles/<name>.parquet` (zstd), `steps/<name>/...`; an existing parquet is skipped
    unless `overwrite` (resume-by-skip).  A pipeline with a `volume_` step also gets `profiles3d/<name>.parquet`, returned as
    `(profiles, {"profiles3d": table})`; without one the files and the return value `(profiles, {})` are the reference's."""
    output_path = Path(output_path)
    profiles_file = output_path / "profiles" / f"{pipeline_name}.parquet"
    validate_pipeline(pipeline)  # before the resume check: a bad / out-of-scope dict fails the same way on every run
    if not overwrite and profiles_file.exists():
        logger.info(f"Skipping {pipeline_name}")
        return None, None
    # While the call runs, what the process allocated before it is out of the cycle collector's sight: a position allocates
    # enough (18 k (object, instruction) pairs for 256 nuclei) to trigger full collections, and a full collection over a heap with
    # torch, pyarrow and the caller's data in it is ~100 ms against the ~18 ms a position takes.  (Nothing is disabled: the
    # collector keeps running over what the call itself allocates.  ALIBY_MANAGE_GC=0: hands off.)
    import gc
    import os

    frozen = gc.isenabled() and gc.get_freeze_count() == 0 and os.environ.get("ALIBY_MANAGE_GC", "1") != "0"
    if frozen:
        gc.freeze()
    try:
        with DEVICE_LOCK:  # (one pipeline at a time per process: callers on several threads share the GPU and the segmenters' models)
            state = run_pipeline_return_state(pipeline, output_path / "steps" / pipeline_name, init_step_fn)
        profiles = get_profiles_from_state(state, pipeline)
        profiles_file.parent.mkdir(parents=True, exist_ok=True)
        write_profiles(profiles, profiles_file)
        extras = {}
        if any(name.startswith("volume_") for name in pipeline["steps"]):
            # the true 3-D rows, beside the reference-faithful ones of the collapse: they join on (metadata_tp, metadata_tile,
            # metadata_object, Projection_Label = metadata_label)
            extras["profiles3d"] = get_volume_profiles_from_state(state, pipeline)
            volume_file = output_path / "profiles3d" / f"{pipeline_name}.parquet"
            volume_file.parent.mkdir(parents=True, exist_ok=True)
            write_profiles(extras["profiles3d"], volume_file)
        if post_state_hook is not None:
            post_state_hook(state, pipeline, output_path, pipeline_name)
        return profiles, extras
    finally:
        if frozen:
            gc.unfreeze()


# ------------------------------------------------------------------------------------------------
# profile table
# ------------------------------------------------------------------------------------------------
def _empty_profiles() -> pa.Table:
    fields = [("metadata_tile", pa.int64()), ("metadata_label", pa.int64()), ("metadata_object", pa.string()),
              ("metadata_tp", pa.int64())]
    return pa.Table.from_pylist([], schema=pa.schema([pa.field(n, t) for n, t in fields]))


def _wide_table(step_name: str, tp: int, output) -> pa.Table | None:
    if isinstance(output, numpy.ndarray):  # arbitrary embedders: one (instructions, metrics) pair
        output = ((("__", "__"),), (output,))
    table = format_extraction(output)
    table = table.rename_columns([{"tile": "metadata_tile", "label": "metadata_label"}.get(c, c) for c in table.column_names])
    if not len(table):
        return None
    table = table.append_column("metadata_object", pa.array([step_name.split("_")[-1]] * len(table), pa.string()))
    return table.append_column("metadata_tp", pa.array([tp] * len(table), pa.uint16()))


def get_profiles_from_state(state: dict, pipeline: dict) -> pa.Table:
    """Pivot every (extract step, tp), concatenate per step prefix ("extract", "extractmulti", ...) and
    join the prefixes on the metadata columns."""
    by_prefix: dict[str, list] = {}
    for name in pipeline["steps"]:
        if not (name.startswith("extract") or name.startswith("nahual_embed")):
            continue
        bucket = by_prefix.setdefault(name.split("_")[0], [])
        for tp, output in enumerate(state["data"][name]):
            table = _wide_table(name, tp, output)
            if table is not None:
                bucket.append(table)
    # the `extractrelate` steps of different object sets carry different columns (Parent_cell on nuclei rows, Parent_nuclei on cell
    # rows): that prefix alone is concatenated with its schemas unified, null-filled, and joined after the others
    related = by_prefix.pop(_RELATE_PREFIX, None)
    merged = [pa.concat_tables(tables) for tables in by_prefix.values() if tables]
    if not merged and not related:
        return _empty_profiles()
    if related:
        merged.append(pa.concat_tables(related, promote_options="default"))
    profiles = merged[0]
    for k, other in enumerate(merged[1:], 1):
        profiles = _join_related(profiles, other) if related and k == len(merged) - 1 else _join_on_metadata(profiles, other)
    return profiles


_RELATE_PREFIX = "extractrelate"


def _join_related(left: pa.Table, right: pa.Table) -> pa.Table:
    """The `extractrelate` rows onto the rows of the extract steps: a left join on the metadata columns that keeps the left table's
    row order (rows without a relation — a tertiary compartment's — get nulls)."""
    joined = _join_on_metadata(left, right, strict=True)
    if joined is not None:
        return joined
    order = "__row__"
    numbered = left.append_column(order, pa.array(numpy.arange(left.num_rows, dtype=numpy.int64)))
    return numbered.join(right, keys=[f"metadata_{k}" for k in _META_KEYS]).sort_by(order).drop_columns([order])


def get_volume_profiles_from_state(state: dict, pipeline: dict) -> pa.Table:
    """One wide table per (`volume_` step, tp), concatenated: the metadata columns of `get_profiles_from_state`, with
    `metadata_label` the VOLUME label.  Kept apart from the extract steps' table, whose labels are those of the collapsed image;
    `<key>/None/projection3d/Projection_Label` is the row's label there (0: hidden in the collapse).  The rows of `volumerelate_`
    steps carry different columns per object set (Parent_cell on nuclei rows, Parent_nuclei on cell rows): they are concatenated with
    their schemas unified, null-filled, and left-joined onto the `volume_` rows on the metadata columns, keeping the row order (the
    arrangement of `_join_related`).  A tertiary compartment's rows carry its own name as metadata_object and the outer object's
    volume label: cytoplasm rows join their cell on (metadata_tp, metadata_tile, metadata_label).  Without such steps the table is
    the `volume_` rows alone."""
    tables, related = [], []
    for name in pipeline["steps"]:
        bucket = tables if name.startswith("volume_") else related if name.startswith(_VOLUME_RELATE_PREFIX) else None
        if bucket is None:
            continue
        for tp, output in enumerate(state["data"][name]):
            table = _wide_table(name, tp, output)
            if table is not None:
                bucket.append(table)
    if not tables:
        return _empty_profiles()
    profiles = pa.concat_tables(tables)
    return _join_related(profiles, pa.concat_tables(related, promote_options="default")) if related else profiles


_VOLUME_RELATE_PREFIX = "volumerelate_"


def _join_on_metadata(left: pa.Table, right: pa.Table, strict: bool = False) -> pa.Table:
    """`left.join(right, keys=metadata_*)` (pipe_core.py:499-510; pyarrow's default left outer join).  Both sides come from
    the same object table, so their key columns are normally equal row for row: the join is then the left table plus the
    right table's other columns, without building an Acero plan for a thousand-column table (tens of ms per position).
    Anything else goes through pyarrow's join."""
    keys = [f"metadata_{k}" for k in _META_KEYS]
    # (column lists taken once: `table[name]` and `table.column_names` cost a pass over a thousand fields each)
    lnames, rnames = left.column_names, right.column_names
    lcols, rcols = left.columns, right.columns
    lpos, rpos = {n: i for i, n in enumerate(lnames)}, {n: i for i, n in enumerate(rnames)}
    keyset = set(keys)
    if left.num_rows == right.num_rows and all(k in lpos and k in rpos for k in keys) and all(
            lcols[lpos[k]].equals(rcols[rpos[k]]) for k in keys) and not (set(lnames) & set(rnames)) - keyset:
        names = list(lnames)
        arrays = list(lcols)
        for name, col in zip(rnames, rcols):
            if name not in keyset:
                names.append(name)
                arrays.append(col)
        return pa.Table.from_arrays(arrays, names=names)
    if strict:  # the caller relies on the row order of the left table: no plan-ordered join
        return None
    return left.join(right, keys=keys)


# ------------------------------------------------------------------------------------------------
# reading step outputs back
# ------------------------------------------------------------------------------------------------
def get_step_output(state_data: dict, fetchers, steps_dir=None) -> numpy.ndarray:
    gathered = []
    for fetcher in fetchers:
        if callable(fetcher):
            gathered.append(fetcher(state_data))
        elif not isinstance(fetcher, str):
            raise Exception(f"Invalid type, expected Callable or string, got {type(fetcher)}")
        elif fetcher.startswith("from_disk:"):
            if steps_dir is None:
                raise ValueError("from_disk fetcher requires steps_dir; pass it through get_step_output(..., steps_dir=...)")
            gathered.append(_load_per_tp_masks(Path(steps_dir) / fetcher.removeprefix("from_disk:")))
        else:
            gathered.append([entry[0] for entry in state_data[fetcher]])  # monotile
    return numpy.asarray(gathered)


def _load_per_tp_masks(step_dir) -> list:
    """Per-tp `.npz` written by io.write.write_ndarray: `tile_i` keys (dict results) or a single `arr_0`."""
    files = sorted(Path(step_dir).glob("*.npz"))
    if not files:
        raise FileNotFoundError(f"No per-tp .npz files found under {step_dir}; ensure this step is listed in pipeline['save'].")
    masks = []
    for path in files:
        with numpy.load(path) as npz:
            keys = list(npz.keys())
            if "tile_0" in keys:
                masks.append(npz["tile_0"])
            elif keys == ["arr_0"]:
                masks.append(npz["arr_0"][0])
            else:
                raise ValueError(f"Unrecognised .npz layout in {path}: keys={keys}")
    return masks
