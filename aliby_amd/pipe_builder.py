"""
Pipeline-definition builder for the Cellpose + cp_measure pipeline.

API-identical to the reference's `build_pipeline_steps` (src/aliby/pipe_builder.py:46-167) and
`_create_extract_multich_tree` (19-43): same keyword arguments, same defaults, same resulting dict
(steps / passed_data / passed_methods / save / save_interval), so a pipeline dict built by either
can be run by `aliby_amd.pipe.run_pipeline_and_post`.
"""

from __future__ import annotations

from itertools import combinations
from typing import Sequence

DEFAULT_FEATURES = ("radial_zernikes", "intensity", "feret", "texture", "radial_distribution", "zernike")
COLOC_METRICS = ("pearson", "costes", "manders_fold", "rwc")


def _step_kwargs(extract_ncores, cp_measure_feature_kwargs):
    kwargs = {"ncores": extract_ncores}
    if cp_measure_feature_kwargs:
        kwargs["cp_measure_kwargs"] = dict(cp_measure_feature_kwargs)
    return kwargs


def _create_extract_multich_tree(channels, extract_ncores, cp_measure_feature_kwargs=None) -> dict:
    """{(c0,c1): {"None": {"max": [pearson, costes, manders_fold, rwc]}}} for every channel pair."""
    tree = {pair: {"None": {"max": list(COLOC_METRICS)}} for pair in combinations(channels, r=2)}
    return {"tree": tree, "kwargs": _step_kwargs(extract_ncores, cp_measure_feature_kwargs)}


def _secondary_sets(objects, secondary):
    """The `secondary` keyword of build_pipeline_steps, checked against the segmented object sets: {name: (primary, distance)}."""
    from aliby_amd.extraction.features import relate_names, secondary_distance

    if secondary is None:
        return {}
    if not isinstance(secondary, dict):
        raise ValueError(f"secondary must be a dict {{name: (primary, distance)}}, got {secondary!r}")
    checked = {}
    for name, entry in secondary.items():
        relate_names(name)  # (a name that a step name or a column name cannot carry)
        if name in objects:
            raise ValueError(f"secondary: '{name}' is already a segmented object set")
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"secondary['{name}'] must be (primary, distance), got {entry!r}")
        if entry[0] not in objects:
            raise ValueError(f"secondary['{name}']: the primary {entry[0]!r} is not a segmented object set of {objects}")
        try:
            checked[name] = (entry[0], secondary_distance(entry[1]))
        except ValueError as e:
            raise ValueError(f"secondary['{name}'] must be (primary, distance): {e}") from None
    return checked


def _volume_secondary_sets(secondary, volume_secondary, volume_features):
    """The `volume_secondary` keyword of build_pipeline_steps against the checked `secondary` sets: {name: (distance, (sz, sy, sx))}
    in the units of the integer lattice, {} for False.  True: unit spacing and the entry's N.  (p, q), two integers: a plane step is
    p/q pixels, so the lattice is (p, q, q) and the distance q N."""
    from aliby_amd.extraction.features import secondary_volume_args

    if volume_secondary is False:
        return {}
    if volume_secondary is True:
        p, q = 1, 1
    elif (isinstance(volume_secondary, (tuple, list)) and len(volume_secondary) == 2
          and all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in volume_secondary)):
        p, q = volume_secondary
    else:
        raise ValueError("volume_secondary must be False, True (unit spacing) or a pair of positive integers (p, q), a plane step of "
                         f"p/q pixels, got {volume_secondary!r}")
    if volume_features is None or not secondary:
        raise ValueError("volume_secondary needs volume_features (the volume labels come from 3-D segment steps) and at least one "
                         "secondary entry")
    grown = {}
    for name, (_, distance) in secondary.items():
        try:
            grown[name] = secondary_volume_args(q * distance, (p, q, q))
        except ValueError as e:
            raise ValueError(f"volume_secondary={volume_secondary!r}, secondary['{name}']: {e}") from None
    return grown


def _propagate_sets(objects, secondary, propagate):
    """The `propagate` keyword of build_pipeline_steps, checked against the segmented and the secondary object sets:
    {name: (primary, channel, {option: checked value})}."""
    from aliby_amd.extraction.features import PROPAGATE_OPTIONS, auto_threshold_options, propagate_args, propagate_channel, relate_names

    if propagate is None:
        return {}
    if not isinstance(propagate, dict):
        raise ValueError(f"propagate must be a dict {{name: (primary, channel)}} or {{name: (primary, channel, options)}}, got {propagate!r}")
    checked = {}
    for name, entry in propagate.items():
        relate_names(name)  # (a name that a step name or a column name cannot carry)
        if name in objects:
            raise ValueError(f"propagate: '{name}' is already a segmented object set")
        if name in secondary:
            raise ValueError(f"propagate: '{name}' is already a secondary object set")
        if not isinstance(entry, (tuple, list)) or len(entry) not in (2, 3):
            raise ValueError(f"propagate['{name}'] must be (primary, channel) or (primary, channel, options), got {entry!r}")
        primary, channel, options = (*entry, {})[:3]
        if primary not in objects:
            raise ValueError(f"propagate['{name}']: the primary {primary!r} is not a segmented object set of {objects}")
        allowed = (*PROPAGATE_OPTIONS, "auto_threshold")
        if not isinstance(options, dict) or set(options) - set(allowed):
            raise ValueError(f"propagate['{name}']: the options must be a dict with keys of {list(allowed)}, got {options!r}")
        try:
            values = propagate_args(**{key: value for key, value in options.items() if key != "auto_threshold"}).options()
            if "auto_threshold" in options:
                auto = options["auto_threshold"]
                values["auto_threshold"] = auto_threshold_options(auto).options(auto)  # (the keys given, checked)
                if values["threshold"] != 0:
                    raise ValueError(f"give threshold or auto_threshold, not both (threshold={options['threshold']!r})")
            checked[name] = (primary, propagate_channel(channel), {key: values[key] for key in options})  # (in the entry's order)
        except ValueError as e:
            raise ValueError(f"propagate['{name}']: {e}") from None
    return checked


def _object_links(objects, relate, tertiary, secondary=(), propagate=()):
    """The `relate` and `tertiary` keywords of build_pipeline_steps, checked against the object sets — the segmented ones and the
    names of `secondary` and `propagate`: ({obj: [partners]} in first-seen order, {name: (outer, inner)})."""
    from aliby_amd.extraction.features import relate_names

    objects = [*objects, *secondary, *propagate]
    tertiary = dict(tertiary or {})
    for name, pair in tertiary.items():
        relate_names(name)  # (a name that a step name or a column name cannot carry)
        if name in secondary:
            raise ValueError(f"tertiary: '{name}' is already a secondary object set")
        if name in propagate:
            raise ValueError(f"tertiary: '{name}' is already a propagated object set")
        if name in objects:
            raise ValueError(f"tertiary: '{name}' is already a segmented object set")
        if not isinstance(pair, (tuple, list)) or len(pair) != 2 or pair[0] == pair[1] or any(o not in objects for o in pair):
            raise ValueError(f"tertiary['{name}'] must be (outer, inner), two different object sets of {objects}, got {pair!r}")
    related: dict[str, list] = {}
    for pair in relate or ():
        if not isinstance(pair, (tuple, list)) or len(pair) != 2 or pair[0] == pair[1]:
            raise ValueError(f"relate: every entry is a pair (a, b) of two different object sets, got {pair!r}")
        for a, b in (pair, pair[::-1]):
            if a not in objects and a not in tertiary:
                raise ValueError(f"relate: '{a}' is not an object set of {[*objects, *tertiary]}")
            relate_names(a)
            if b not in related.setdefault(a, []):
                related[a].append(b)
    return related, {name: tuple(pair) for name, pair in tertiary.items()}


def build_pipeline_steps(
    channels_to_segment: dict[str, int] | None = None,
    channels_to_extract: Sequence[int] | None = None,
    features_to_extract: Sequence[str] = DEFAULT_FEATURES,
    extract_ncores: int | None = None,
    nahual_addresses=None,
    steps_to_write: Sequence[str] | None = None,
    trackastra_address: str | None = None,
    trackastra_parameters: dict | None = None,
    cp_measure_feature_kwargs: dict[str, dict] | None = None,
    *,
    volume_features: Sequence[str] | None = None,
    volume_coloc: bool = False,
    relate: Sequence[tuple[str, str]] | None = None,
    tertiary: dict[str, tuple[str, str]] | None = None,
    volume_relate: bool = False,
    secondary: dict[str, tuple[str, int]] | None = None,
    volume_secondary: bool | tuple[int, int] = False,
    propagate: dict[str, tuple] | None = None,
) -> dict:
    """Extension (not in the reference): `volume_features`, a sequence of per-channel volume family names
    (extraction.families.VOLUME: "intensity3d", "intensity3d_detail", "texture3d", "granularity3d"), makes every segment step
    segment Z-stacks as volumes (`do_3D=True`) and adds a `volume_<obj>` step per object set: sizeshape3d and projection3d, the
    given names under every channel of `channels_to_extract`, and with `volume_coloc=True` COLOC_METRICS under every channel
    pair.  Its rows go to profiles3d/<name>.parquet; the extract steps stay and measure the collapse, so profiles/ is the
    reference-faithful table and profiles3d/ the true 3-D one, joined on (metadata_tp, metadata_tile, metadata_object,
    Projection_Label = metadata_label).  With the default None the dict is the reference's.

    Extensions (not in the reference; CellProfiler's RelateObjects and IdentifyTertiaryObjects, csrc/feat_relate.hip): `relate`, pairs
    (a, b) of object sets, adds an `extractrelate_<obj>` step per object set named in a pair, which relates it to its partners in both
    directions (columns None/None/relate/Parent_<other>, ... on the rows of <obj>).  `tertiary`, {name: (outer, inner)}, adds a
    `tertiary_<name>` step right after the segment steps (outer's labels minus inner's objects: {"cytoplasm": ("cell", "nuclei")}),
    saved like them, and `extract_<name>` / `extractmulti_<name>` steps with the shared specs: rows with metadata_object = <name>
    whose metadata_label is the outer object's.  A name that is not an object set is a ValueError.  With both None the dict is the
    reference's.

    `volume_relate=True` (with `volume_features` and at least one of `relate` / `tertiary`, else a ValueError) takes both to the volume
    labels (csrc/feat_relate3d.hip): a `volumetertiary_<name>` step per tertiary entry right after the segment and tertiary steps
    (the tertiary volume of the two segment steps' kept volumes), a `volume_<name>` step that measures it with the shared volume tree,
    and a `volumerelate_<obj>` step per related object set (columns None/None/relate3d/Parent_<other>, ...).  Their rows go to
    profiles3d/: nuclei, cell and cytoplasm rows keyed by volume label, the relate3d columns joined onto the rows of their object set.
    With the default False the dict is what it is without the keyword.

    Extension (not in the reference; CellProfiler's IdentifySecondaryObjects, method "Distance - N", csrc/feat_secondary.hip):
    `secondary`, {name: (primary, distance)}, adds a `secondary_<name>` step {"distance": N} right after the segment steps and before
    any tertiary step (the primary's labels grown by N pixels, N an integer in 1..64: {"cell": ("nuclei", 10)}), saved like them, and
    `extract_<name>` / `extractmulti_<name>` steps with the shared specs: rows with metadata_object = <name> whose metadata_label is
    the primary object's.  A secondary name may be the outer or inner set of a `tertiary` entry and a member of a `relate` pair:
    secondary={"cell": ("nuclei", 10)}, tertiary={"cytoplasm": ("cell", "nuclei")} with channels_to_segment={"nuclei": 1} gives
    nuclei, cell and cytoplasm rows from one network pass.  A name that is already an object set, a primary that is not a segmented
    object set, a malformed entry, and — without `volume_secondary` — a secondary name in an entry that `volume_relate=True` would
    take to the volume labels (a `secondary_` step grows the collapsed 2-D labels) are ValueErrors.  With the default None the dict is
    what it is without the keyword.

    `volume_secondary` (with `volume_features` and at least one `secondary` entry, else a ValueError) takes the secondary sets to the
    volume labels (csrc/feat_secondary3d.hip): a `volumesecondary_<name>` step {"primary": "segment_<primary>", "distance", "spacing"}
    per secondary entry, after the tertiary steps and before any `volumetertiary_` step (the primary's kept volume grown on an integer
    lattice), and a `volume_<name>` step that measures it with the shared volume tree.  True: spacing (1, 1, 1) and the entry's N.  A
    pair of integers (p, q): a plane step is p/q pixels, so the spacing is (p, q, q) and the distance q N — N stays in pixels; (13, 5)
    stands for 0.6 um per plane over 0.23 um per pixel.  q N above 255 and a reach above 64 voxels along an axis are ValueErrors
    (features.secondary_volume_args), and so is any other value.  Under `volume_relate=True` the secondary names may then stand in
    `relate` / `tertiary`, their volumes coming from the `volumesecondary_` steps: secondary={"cell": ("nuclei", 10)},
    tertiary={"cytoplasm": ("cell", "nuclei")}, volume_features=(...), volume_relate=True, volume_secondary=True with only nuclei
    segmented puts nuclei, cell and cytoplasm rows into profiles3d/, joined on the volume label.  With the default False the dict and
    every refusal are what they are without the keyword.

    Extension (not in the reference; CellProfiler's IdentifySecondaryObjects, method "Propagation", csrc/feat_propagate.hip):
    `propagate`, {name: (primary, channel)} or {name: (primary, channel, options)}, adds a `propagate_<name>` step
    {"channel": c, **options} right after the secondary steps and before any tertiary step: the primary's labels grown along the stain
    in channel c of the tile's pixels, max-projected over Z.  options: "threshold", "regularization", "distance", "image_max"
    (features.propagate_args; {"distance": N} alone is "Distance - B"), and "auto_threshold", an option dict of
    features.auto_threshold_args in place of "threshold" ({"classes": 3, "middle": "foreground", "correction": 0.7}: every tile at its
    own three-class Otsu level, computed on the device), written into the step checked.  The step is saved like a segment step, its passed_data are
    [("masks", "segment_<primary>", "primary"), ("pixels", "tile")], and `extract_<name>` / `extractmulti_<name>` steps with the
    shared specs measure it: rows with metadata_object = <name> whose metadata_label is the primary object's.  A propagated name may
    be the outer or inner set of a `tertiary` entry and a member of a `relate` pair: propagate={"cell": ("nuclei", 0, {"threshold":
    400})}, tertiary={"cytoplasm": ("cell", "nuclei")}.  A name that is already a segmented, secondary or tertiary object set, a
    primary that is not a segmented object set, a malformed entry or option, and a propagated name in an entry that
    `volume_relate=True` takes to the volume labels (there is no volume form) are ValueErrors.  With the default None the dict is
    what it is without the keyword."""
    if channels_to_segment is None:
        channels_to_segment = {"nuclei": 1, "cell": 0}
    kind = "cellpose" if nahual_addresses is None else "nahual_cellpose"
    if channels_to_extract is None:
        channels_to_extract = list(channels_to_segment.values())
    objects = list(channels_to_segment)
    secondary = _secondary_sets(objects, secondary)
    propagate = _propagate_sets(objects, secondary, propagate)
    related, tertiary = _object_links(objects, relate, tertiary, secondary, propagate)
    if not isinstance(volume_relate, bool):
        raise ValueError(f"volume_relate must be a bool, got {volume_relate!r}")
    if volume_relate and (volume_features is None or not (related or tertiary)):
        raise ValueError("volume_relate=True needs volume_features (the volume labels come from 3-D segment steps) and at least one "
                         "of relate / tertiary")
    grown = _volume_secondary_sets(secondary, volume_secondary, volume_features)
    if volume_relate and not grown:
        reached = [name for name in secondary if name in related or any(name in pair for pair in tertiary.values())]
        if reached:
            raise ValueError(f"volume_relate=True: the secondary object sets {reached} have no volume form (a 'secondary_' step grows "
                             "2-D labels): keep them out of relate / tertiary, or leave volume_relate off")
    if volume_relate:
        reached = [name for name in propagate if name in related or any(name in pair for pair in tertiary.values())]
        if reached:
            raise ValueError(f"volume_relate=True: the propagated object sets {reached} have no volume form (a 'propagate_' step grows "
                             "2-D labels): keep them out of relate / tertiary, or leave volume_relate off")
    producer = ({obj: f"segment_{obj}" for obj in objects} | {name: f"secondary_{name}" for name in secondary}
                | {name: f"propagate_{name}" for name in propagate} | {name: f"tertiary_{name}" for name in tertiary})
    derived = (*secondary, *propagate, *tertiary)  # object sets without a segment step of their own, in step order

    steps = {"tile": {"tile_size": None}}
    for obj, ch in channels_to_segment.items():
        steps[f"segment_{obj}"] = {"segmenter_kwargs": {"kind": kind}, "channel_to_segment": ch}
    for name, (_, distance) in secondary.items():
        steps[f"secondary_{name}"] = {"distance": distance}
    for name, (_, channel, options) in propagate.items():
        steps[f"propagate_{name}"] = {"channel": channel, **options}
    for name in tertiary:
        steps[f"tertiary_{name}"] = {"shrink_inner": True}
    # the steps that keep the volume labels of an object set (a tertiary name: only under volume_relate)
    volume_producer = ({obj: f"segment_{obj}" for obj in objects} | {name: f"volumesecondary_{name}" for name in grown}
                       | {name: f"volumetertiary_{name}" for name in tertiary})
    for name, (distance, spacing) in grown.items():
        steps[f"volumesecondary_{name}"] = {"primary": f"segment_{secondary[name][0]}", "distance": distance, "spacing": spacing}
    if volume_relate:
        for name, (outer, inner) in tertiary.items():
            steps[f"volumetertiary_{name}"] = {"outer": volume_producer[outer], "inner": volume_producer[inner], "shrink_inner": True}

    # the single-channel spec is shared by every object set (as in the reference, where both
    # extract_<obj> entries point at the same dict)
    mono = {"tree": {"None": {"None": ("sizeshape",)}},
            "kwargs": _step_kwargs(extract_ncores, cp_measure_feature_kwargs)}
    for ch in channels_to_extract:
        mono["tree"][ch] = {"max": features_to_extract}
    multi = _create_extract_multich_tree(channels_to_extract, extract_ncores, cp_measure_feature_kwargs)
    for prefix, spec in (("extract", mono), ("extractmulti", multi)):
        if len(spec):
            for obj in (*objects, *derived):
                steps[f"{prefix}_{obj}"] = spec
    for obj, others in related.items():
        steps[f"extractrelate_{obj}"] = {"others": others, "kwargs": _step_kwargs(extract_ncores, cp_measure_feature_kwargs)}

    pipeline = {
        "steps": steps,
        "passed_data": {
            f"extract{m}_{obj}": [("masks", producer[obj]), ("pixels", "tile")]
            for obj in (*objects, *derived)
            for m in ("", "multi")
        },
        "passed_methods": {f"segment_{obj}": ("tile", "get_fczyx") for obj in objects},
        "save": [producer[obj] for obj in (*objects, *derived)],
        "save_interval": 1,
    }
    for name, (primary, _) in secondary.items():
        pipeline["passed_data"][f"secondary_{name}"] = [("masks", f"segment_{primary}", "primary")]
    for name, (primary, _, _) in propagate.items():
        pipeline["passed_data"][f"propagate_{name}"] = [("masks", f"segment_{primary}", "primary"), ("pixels", "tile")]
    for name, (outer, inner) in tertiary.items():
        pipeline["passed_data"][f"tertiary_{name}"] = [("masks", producer[outer], "outer"), ("masks", producer[inner], "inner")]
    for obj, others in related.items():
        pipeline["passed_data"][f"extractrelate_{obj}"] = [("masks", producer[obj])] + [("masks", producer[o], f"masks_{o}") for o in others]
    if volume_features is not None:
        tree = {"None": {"None": ["sizeshape3d", "projection3d"]}}
        for ch in channels_to_extract:
            tree[ch] = {"None": list(volume_features)}
        if volume_coloc:
            for pair in combinations(channels_to_extract, r=2):
                tree[pair] = {"None": list(COLOC_METRICS)}
        for obj in objects:
            steps[f"segment_{obj}"]["segmenter_kwargs"]["do_3D"] = True
            steps[f"volume_{obj}"] = {"tree": tree, "volume_from": f"segment_{obj}",
                                      "kwargs": _step_kwargs(extract_ncores, cp_measure_feature_kwargs)}
            pipeline["passed_data"][f"volume_{obj}"] = [("pixels", "tile")]
        # (the volumesecondary, volumetertiary and volumerelate steps read the kept volumes through the initialised steps, as a
        # volume step does: they have no passed_data entry)
        for name in (*grown, *(tertiary if volume_relate else ())):
            steps[f"volume_{name}"] = {"tree": tree, "volume_from": volume_producer[name],
                                       "kwargs": _step_kwargs(extract_ncores, cp_measure_feature_kwargs)}
            pipeline["passed_data"][f"volume_{name}"] = [("pixels", "tile")]
        if volume_relate:
            for obj, others in related.items():
                steps[f"volumerelate_{obj}"] = {"volume_from": volume_producer[obj], "others": {o: volume_producer[o] for o in others},
                                                "spacing": (1.0, 1.0, 1.0)}
    if steps_to_write is not None:
        pipeline["save"] = list(steps_to_write)
    if trackastra_address is not None:
        raise NotImplementedError("nahual_trackastra global steps are remote services (SURVEY §2 row 16): out of scope")
    return pipeline
