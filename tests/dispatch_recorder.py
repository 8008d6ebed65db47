"""
TEST INFRASTRUCTURE — a recording stand-in for FeatureEngine and for families._FanOut, and the cases of
tests/test_cpu_feature_dispatch.py.  `families.evaluate` runs against it without a GPU: what it decides (which engine method,
with which arguments, after which stream slot, into which columns) becomes an ordered list of events that is compared, exactly,
with tests/golden/feature_dispatch_trace.json (written by tests/golden/make_feature_dispatch_golden.py at the commit before
`evaluate` was split into `plan` and its executors).

An event is [name, arguments].  A tensor is logged as {"shape", "dtype"}, the object table as "table", a channel pair as a list.
Every fake launch fills the columns it owns with the column's own index, and a `cell_metrics` block holds -(100 k + j + 1) in
column j of the k-th block: after the run, a column that holds another column's index was copied from it ("columns" of a case).
`new_output` is an allocation, not a launch: it is kept as the case's "shape", not as an event, so that a refusal may move to
either side of it.

Two shims let the recorder drive the `evaluate` of that earlier commit, whose PlaneCache called ctypes itself:
  * `lib.aliby_reduce_z`, a fake of the C entry, and `ctx.handle` for its first argument;
  * `families._stream_ptr` patched to return 0 (it asked torch for the current HIP stream).
The fake entry and `RecordingEngine.reduce_z` log the same event: operation, rows, Z, plane size, in and out dtype codes.
"""
import contextlib
import math

import torch

from aliby_amd import _lib
from aliby_amd.extraction import families
from aliby_amd.extraction import features as feat
from aliby_amd.extraction.engine import FeatureEngine, ObjectTable
from aliby_amd.pipe_builder import build_pipeline_steps

_OUT_DTYPES = {_lib.U16: torch.uint16, _lib.F32: torch.float32, _lib.U64: torch.uint64, _lib.F64: torch.float64}


def _norm(v):
    if isinstance(v, torch.Tensor):
        return {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}
    if isinstance(v, ObjectTable):
        return "table"
    if isinstance(v, dict):
        return {str(k): _norm(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_norm(x) for x in v]
    return v


class _FakeLib:
    def __init__(self, events):
        self.events = events

    def aliby_reduce_z(self, handle, src, in_dt, rows, Z, plane, op, dst, out_dt, stream):
        self.events.append(["reduce_z", {"op": op, "rows": rows, "Z": Z, "plane": plane, "in_dt": in_dt, "out_dt": out_dt}])
        return 0


class _FakeCtx:
    handle = 0


class RecordingEngine:
    CELL_COLUMNS = FeatureEngine.CELL_COLUMNS

    def __init__(self, coloc_pairs_result=True):
        self.events = []
        self.coloc_pairs_result = coloc_pairs_result
        self.lib, self.ctx = _FakeLib(self.events), _FakeCtx()
        self.out = None
        self.cell_blocks = 0

    def _log(self, name, **args):
        self.events.append([name, {k: _norm(v) for k, v in args.items()}])

    @staticmethod
    def _mark(out, col0, n):
        for j in range(n):
            out[:, col0 + j] = float(col0 + j)

    # ---- not launches
    def timed(self, name):
        return contextlib.nullcontext()

    def new_output(self, n_obj, n_cols):
        self.out = torch.full((max(n_obj, 1), max(n_cols, 1)), float("nan"), dtype=torch.float64)[:n_obj]
        return self.out

    # ---- shared inputs
    def reduce_z(self, t, op, in_dt, out_dt):
        *lead, Z, Y, X = t.shape
        self._log("reduce_z", op=op, rows=math.prod(lead), Z=Z, plane=Y * X, in_dt=in_dt, out_dt=out_dt)
        return torch.empty((*lead, Y, X), dtype=_OUT_DTYPES[out_dt])

    def mec(self, labels, table):
        self._log("mec", labels=labels, table=table)

    def radial_geometry(self, labels, table, bin_count, maximum_radius=None):
        self._log("radial_geometry", labels=labels, table=table, bin_count=bin_count, maximum_radius=maximum_radius)

    def rank_planes(self, labels, planes, dtype, table, channels):
        self._log("rank_planes", labels=labels, planes=planes, dtype=dtype, table=table, channels=channels)

    def cell_metrics(self, labels, planes, dtype, channel, table):
        self._log("cell_metrics", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table)
        block = torch.empty((table.n_obj, len(self.CELL_COLUMNS)), dtype=torch.float64)
        for j in range(block.shape[1]):
            block[:, j] = -float(100 * self.cell_blocks + j + 1)
        self.cell_blocks += 1
        return block

    # ---- launches that write columns of `out`
    def intensity(self, labels, planes, dtype, channel, table, out, col0, edge_measurements=True):
        self._log("intensity", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table, out=out, col0=col0,
                  edge_measurements=edge_measurements)
        self._mark(out, col0, len(feat.intensity_names(edge_measurements)))

    def sizeshape(self, labels, table, out, col0):
        self._log("sizeshape", labels=labels, table=table, out=out, col0=col0)
        self._mark(out, col0, len(feat.sizeshape_names()))

    def feret(self, labels, table, out, col0):
        self._log("feret", labels=labels, table=table, out=out, col0=col0)
        self._mark(out, col0, len(feat.feret_names()))

    def zernike(self, labels, planes, dtype, channel, table, out, col0, weighted):
        self._log("zernike", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table, out=out, col0=col0,
                  weighted=weighted)
        self._mark(out, col0, len(feat.radial_zernike_names() if weighted else feat.zernike_names()))

    def radial_zernikes_multi(self, labels, planes, dtype, channels, table, out, col0s):
        self._log("radial_zernikes_multi", labels=labels, planes=planes, dtype=dtype, channels=channels, table=table, out=out,
                  col0s=col0s)
        for c0 in col0s:
            self._mark(out, c0, len(feat.radial_zernike_names()))

    def texture(self, labels, planes, dtype, channel, table, out, col0, scale=3, gray_levels=256):
        self._log("texture", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table, out=out, col0=col0,
                  scale=scale, gray_levels=gray_levels)
        self._mark(out, col0, len(feat.texture_names(scale, gray_levels)))

    def radial_distribution(self, labels, planes, dtype, channel, table, out, col0, bin_count=4, scaled=True, maximum_radius=100):
        self._log("radial_distribution", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table, out=out,
                  col0=col0, bin_count=bin_count, scaled=scaled, maximum_radius=maximum_radius)
        self._mark(out, col0, len(feat.radial_distribution_names(bin_count, scaled)))

    def granularity(self, labels, planes, dtype, channel, table, out, col0, **kw):
        self._log("granularity", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table, out=out, col0=col0, **kw)
        self._mark(out, col0, len(feat.granularity_names(kw.get("granular_spectrum_length", 16))))

    def nuc_est_conv(self, labels, planes, dtype, channel, table, out, col0, median=None):
        self._log("nuc_est_conv", labels=labels, planes=planes, dtype=dtype, channel=channel, table=table, out=out, col0=col0,
                  median=median, median_from=None if median is None or not median.numel() else float(median[0]))
        self._mark(out, col0, 1)

    def nuc_conv_3d(self, labels, stack, dtype, channel, table, out, col0):
        self._log("nuc_conv_3d", labels=labels, stack=stack, dtype=dtype, channel=channel, table=table, out=out, col0=col0)
        self._mark(out, col0, 1)

    def coloc_pairs(self, labels, planes, dtype, pairs, table, out, thr=15.0, scale_max=255.0):
        self._log("coloc_pairs", labels=labels, planes=planes, dtype=dtype, pairs=pairs, table=table, out=out, thr=thr,
                  scale_max=scale_max, returns=self.coloc_pairs_result)
        if self.coloc_pairs_result:
            for _, cols in pairs:
                for c0 in cols.values():
                    self._mark(out, c0, 2)
        return self.coloc_pairs_result

    def coloc(self, labels, planes, dtype, ch0, ch1, table, out, cols, thr=15.0, scale_max=255.0):
        self._log("coloc", labels=labels, planes=planes, dtype=dtype, ch0=ch0, ch1=ch1, table=table, out=out, cols=cols, thr=thr,
                  scale_max=scale_max)
        for c0 in cols.values():
            self._mark(out, c0, 2)


def recording_fanout(events):
    """A class to put in place of families._FanOut: logs fork, slot k (the ordinal of each next_stream()) and join."""

    class RecordingFanOut:
        def __init__(self, eng, table, out):
            self.k = 0

        def fork(self):
            events.append(["fork", {}])

        def next_stream(self):
            events.append([f"slot {self.k}", {}])
            self.k += 1
            return contextlib.nullcontext()

        def join(self):
            events.append(["join", {}])

    return RecordingFanOut


def fake_table(n_obj=4):
    return ObjectTable(dev=None, host=None, offsets=None, n_obj=n_obj, max_area=100 if n_obj else 0, max_h=12 if n_obj else 0,
                       max_w=12 if n_obj else 0)


def instructions_of(tree):
    from aliby_amd.extraction.extract import flatten, kv

    return kv(flatten(tree))


def _builder_trees(n_channels=5):
    steps = build_pipeline_steps(channels_to_extract=list(range(n_channels)))["steps"]
    return steps["extract_nuclei"]["tree"], steps["extractmulti_nuclei"]["tree"]


def _pairs_tree(n, metrics=("pearson", "costes", "manders_fold", "rwc"), red_ch="None"):
    return {(a, b): {red_ch: {"max": list(metrics)}} for a in range(n) for b in range(a + 1, n)}


def cases():
    """name -> dict(tree, kwargs, multi, n_obj, Z, C, pixels ("uint16" | "float32" | None), coloc_pairs_result)."""
    mono5, multi5 = _builder_trees(5)
    cell = ["median", "mean", "nuc_est_conv"]
    c = {}

    def add(name, tree, kwargs=None, multi=False, n_obj=4, Z=1, C=5, pixels="uint16", coloc_pairs_result=True):
        assert name not in c
        c[name] = dict(tree=tree, kwargs=kwargs or {}, multi=multi, n_obj=n_obj, Z=Z, C=C, pixels=pixels,
                       coloc_pairs_result=coloc_pairs_result)

    # builder trees
    add("builder_mono_5ch", mono5)
    add("builder_multi_5ch", multi5, multi=True)
    add("builder_mono_5ch_no_objects", mono5, n_obj=0)
    # copied columns
    add("feret_with_sizeshape", {"None": {"None": ["sizeshape", "feret"]}})
    add("feret_alone", {"None": {"None": ["feret"]}})
    add("zernike_feret_three_channels", {ch: {"max": ["zernike", "feret"]} for ch in range(3)})
    # zernike
    add("radial_zernikes_one_channel", {0: {"max": ["radial_zernikes"]}})
    add("radial_zernikes_three_channels", {ch: {"max": ["radial_zernikes"]} for ch in range(3)})
    add("radial_zernikes_two_reducers", {0: {"max": ["radial_zernikes"], "add": ["radial_zernikes"]},
                                         1: {"max": ["radial_zernikes"], "add": ["radial_zernikes"]}}, Z=3)
    # cell and localisation metrics
    add("cell_metrics_one_channel", {1: {"max": cell}})
    add("cell_metrics_two_channels", {1: {"max": cell}, 2: {"max": cell}})
    add("cell_metrics_mask_only_and_pixels", {"None": {"None": ["area", "volume"]}, 0: {"max": ["area", "median"]}})
    add("nuc_conv_3d_unreduced", {0: {"None": ["nuc_conv_3d"]}, 1: {"max": ["mean"]}}, Z=3)
    add("ratio", {0: {"max": ["ratio"]}})
    add("granularity_keywords", {0: {"max": ["granularity", "intensity"]}},
        kwargs={"granularity": {"subsample_size": 0.5, "element_size": 4, "granular_spectrum_length": 6}})
    # reducers and pixels
    for Z in (1, 3):
        for px in ("uint16", "float32"):
            add(f"reducers_Z{Z}_{px}", {0: {"max": ["intensity"], "add": ["intensity"], "div": ["intensity"]},
                                        1: {"add": ["texture", "feret"]}}, Z=Z, pixels=px)
    add("add_uint16_Z257_refused", {0: {"max": ["intensity"], "add": ["intensity"]}}, Z=257, C=1)
    add("bad_reducer_mean", {0: {"max": ["intensity"], "mean": ["intensity"]}}, Z=3)
    add("bad_reducer_under_mask_only_family", {0: {"max": ["intensity"], "median": ["zernike"]}}, Z=3)
    add("no_pixels_pixel_free_tree", {"None": {"None": ["sizeshape", "zernike", "area"]}, 0: {"max": ["feret"]}}, pixels=None)
    add("no_pixels_needed", {"None": {"None": ["sizeshape"]}, 0: {"max": ["intensity"]}}, pixels=None)
    add("no_pixels_needed_after_join", {"None": {"None": ["sizeshape"]}, 0: {"max": ["median"]}}, pixels=None)
    # multi
    add("multi_default_keywords", _pairs_tree(3), multi=True)
    add("multi_thr_split", _pairs_tree(3), kwargs={"manders_fold": {"thr": 30}}, multi=True)
    add("multi_costes_scale_max", _pairs_tree(3), kwargs={"costes": {"scale_max": 4095}}, multi=True)
    add("multi_single_pair", _pairs_tree(2), multi=True)
    add("multi_coloc_pairs_false", _pairs_tree(3), multi=True, coloc_pairs_result=False)
    add("multi_two_reducers", {(0, 1): {"None": {"max": ["pearson", "rwc"], "add": ["pearson"]}},
                               (0, 2): {"None": {"max": ["rwc"], "add": ["costes", "rwc"]}}}, multi=True, Z=3)
    # (under a red_ch other than "None" the name is looked up among the single-channel families: a colocalisation name is
    # unknown there, a single-channel name reaches the refusal of channel-combining instructions)
    add("multi_red_ch_coloc_metric", _pairs_tree(3, red_ch="max"), multi=True)
    add("multi_red_ch_mono_metric", {(0, 1): {"max": {"max": ["intensity"]}}}, multi=True)
    add("multi_no_pixels", _pairs_tree(3), multi=True, pixels=None)
    # refusals
    add("unknown_metric", {0: {"max": ["intensity", "no_such_metric"]}})
    add("multi_unknown_metric", {(0, 1): {"None": {"max": ["pearson", "intensity"]}}}, multi=True)
    add("unbuilt_keyword", {0: {"max": ["intensity", "texture"]}}, kwargs={"texture": {"distance": 2}})
    add("unbuilt_keyword_family_not_in_tree", {0: {"max": ["intensity"]}}, kwargs={"texture": {"distance": 2}})
    add("keyword_of_in_repo_function_ignored", {0: {"max": ["median"]}}, kwargs={"median": {"anything": 1}})
    add("stack_metric_under_reduced_channel", {0: {"max": ["nuc_conv_3d"]}}, Z=3)
    add("stack_metric_without_channel", {"None": {"None": ["nuc_conv_3d"]}}, Z=3)
    add("ordinary_metric_under_None", {0: {"None": ["intensity"]}}, Z=3)
    add("granularity_objects_mask", {0: {"max": ["intensity", "granularity"]}}, kwargs={"granularity": {"image_mask": "objects"}})
    return c


def run_case(case, monkeypatch_setattr):
    """Replays one case through families.evaluate -> dict as stored in the golden.  `monkeypatch_setattr(obj, name, value)`
    patches for the length of the caller's test (pytest's monkeypatch.setattr, or the generator's own)."""
    eng = RecordingEngine(case["coloc_pairs_result"])
    monkeypatch_setattr(families, "_FanOut", recording_fanout(eng.events))
    if hasattr(families, "_stream_ptr"):  # the second shim (see the module's docstring)
        monkeypatch_setattr(families, "_stream_ptr", lambda: 0)
    planes = None
    if case["pixels"] is not None:
        dtype = getattr(torch, case["pixels"])
        planes = (torch.zeros((2, case["C"], case["Z"], 16, 20), dtype=dtype), _lib.U16 if dtype == torch.uint16 else _lib.F32)
    labels = torch.zeros((2, 16, 20), dtype=torch.uint16)
    rec = {}
    try:
        out, blocks = families.evaluate(eng, labels, fake_table(case["n_obj"]), planes, instructions_of(case["tree"]), case["kwargs"],
                                        multi=case["multi"])
    except Exception as e:  # noqa: BLE001 — the type and the text are what is recorded
        rec["raises"] = [type(e).__name__, str(e)]
    else:
        assert out is eng.out
        rec["blocks"] = [[c0, names] for c0, names in blocks]
        rec["shape"] = list(out.shape)
        row = out[0].tolist() if out.shape[0] else []
        rec["columns"] = [None if math.isnan(v) else int(v) for v in row]
    rec["events"] = eng.events
    return rec
