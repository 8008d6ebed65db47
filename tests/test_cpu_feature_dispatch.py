"""
The feature dispatcher (aliby_amd/extraction/families.py) without a GPU: every case of tests/dispatch_recorder.py is replayed
through `families.evaluate` on a recording engine and compared, exactly, with tests/golden/feature_dispatch_trace.json — the
engine calls with their arguments, the fork / slot / join sequence, the column layout and the copied columns, and for the refused
cases the events up to the raise with the exception's type and text.  `families.plan`, the part that needs no engine, is then
asked directly for the refusals and for the grouping of the colocalisation launches.
"""
import json
from pathlib import Path

import pytest

from tests import dispatch_recorder as dr

GOLDEN = json.loads((Path(__file__).parent / "golden" / "feature_dispatch_trace.json").read_text())
CASES = dr.cases()


def test_golden_holds_exactly_the_cases():
    assert list(GOLDEN) == list(CASES)
    # the figures of the builder's 5-channel trees: instructions, columns, engine calls (events less fork / slot / join)
    calls = lambda t: sum(1 for name, _ in t["events"] if name not in ("fork", "join") and not name.startswith("slot "))  # noqa: E731
    mono, multi = GOLDEN["builder_mono_5ch"], GOLDEN["builder_multi_5ch"]
    assert (len(mono["blocks"]), mono["shape"], calls(mono)) == (31, [4, 963], 33)
    assert (len(multi["blocks"]), multi["shape"], calls(multi)) == (40, [4, 80], 11)


@pytest.mark.parametrize("name", list(CASES))
def test_dispatch_is_as_recorded(name, monkeypatch):
    got = json.loads(json.dumps(dr.run_case(CASES[name], monkeypatch.setattr)))
    want = GOLDEN[name]
    assert got.get("raises") == want.get("raises")
    assert got["events"] == want["events"]
    assert got == want


def test_rules_the_trace_pins():
    """The rules named where the dispatcher was split, read off the golden itself (so that a regenerated file cannot drop them)."""
    names = lambda case: [e[0] for e in GOLDEN[case]["events"]]  # noqa: E731
    # feret beside sizeshape: no launch of its own, its two columns copied out of the sizeshape block
    t = GOLDEN["feret_with_sizeshape"]
    assert names("feret_with_sizeshape").count("feret") == 0 and all(c is not None and c < 78 for c in t["columns"][78:80])
    assert names("feret_alone").count("feret") == 1
    # a pixel-independent family listed under three channels: one launch, two copies
    t = GOLDEN["zernike_feret_three_channels"]
    assert names("zernike_feret_three_channels").count("zernike") == 1 and t["columns"][32:62] == t["columns"][0:30] == list(range(30))
    # one cell_metrics block per (plane, channel), shared by median, mean and nuc_est_conv
    assert names("cell_metrics_one_channel").count("cell_metrics") == 1 and names("cell_metrics_two_channels").count("cell_metrics") == 2
    # manders_fold's thr does not leak into rwc: two launches, the threshold-free metrics ride with the first (thr 15, rwc's)
    first, second = [e[1] for e in GOLDEN["multi_thr_split"]["events"] if e[0] == "coloc_pairs"]
    assert (first["thr"], second["thr"]) == (15.0, 30.0)
    assert all(sorted(cols) == ["costes", "pearson", "rwc"] for _, cols in first["pairs"])
    assert all(sorted(cols) == ["manders_fold"] for _, cols in second["pairs"])
    # a single pair, and a declined coloc_pairs, go pair by pair over the fan-out slots
    assert names("multi_single_pair") == ["rank_planes", "fork", "slot 0", "coloc", "join"]
    assert names("multi_coloc_pairs_false")[3:] == ["coloc_pairs", "fork", "slot 0", "coloc", "slot 1", "coloc", "slot 2", "coloc", "join"]
    # without objects nothing is prefetched per object and the Zernike channels are not grouped
    assert not {"mec", "radial_geometry", "radial_zernikes_multi"} & set(names("builder_mono_5ch_no_objects"))


# ---- plan(): pure — no engine, table or tensor in sight

REFUSED_BEFORE_ANY_EVENT = [n for n, t in GOLDEN.items() if "raises" in t and not t["events"] and n != "multi_no_pixels"]


def test_refusals_split_as_expected():
    assert sorted(REFUSED_BEFORE_ANY_EVENT) == sorted([
        "multi_red_ch_coloc_metric", "multi_red_ch_mono_metric", "unknown_metric", "multi_unknown_metric", "unbuilt_keyword",
        "stack_metric_under_reduced_channel", "stack_metric_without_channel"])


@pytest.mark.parametrize("name", REFUSED_BEFORE_ANY_EVENT)
def test_plan_refuses_what_evaluate_refused_before_its_first_launch(name):
    from aliby_amd.extraction import families

    case = CASES[name]
    with pytest.raises(Exception) as e:
        families.plan(dr.instructions_of(case["tree"]), case["kwargs"], case["multi"])
    assert [type(e.value).__name__, str(e.value)] == GOLDEN[name]["raises"]


@pytest.mark.parametrize("name", [n for n, t in GOLDEN.items() if "raises" in t and (t["events"] or n == "multi_no_pixels")])
def test_plan_accepts_what_is_refused_while_launching(name):
    """A bad reducer, missing pixels and granularity's object mask surface from the launch that meets them, where the trace has them."""
    from aliby_amd.extraction import families

    case = CASES[name]
    families.plan(dr.instructions_of(case["tree"]), case["kwargs"], case["multi"])


@pytest.mark.parametrize("name", [n for n, t in GOLDEN.items() if "raises" not in t])
def test_plan_layout_matches_the_trace(name):
    from aliby_amd.extraction import families

    case = CASES[name]
    p = families.plan(dr.instructions_of(case["tree"]), case["kwargs"], case["multi"])
    assert json.loads(json.dumps([list(b) for b in p.blocks])) == GOLDEN[name]["blocks"]
    assert max(p.n_cols, 1) == GOLDEN[name]["shape"][1]
    assert [s.col0 for s in p.steps] == [b[0] for b in p.blocks]
    assert [(s.family, s.kw) for s in p.steps] == [
        ((families.MULTI if case["multi"] else families.MONO)[i[-1]], dict(case["kwargs"].get(i[-1], {})))
        for i in dr.instructions_of(case["tree"])]


def test_plan_groups_colocalisation_launches():
    from aliby_amd.extraction import families

    tree = dr._pairs_tree(3)
    pairs = [(0, 1), (0, 2), (1, 2)]
    col = lambda k, j: 8 * k + 2 * j  # noqa: E731 — pair k, j-th of pearson / costes / manders_fold / rwc
    p = families.plan(dr.instructions_of(tree), {}, multi=True)
    assert p.prefetch == [("max", pair, True) for pair in pairs]
    assert p.batches == {("max", 15.0, 255.0): [(pair, {"pearson": col(k, 0), "costes": col(k, 1), "manders_fold": col(k, 2), "rwc": col(k, 3)})
                                                for k, pair in enumerate(pairs)]}
    # thr of manders_fold alone: its launch splits off, the rest rides with rwc's default threshold
    p = families.plan(dr.instructions_of(tree), {"manders_fold": {"thr": 30}}, multi=True)
    assert list(p.batches) == [("max", 15.0, 255.0), ("max", 30.0, 255.0)]
    assert p.batches[("max", 30.0, 255.0)] == [(pair, {"manders_fold": col(k, 2)}) for k, pair in enumerate(pairs)]
    assert all(sorted(cols) == ["costes", "pearson", "rwc"] for _, cols in p.batches[("max", 15.0, 255.0)])
    assert p.prefetch == [("max", pair, ranks) for pair in pairs for ranks in (True, False)]
    # scale_max of costes reaches every launch of its pair
    p = families.plan(dr.instructions_of(tree), {"costes": {"scale_max": 4095}}, multi=True)
    assert list(p.batches) == [("max", 15.0, 4095.0)]
    # without rwc no rank planes are asked for; two reducers make two launches
    p = families.plan(dr.instructions_of({(0, 1): {"None": {"max": ["pearson"], "add": ["costes"]}}}), {}, multi=True)
    assert p.prefetch == [("max", (0, 1), False), ("add", (0, 1), False)] and list(p.batches) == [("max", 15.0, 255.0), ("add", 15.0, 255.0)]
    # a single-channel plan has neither
    p = families.plan(dr.instructions_of({0: {"max": ["intensity"]}}), {})
    assert p.prefetch == [] and p.batches == {}


def test_registry_has_one_shape_and_is_complete_at_import():
    import dataclasses

    from aliby_amd.extraction import families
    from aliby_amd.extraction.engine import FeatureEngine
    from aliby_amd.pipe_builder import COLOC_METRICS, DEFAULT_FEATURES

    for reg in (families.MONO, families.MULTI):
        for name, fam in reg.items():
            assert isinstance(fam, families.Family) and dataclasses.is_dataclass(fam), name
            assert isinstance(fam.needs_pixels, bool) and isinstance(fam.after_join, bool) and isinstance(fam.stack, bool), name
    assert set(DEFAULT_FEATURES) | {"sizeshape", "granularity"} <= set(families.MONO) and set(COLOC_METRICS) == set(families.MULTI)
    assert sorted(n for n, f in families.MONO.items() if f.after_join and n not in FeatureEngine.CELL_COLUMNS) == [
        "granularity", "nuc_conv_3d", "nuc_est_conv"]
    assert families.register_optional(FeatureEngine) is None  # still importable: the benchmark calls it
    assert set(families.BUILT_KWARGS) <= set(families.CP_MEASURE_NAMES)


def test_lds_resident_is_the_fan_out_condition():
    from aliby_amd.extraction.engine import ObjectTable

    table = lambda n, h, w: ObjectTable(dev=None, host=None, offsets=None, n_obj=n, max_area=h * w, max_h=h, max_w=w)  # noqa: E731
    assert table(0, 0, 0).lds_resident is False
    assert table(3, 64, 64).lds_resident is True
    assert table(3, 65, 64).lds_resident is False
    assert "object_launch.h" in ObjectTable.lds_resident.__doc__
