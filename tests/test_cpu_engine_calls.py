"""
The engine's host layer (aliby_amd/extraction/engine.py) without a GPU: every case of tests/engine_call_recorder.py runs the real
`FeatureEngine` on CPU tensors over a recording stand-in for the library and is compared, exactly, with
tests/golden/engine_call_trace.json — every C call with its arguments, the profile group around it, what the method returns, and
for the refused cases the exception's type and text with the events before it.  A few rules are then read off the golden itself.
"""
import ctypes as C
import json
from pathlib import Path

import pytest

from aliby_amd import _lib
from tests import engine_call_recorder as er

GOLDEN = json.loads((Path(__file__).parent / "golden" / "engine_call_trace.json").read_text())
CASES = er.cases()


def _calls(case):
    return [e for e in GOLDEN[case]["events"] if e[0].startswith("aliby_")]


def test_golden_holds_exactly_the_cases():
    assert list(GOLDEN) == list(CASES)
    assert Path(__file__).with_name("golden").joinpath("engine_call_trace.json").stat().st_size <= 360 * 1024


@pytest.mark.parametrize("name", list(CASES))
def test_calls_are_as_recorded(name, monkeypatch):
    got = json.loads(json.dumps(er.run_case(CASES[name], monkeypatch.setattr)))
    want = GOLDEN[name]
    assert got.get("raises") == want.get("raises")
    assert got["events"] == want["events"]
    assert got == want


def test_every_call_has_the_arity_of_its_signature():
    seen = set()
    for name in GOLDEN:
        for entry, args in _calls(name):
            assert len(args) == len(_lib._SIGNATURES[entry][1]), (name, entry)
            seen.add(entry)
    assert len(seen) >= 41


def test_every_launch_is_inside_its_group_or_untimed():
    """A timed launch sits alone between the enter and the exit of one group; the untimed entries are the ones named here."""
    untimed = {"aliby_relabel_sequential", "aliby_track_stitch", "aliby_labels_apply_lut"}
    for name, t in GOLDEN.items():
        group = None
        for kind, what in t["events"]:
            if kind == "enter":
                assert group is None, name
                group = what
            elif kind == "exit":
                assert group == what, name
                group = None
            elif kind.startswith("aliby_") and _lib._SIGNATURES[kind][0] is not C.c_size_t:
                assert group is not None or (kind in untimed and (kind != "aliby_track_stitch" or name.startswith("stitch_planes"))), (name, kind)
        assert group is None, name


def test_the_caches_launch_once():
    for name in ("cache_mec", "cache_radial_geometry_scaled", "cache_radial_geometry_unscaled", "cache_rank_planes"):
        kinds = [e[0] for e in GOLDEN[name]["events"]]
        assert kinds.index("mark") > 0 and kinds[-1] == "mark", name  # nothing after the mark of the second call
        assert GOLDEN[name]["returns"][-1] == "the same object", name
    # per channel: 0, then only 2, then both again for other planes
    t = GOLDEN["cache_rank_planes_per_channel"]
    assert [e[1][8] if e[0] != "mark" else "|" for e in t["events"] if e[0] not in ("enter", "exit")] == [0, "|", 2, "|", 0, 2]
    t = GOLDEN["cache_offsets_dev"]
    assert t["returns"][1:] == [[0, 1, 4], "the same object"] and len(_calls("cache_offsets_dev")) == 1


def test_a_table_without_its_cache_attributes_has_empty_caches(monkeypatch):
    """The GPU tests copy a table and drop the caches from the copy's __dict__ (tests/test_gpu_object_forms.py `hinted`): every
    cache must then read as empty and fill again, and none of them is part of the table's repr or its comparison."""
    import dataclasses

    from aliby_amd.extraction.engine import ObjectTable

    caches = ("_mec", "_offsets_dev", "_binmaps", "_ranks")
    fields = dataclasses.fields(ObjectTable)
    assert [f.name for f in fields] == ["dev", "host", "offsets", "n_obj", "max_area", "max_h", "max_w", *caches]
    assert all(not f.repr and not f.compare and f.default is None for f in fields[7:])
    monkeypatch.setattr(er.engine_mod, "_ptr", er.Pointer)
    monkeypatch.setattr(er.engine_mod, "_stream_ptr", lambda: 0)
    run, t, labels, planes = er.Run(), er.table(), er.labels(), er.planes()
    for _ in range(2):
        for name in caches:
            t.__dict__.pop(name, None)
        before = len(run.eng.events)
        run.eng.mec(labels, t), run.eng.radial_geometry(labels, t, 4), run.eng.rank_planes(labels, planes, er.U16, t, (1,))
        run.eng._offsets_dev(t, "cpu")
        assert len(run.eng.events) - before == 9  # three launches, each between its enter and exit
        assert t._mec is not None and t._offsets_dev is not None and list(t._binmaps) == [4] and len(t._ranks) == 1


def test_radial_zernike_channels_are_grouped_by_five_and_never_leave_one():
    groups = {}
    for n in (1, 2, 5, 6, 7, 11):
        groups[n] = [1 if entry == "aliby_features_zernike" else args[10] for entry, args in _calls(f"radial_zernikes_multi_{n}")
                     if entry != "aliby_object_mec"]
    assert groups == {1: [1], 2: [2], 5: [5], 6: [4, 2], 7: [5, 2], 11: [5, 4, 2]}


def test_coloc_pairs_verdicts():
    assert GOLDEN["coloc_pairs_accepted"]["returns"] is True and _calls("coloc_pairs_accepted")[-1][0] == "aliby_features_coloc_pairs"
    for name in ("coloc_pairs_29_pairs", "coloc_pairs_9_channels", "coloc_pairs_8_channels_area_5000"):
        assert GOLDEN[name] == {"returns": False, "events": []}, name


def test_texture_alone_gets_the_raw_dtype_code():
    assert _calls("texture_u8w")[0][1][3] == _lib.U8W
    for name in ("intensity_u8w", "granularity", "cell_metrics", "nuc_est_conv", "coloc_with_rwc", "zernike_weighted", "trap_background"):
        assert _calls(name)[-1][1][3] == _lib.U16, name


def test_no_null_output_with_rows():
    """relate and relate3d hand over a null matrix exactly for the side without rows; no other launch has a null pointer but
    the context and the stream of the stand-in and the inputs that are optional in the C interface."""
    optional = {"aliby_features_zernike": {2}, "aliby_features_cell": {2}, "aliby_features_coloc": {21, 22}, "aliby_features_coloc_pairs": {17, 18},
                "aliby_track_stitch": {10, 11}}
    relate = {"aliby_features_relate": ((7, 19), (11, 22)), "aliby_features_relate3d": ((7, 10), (8, 13))}
    n_relate = 0
    for name in GOLDEN:
        for entry, args in _calls(name):
            kinds = _lib._SIGNATURES[entry][1]
            nulls = {k for k, (kind, v) in enumerate(zip(kinds, args)) if kind is C.c_void_p and v == "null"}
            if kinds and kinds[0] is C.c_void_p and kinds[-1] is C.c_void_p and _lib._SIGNATURES[entry][0] is not C.c_size_t:
                assert {0, len(args) - 1} <= nulls, (name, entry)
                nulls -= {0, len(args) - 1}
            if entry in relate:
                for rows_at, out_at in relate[entry]:
                    rows = args[rows_at] if isinstance(args[rows_at], int) else args[rows_at]["values"][-1]
                    assert (out_at in nulls) == (rows == 0), (name, entry)
                    nulls.discard(out_at)
                    n_relate += rows == 0
            assert nulls <= optional.get(entry, set()), (name, entry, nulls)
    assert n_relate >= 4
