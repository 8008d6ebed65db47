"""
nuc_est_conv on the GPU (aliby_amd/csrc/feat_localisation.hip) against tests/localisation_ref.py, the float64 restatement that
tests/test_cpu_localisation_ref.py pins to the reference's own function, through every layer: the engine call in each launch
form, functions.nuc_est_conv, the extraction tree and run_positions.

Pass bar: rtol 1e-4, atol 1e-9, NaN equal to NaN; 0.0 and bit-equality where a case states them.  Every comparison prints its
largest relative error first.  Measured on an MI355X: see test_mixed_batch.

Launch forms, restated from the header of feat_localisation.hip (hw = ceil(2 sqrt(0.085 max_area / pi)), wd = min(X, max_w + 2 hw)):

    need = r16(8 (max_h wd + 2 hw + 1) + 4 max_h max_w)      LDS up to 64 KiB, the attribute raised above 32 KiB, else global

The mixed batch (case 1) holds a 48 x 49 object of 1957 pixels: 40 000 bytes, so its true limits are already the "attr" form
and no hint, which may only grow a capacity, puts it in plain LDS.  Its rungs are attr / glob / glob; the border scene (objects
of 12 x 12) runs lds / lds / attr / glob, and each scene's rows are bit-equal across its rungs.
"""
import math

import numpy as np
import pytest

from tests import localisation_ref as lr
from tests.test_gpu_object_forms import hinted, stride_scene

pytestmark = pytest.mark.gpu

KIB = 1024
RUNGS = {
    "mixed_u16": {"true": None, "64x64": (64, 64, 4096), "180x180": (180, 180, 8192)},
    "border": {"true": None, "40x40": (40, 40, 1600), "64x56": (64, 56, 3000), "100x100": (100, 100, 8000)},
}
RUNGS["mixed_f32"] = RUNGS["mixed_u16"]


def need_bytes(h, w, a, X, ore=0.085):
    hw = math.ceil(2.0 * math.sqrt(ore * a / math.pi))
    wd = min(X, w + 2 * hw)
    return (8 * (h * wd + 2 * hw + 1) + 4 * h * w + 15) // 16 * 16


def form(h, w, a, X, ore=0.085):
    need = need_bytes(h, w, a, X, ore)
    return "glob" if need > 64 * KIB else ("attr" if need > 32 * KIB else "lds")


_DEVICE = {}


def device(engine, name):
    """-> (labels, planes, dtype code, object table) of a scene on the GPU, made once"""
    if name not in _DEVICE:
        from aliby_amd.extraction.engine import to_device_planes, to_device_u16

        s = lr.scenes()[name]
        dl = to_device_u16(np.array(s["labels"]))
        dp, dt = to_device_planes(np.array(s["planes"]))
        tab = engine.object_table(dl)
        assert tab.n_obj == len(lr.rows(s))
        _DEVICE[name] = (dl, dp, dt, tab)
    return _DEVICE[name]


def run(engine, name, hint=None, **override):
    import torch

    s = lr.scenes()[name]
    dl, dp, dt, tab = device(engine, name)
    out = engine.new_output(tab.n_obj, 3)
    kw = dict(s["kwargs"], **override)
    assert engine.nuc_est_conv(dl, dp, dt, s["channel"], hinted(tab, hint), out, 1, **kw) == 1
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 2]).all()  # only column col0 is written
    return got[:, 1].copy()


def close(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    both = ~(np.isnan(got) | np.isnan(want))
    rel = np.abs(got[both] - want[both]) / np.maximum(np.abs(want[both]), 1e-300)
    rel = np.where(got[both] == want[both], 0.0, rel)
    print(f"{what}: largest relative error {rel.max() if rel.size else 0.0:.3g} over {int(both.sum())} rows")
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-9, equal_nan=True), (what, got, want)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ------------------------------------------------------------------------------------------------------------------- cases 1-7
@pytest.mark.parametrize("name", ["mixed_u16", "mixed_f32"])
def test_mixed_batch(engine, name):
    """Case 1.  Measured on an MI355X, largest relative error against the restatement: uint16 pixels 1.05e-15, float32 pixels
    1.15e-15, which is also the largest of every comparison of this file."""
    got = run(engine, name)
    assert np.isfinite(got).all() and len(got) == 8
    close(got, lr.expected(name), name)


def test_tile_border(engine):
    """Case 2: the "same" crop.  A kernel that took positions off the tile as candidates would return more for these objects,
    whose bright spots sit against the border."""
    close(run(engine, "border"), lr.expected("border"), "border")


def test_tiny_objects(engine):
    """Case 3: one pixel (0.0 exactly), a 1 x 3 line, a 2 x 2 block: hw = 1 and a filter that is nearly a delta."""
    got = run(engine, "tiny")
    assert got[0] == 0.0 and not np.signbit(got[0])
    close(got, lr.expected("tiny"), "tiny")


def test_zeros_inside_the_cell(engine):
    """Case 4: N counts the non-zero pixels, half the area here."""
    close(run(engine, "zeros_inside"), lr.expected("zeros_inside"), "zeros_inside")


def test_undefined_and_degenerate_cells(engine):
    """Case 5: all-zero object and absent label -> NaN, uniform object -> 0.0 exactly."""
    got = run(engine, "degenerate")
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0.0 and not np.signbit(got[2]) and np.isfinite(got[3])
    close(got, lr.expected("degenerate"), "degenerate")
    # with a given sigma the reference's filter for N == 0 is the 1 x 1 filter over J == 0: 0.0, and still NaN for the absent label
    given = run(engine, "degenerate", gaussian_sigma=1.5)
    assert given[0] == 0.0 and np.isnan(given[1])
    s = lr.scenes()["degenerate"]
    assert lr.nuc_est_conv(s["labels"][0] == 1, s["planes"][0, 0], gaussian_sigma=1.5) == 0.0


def test_neighbours_do_not_leak(engine):
    """Case 6: the dim object beside a neighbour 50 000 counts brighter equals, bit for bit, its value with the neighbour's
    pixels zeroed."""
    bright, zeroed = run(engine, "neighbours"), run(engine, "neighbours_zeroed")
    close(bright, lr.expected("neighbours"), "neighbours")
    close(zeroed, lr.expected("neighbours_zeroed"), "neighbours_zeroed")
    assert same_bits(bright[0], zeroed[0])


def test_keyword_forms(engine):
    """Case 7."""
    from aliby_amd.extraction import functions

    close(run(engine, "kw_alpha_ore"), lr.expected("kw_alpha_ore"), "alpha=0.9, object_radius_estimation=0.2")
    close(run(engine, "kw_sigma"), lr.expected("kw_sigma"), "gaussian_sigma=2.0")
    assert same_bits(run(engine, "mixed_u16", alpha=None, object_radius_estimation=None), run(engine, "mixed_u16"))  # None: the defaults
    s = lr.scenes()["border"]
    mask, image = s["labels"][0] == 1, np.array(s["planes"][0, 0])
    plain = functions.nuc_est_conv(mask, image)
    assert functions.nuc_est_conv(mask, image, gaussian_filter_shape=(3, 3)) == plain == run(engine, "border")[0]
    for alpha in (0.0, 1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            functions.nuc_est_conv(mask, image, alpha=alpha)
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            functions.nuc_est_conv(mask, image, gaussian_sigma=sigma)
    with pytest.raises(ValueError):
        functions.nuc_est_conv(mask, image, object_radius_estimation=0.0)


# --------------------------------------------------------------------------------------------------------------- cases 8 and 9
def _forms_of(name):
    s = lr.scenes()[name]
    X = s["labels"].shape[2]
    true = (0, 0, 0)
    for f, l in lr.rows(s):
        ys, xs = np.nonzero(s["labels"][f] == l)
        if len(ys):
            true = (max(true[0], int(ys.max() - ys.min() + 1)), max(true[1], int(xs.max() - xs.min() + 1)), max(true[2], len(ys)))
    return {rung: form(*(hint or true), X) for rung, hint in RUNGS[name].items()}


def test_rungs_reach_every_form():
    assert _forms_of("mixed_u16") == {"true": "attr", "64x64": "glob", "180x180": "glob"}
    assert _forms_of("border") == {"true": "lds", "40x40": "lds", "64x56": "attr", "100x100": "glob"}
    assert form(181, 181, 25445, 200) == "glob"  # the radius-90 disc, without hints


@pytest.mark.parametrize("name", ["mixed_u16", "mixed_f32", "border"])
def test_launch_forms_give_the_same_bits(engine, name):
    """Case 8: the same rows under hinted capacities, in every form the scene reaches."""
    base = run(engine, name)
    close(base, lr.expected(name), name)
    for rung, hint in RUNGS[name].items():
        assert same_bits(run(engine, name, hint), base), (name, rung)


def test_large_object_in_the_global_form(engine):
    """Case 8, the genuinely large object: a disc of radius 90 (hw = 53) in a 200 x 200 tile."""
    _, _, _, tab = device(engine, "disc90")
    assert form(tab.max_h, tab.max_w, tab.max_area, 200) == "glob"
    close(run(engine, "disc90"), lr.expected("disc90"), "disc90")


def test_batch_independence(engine):
    """Case 9: an object measured alone (one wave, LDS) and in a batch beside the radius-90 disc (256 threads, global scratch)."""
    import torch
    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    disc, small = lr.scenes()["disc90"], lr.scenes()["zeros_inside"]
    lab = np.zeros((2, 200, 200), np.uint16)
    px = np.zeros((2, 1, 200, 200), np.uint16)
    lab[0], px[0] = disc["labels"][0], disc["planes"][0]
    lab[1, 150:190, 3:43], px[1, 0, 150:190, 3:43] = small["labels"][0], small["planes"][0, 0]
    res = []
    for sel in (slice(1, 2), slice(0, 2)):
        dl = to_device_u16(lab[sel])
        dp, dt = to_device_planes(px[sel])
        tab = engine.object_table(dl)
        out = engine.new_output(tab.n_obj, 1)
        engine.nuc_est_conv(dl, dp, dt, 0, tab, out, 0)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy()[:, 0], form(tab.max_h, tab.max_w, tab.max_area, 200)))
    (alone, form_alone), (batch, form_batch) = res
    assert (form_alone, form_batch) == ("lds", "glob") and len(alone) == 1 and len(batch) == 2
    assert same_bits(alone[0], batch[1])
    close(batch, [lr.expected("disc90")[0], lr.nuc_est_conv(lab[1] == 1, px[1, 0])], "disc and small object")


def test_global_form_strides_over_600_objects(engine):
    """600 rows through at most 512 workgroups of the global form: the first 88 take a second object.  Against the LDS run."""
    import torch
    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    lab, px = stride_scene()
    dl = to_device_u16(lab)
    dp, dt = to_device_planes(px)
    tab = engine.object_table(dl)
    assert tab.n_obj == 600 and form(3, 3, 9, 128) == "lds" and form(100, 100, 8000, 128) == "glob"
    assert 512 * need_bytes(100, 100, 8000, 128) < 128 * KIB * KIB
    res = []
    for hint in (None, (100, 100, 8000)):
        out = engine.new_output(600, 1)
        engine.nuc_est_conv(dl, dp, dt, 1, hinted(tab, hint), out, 0)
        torch.cuda.synchronize()
        res.append(out.cpu().numpy()[:, 0])
    assert np.isfinite(res[0]).all() and same_bits(res[0], res[1])
    for k in (0, 299, 599):
        assert np.isclose(res[0][k], lr.nuc_est_conv(lab[0] == k + 1, px[0, 1]), rtol=1e-4, atol=1e-9)


# --------------------------------------------------------------------------------------------------------------------- case 10
@pytest.mark.parametrize("name", ["mixed_u16", "mixed_f32"])
def test_function_equals_the_batched_row(engine, name):
    from aliby_amd.extraction import functions

    s = lr.scenes()[name]
    batched = run(engine, name)
    for i in (0, 7):
        f, l = lr.rows(s)[i]
        assert functions.nuc_est_conv(s["labels"][f] == l, np.array(s["planes"][f, s["channel"]])) == batched[i]
    assert np.isnan(functions.nuc_est_conv(np.zeros((8, 8), bool), np.ones((8, 8), np.uint16)))  # an empty mask
    # a float64 image that holds uint16 values goes up as uint16
    f, l = lr.rows(s)[0]
    if name == "mixed_u16":
        assert functions.nuc_est_conv(s["labels"][f] == l, s["planes"][f, s["channel"]].astype(np.float64)) == batched[0]


def test_through_the_extraction_tree(engine):
    """One cell_metrics launch serves both nuc_est_conv (its median) and the `median` metric of the same (plane, channel)."""
    import torch
    from aliby_amd.extraction.engine import FeatureEngine
    from aliby_amd.extraction.extract import extract_tree, format_extraction, process_tree_masks

    s = lr.scenes()["mixed_u16"]
    masks = [np.array(s["labels"][f]) for f in range(2)]
    pixels = np.array(s["planes"])[:, :, None]  # [F,C,Z,Y,X]
    FeatureEngine(0).collect_profile()
    FeatureEngine.shared_profile = {}
    try:
        inst, res = process_tree_masks({1: {"max": ["nuc_est_conv", "median"]}}, masks, pixels, extract_tree)
        prof = FeatureEngine(0).collect_profile()
    finally:
        FeatureEngine.shared_profile = None
    assert prof["cell_metrics"]["launches"] == 1 and prof["nuc_est_conv"]["launches"] == 1, prof
    assert len(inst) == len(res) == 16 and inst[0] == ((0, 1), (1, "max", "nuc_est_conv"))
    direct = run(engine, "mixed_u16")
    dl, dp, dt, tab = device(engine, "mixed_u16")
    median = engine.cell_metrics(dl, dp, dt, 1, tab)[:, engine.CELL_COLUMNS.index("median")].cpu().numpy()
    torch.cuda.synchronize()
    assert all(isinstance(r, float) for r in res)
    assert same_bits([res[2 * i] for i in range(8)], direct) and same_bits([res[2 * i + 1] for i in range(8)], median)
    table = format_extraction((inst, res))
    assert same_bits(table["1/max/nuc_est_conv/nuc_est_conv"].to_numpy(), direct)
    with pytest.raises(Exception):  # no pixels of a channel to measure
        process_tree_masks({"None": {"None": ["nuc_est_conv"]}}, masks, pixels, extract_tree)


def test_run_positions_writes_the_column(tmp_path, engine):
    import pyarrow.parquet
    from aliby_amd import synth
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe_builder import build_pipeline_steps
    from tests.test_gpu_configs import _keyed_override

    fovs = [synth.make_fov(2, 70 + i, shape=(224, 256), n_channels=2, n_target=6) for i in range(2)]
    override = _keyed_override(fovs)
    pipes = []
    for f in fovs:
        p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[1], features_to_extract=("nuc_est_conv", "median"))
        p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
        p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
        pipes.append(p)
    names = ["N00__1", "N01__1"]
    got = run_positions(pipes, names, tmp_path, batch_size=2)
    col = "1/max/nuc_est_conv/nuc_est_conv"
    for (prof, _), nm, f in zip(got, names, fovs):
        on_disk = pyarrow.parquet.read_table(tmp_path / "profiles" / f"{nm}.parquet")
        assert col in on_disk.column_names and "1/max/median/median" in on_disk.column_names and prof.num_rows > 0
        with np.load(tmp_path / "steps" / nm / "segment_nuclei" / "0000.npz") as z:
            lab = z["arr_0"].reshape(224, 256)
        labels = prof["metadata_label"].to_numpy()
        want = [lr.nuc_est_conv(lab == l, f["pixels"][1].max(axis=0)) for l in labels]
        close(on_disk[col].to_numpy(), want, f"run_positions {nm}")
        assert same_bits(on_disk[col].to_numpy(), prof[col].to_numpy())
