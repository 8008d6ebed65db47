"""
nuc_conv_3d on the GPU (k_nuc3d of aliby_amd/csrc/feat_localisation.hip) against tests/localisation3d_ref.py, the float64
restatement that tests/test_cpu_localisation3d_ref.py pins to the reference's own function, through every layer: the engine call
in each launch form, functions.nuc_conv_3d, the extraction tree and run_positions.

Pass bar: rtol 1e-4, atol 1e-9, NaN equal to NaN; 0.0 and bit-equality where a case states them.  Every comparison prints its
largest relative error first.  Measured on an MI355X, largest relative error against the restatement over every comparison of
this file: uint16 voxels 2.46e-15 (the mixed batch with pixel_size = z_spacing = 0.5), float32 voxels 1.57e-15 (the mixed batch).

Launch forms, restated from the header of feat_localisation.hip (hw = ceil(2 sqrt(0.085 max_area Z / pi)), wd = min(X, max_w + 2 hw)):

    need = r16(8 (max_h wd + max_h max_w + 2 (2 hw + 1)) + 4 Z max_h max_w)     LDS up to 64 KiB, the attribute raised above 32 KiB,
                                                                                 else global

The mixed batch (case 1) holds a 48 x 49 object of 1957 pixels on three planes: 84 752 bytes, so its true limits are already the
global form, and no hint, which may only grow a capacity, brings it back.  Its rungs are glob / glob with different slabs; the
corner scene (objects of 12 x 12, five planes) runs lds / attr / attr / glob, as uint16 and as float32, and each scene's rows are
bit-equal across its rungs.  Every other scene runs in plain LDS at its true limits, except the radius-40 disc (glob).
"""
import math

import numpy as np
import pytest

from tests import localisation3d_ref as lr
from tests.test_gpu_object_forms import hinted, stride_scene

pytestmark = pytest.mark.gpu

KIB = 1024
RUNGS = {
    "mixed_u16": {"true": None, "64x64": (64, 64, 4096)},
    "corner": {"true": None, "30x30": (30, 30, 900), "40x40": (40, 40, 1600), "48x56": (48, 56, 2600)},
}
RUNGS["mixed_f32"] = RUNGS["mixed_u16"]
RUNGS["corner_f32"] = RUNGS["corner"]


def need_bytes(h, w, a, Z, X):
    hw = math.ceil(2.0 * math.sqrt(0.085 * a * Z / math.pi))
    wd = min(X, w + 2 * hw)
    return (8 * (h * wd + h * w + 2 * (2 * hw + 1)) + 4 * Z * h * w + 15) // 16 * 16


def form(h, w, a, Z, X):
    need = need_bytes(h, w, a, Z, X)
    return "glob" if need > 64 * KIB else ("attr" if need > 32 * KIB else "lds")


def form_of(tab, stack):
    return form(tab.max_h, tab.max_w, tab.max_area, stack.shape[2], stack.shape[4])


_DEVICE = {}


def upload(engine, labels, stack):
    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    dl = to_device_u16(np.array(labels))
    dp, dt = to_device_planes(np.array(stack))
    return dl, dp, dt, engine.object_table(dl)


def device(engine, name):
    """-> (labels, stack, dtype code, object table) of a scene on the GPU, made once"""
    if name not in _DEVICE:
        s = lr.scenes()[name]
        _DEVICE[name] = upload(engine, s["labels"], s["stack"])
        assert _DEVICE[name][3].n_obj == len(lr.rows(s))
    return _DEVICE[name]


def launch(engine, dl, dp, dt, tab, channel=0, **kw):
    import torch

    out = engine.new_output(tab.n_obj, 3)
    assert engine.nuc_conv_3d(dl, dp, dt, channel, tab, out, 1, **kw) == 1
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 2]).all()  # only column col0 is written
    return got[:, 1].copy()


def run(engine, name, hint=None, **override):
    s = lr.scenes()[name]
    dl, dp, dt, tab = device(engine, name)
    return launch(engine, dl, dp, dt, hinted(tab, hint), s["channel"], **dict(s["kwargs"], **override))


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


def true_form(engine, name):
    _, dp, _, tab = device(engine, name)
    return form_of(tab, dp)


# ------------------------------------------------------------------------------------------------------------------- cases 1-8
@pytest.mark.parametrize("name", ["mixed_u16", "mixed_f32"])
def test_mixed_batch(engine, name):
    """Case 1.  Measured on an MI355X, largest relative error against the restatement: 1.57e-15 for uint16 and for float32
    voxels, both in the global form."""
    got = run(engine, name)
    assert np.isfinite(got).all() and len(got) == 8 and true_form(engine, name) == "glob"
    close(got, lr.expected(name), name)


def test_corner_objects(engine):
    """Case 2: the "same" crop on Y and X.  A kernel that took positions off the tile as candidates would return more for these
    objects, whose bright spots sit against the corners on the first and the last plane."""
    assert true_form(engine, "corner") == "lds"
    close(run(engine, "corner"), lr.expected("corner"), "corner")


@pytest.mark.parametrize("name", ["tiny_z1", "tiny_z9"])
def test_tiny_objects(engine, name):
    """Case 3: 1, 3 and 4 pixels.  On one plane the single voxel gives 0.0 exactly; on nine planes hw = 1 .. 2, the z taps end
    before the stack does."""
    got = run(engine, name)
    assert true_form(engine, name) == "lds"
    if name == "tiny_z1":
        assert got[0] == 0.0 and not np.signbit(got[0])
    close(got, lr.expected(name), name)


@pytest.mark.parametrize("name", ["fill", "fill_f32"])
def test_object_that_fills_the_tile(engine, name):
    """Case 4: the dilated box covers the whole 12 x 12 x 2 stack, so no 0 from outside takes part in the maximum.  The object has
    262 voxels: as float32 its median is the float32 mean of the two middle values, selected in LDS."""
    assert true_form(engine, name) == "lds"
    close(run(engine, name), lr.expected(name), name)


def test_zeros_inside_the_cell(engine):
    """Case 5: N counts the non-zero voxels: alternate columns of alternate planes are 0."""
    assert true_form(engine, "zeros_inside") == "lds"
    close(run(engine, "zeros_inside"), lr.expected("zeros_inside"), "zeros_inside")


def test_undefined_and_degenerate_cells(engine):
    """Case 6: all-zero object and absent label -> NaN, uniform object -> 0.0 exactly, an ordinary blob."""
    got = run(engine, "degenerate")
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0.0 and not np.signbit(got[2]) and np.isfinite(got[3])
    close(got, lr.expected("degenerate"), "degenerate")


def test_neighbours_do_not_leak(engine):
    """Case 7: the dim object beside a neighbour 50 000 counts brighter equals, bit for bit, its value with the neighbour's
    voxels zeroed and its value alone in the tile."""
    bright, zeroed, alone = run(engine, "neighbours"), run(engine, "neighbours_zeroed"), run(engine, "neighbours_alone")
    close(bright, lr.expected("neighbours"), "neighbours")
    close(zeroed, lr.expected("neighbours_zeroed"), "neighbours_zeroed")
    close(alone, lr.expected("neighbours_alone"), "neighbours_alone")
    assert np.isnan(zeroed[1]) and len(alone) == 1
    assert same_bits(bright[0], zeroed[0]) and same_bits(bright[0], alone[0])


@pytest.mark.parametrize("name", ["kw_flat", "kw_cubic"])
def test_pixel_size_and_z_spacing(engine, name):
    """Case 8: (0.1, 1.0) and (0.5, 0.5) on the mixed batch; only their quotient enters."""
    got = run(engine, name)
    close(got, lr.expected(name), name)
    assert not same_bits(got, run(engine, "mixed_u16"))
    kw = lr.scenes()[name]["kwargs"]
    assert same_bits(got, run(engine, "mixed_u16", pixel_size=2 * kw["pixel_size"], z_spacing=2 * kw["z_spacing"]))


def test_argument_checks(engine):
    dl, dp, dt, tab = device(engine, "corner")
    for kw in (dict(pixel_size=0.0), dict(pixel_size=-1.0), dict(z_spacing=0.0), dict(z_spacing=float("inf")), dict(pixel_size=float("nan"))):
        with pytest.raises(ValueError):
            launch(engine, dl, dp, dt, tab, **kw)
    with pytest.raises(ValueError):
        launch(engine, dl, dp, dt, tab, channel=1)  # the scene has one channel
    with pytest.raises(ValueError):
        engine.nuc_conv_3d(dl, dp[:, :, 0], dt, 0, tab, engine.new_output(tab.n_obj, 1), 0)  # a reduced plane is not a stack
    with pytest.raises(ValueError):
        engine.nuc_conv_3d(dl, dp, dt, 0, tab, engine.new_output(tab.n_obj, 1), 1)  # column past the row
    with pytest.raises(ValueError):
        engine.nuc_conv_3d(dl, dp[:, :, :0], dt, 0, tab, engine.new_output(tab.n_obj, 1), 0)  # Z = 0: no plane
    with pytest.raises(ValueError):
        engine.nuc_conv_3d(dl, dp, 7, 0, tab, engine.new_output(tab.n_obj, 1), 0)  # neither uint16 nor float32


# -------------------------------------------------------------------------------------------------------------- cases 9 to 12
def _forms_of(name):
    s = lr.scenes()[name]
    Z, X = s["stack"].shape[2], s["stack"].shape[4]
    true = (0, 0, 0)
    for f, l in lr.rows(s):
        ys, xs = np.nonzero(s["labels"][f] == l)
        if len(ys):
            true = (max(true[0], int(ys.max() - ys.min() + 1)), max(true[1], int(xs.max() - xs.min() + 1)), max(true[2], len(ys)))
    return {rung: form(*(hint or true), Z, X) for rung, hint in RUNGS[name].items()}


def test_rungs_reach_every_form():
    assert _forms_of("mixed_u16") == {"true": "glob", "64x64": "glob"}
    assert _forms_of("corner") == _forms_of("corner_f32") == {"true": "lds", "30x30": "attr", "40x40": "attr", "48x56": "glob"}
    assert need_bytes(40, 40, 1600, 5, 56) > 60 * KIB  # the upper attr rung sits just under the budget
    assert form(81, 81, 5025, 5, 120) == "glob"  # the radius-40 disc, without hints


def test_large_object_in_the_global_form(engine):
    """Case 9: a disc of radius 40 on five planes (25 125 voxels, hw = 53) in a 120 x 120 tile."""
    _, dp, _, tab = device(engine, "disc40")
    assert (tab.max_h, tab.max_w, tab.max_area) == (81, 81, 5025) and form_of(tab, dp) == "glob"
    close(run(engine, "disc40"), lr.expected("disc40"), "disc40")


@pytest.mark.parametrize("name", ["mixed_u16", "mixed_f32", "corner", "corner_f32"])
def test_launch_forms_give_the_same_bits(engine, name):
    """Case 10: the same rows under hinted capacities, in every form the scene reaches."""
    base = run(engine, name)
    close(base, lr.expected(name), name)
    for rung, hint in RUNGS[name].items():
        assert same_bits(run(engine, name, hint), base), (name, rung)


def _small_object():
    """a 95-pixel ellipse on five planes, with a spot: one wave's worth of work"""
    shape = (5, 24, 28)
    lab = lr._ellipse(shape[1:], 11, 14, 5.0, 6.0).astype(np.uint16)
    return lab, (lr._noise(41, shape) + lr._spot(shape, 2, 9, 16, 1.5, 3000)).astype(np.uint16)


def test_batch_independence(engine):
    """Case 11: an object measured alone (one wave, LDS) and in a batch beside the radius-40 disc (256 threads, global scratch)."""
    disc = lr.scenes()["disc40"]
    small_lab, small_px = _small_object()
    lab = np.zeros((2, 120, 120), np.uint16)
    px = np.zeros((2, 1, 5, 120, 120), np.uint16)
    lab[0], px[0] = disc["labels"][0], disc["stack"][0]
    lab[1, 90:114, 3:31], px[1, 0, :, 90:114, 3:31] = small_lab, small_px
    res = []
    for sel in (slice(1, 2), slice(0, 2)):
        dl, dp, dt, tab = upload(engine, lab[sel], px[sel])
        hw = math.ceil(2.0 * math.sqrt(0.085 * tab.max_area * 5 / math.pi))
        res.append((launch(engine, dl, dp, dt, tab), form_of(tab, dp), min(120, tab.max_h + 2 * hw) * min(120, tab.max_w + 2 * hw)))
    (alone, form_alone, work_alone), (batch, form_batch, work_batch) = res
    assert (form_alone, form_batch) == ("lds", "glob") and len(alone) == 1 and len(batch) == 2
    assert work_alone <= 2048 < 8192 < work_batch  # one wave alone (the workgroup size rule of the LDS form); 256 threads in the batch
    assert same_bits(alone[0], batch[1])
    close(batch, [lr.expected("disc40")[0], lr.nuc_conv_3d(lab[1] == 1, px[1, 0])], "disc and small object")


def test_global_form_strides_over_600_objects(engine):
    """Case 12: 600 rows through at most 512 workgroups of the global form, two channels of the scene taken as a Z = 2 stack: the
    first 88 workgroups take a second object.  Against the LDS run."""
    lab, px = stride_scene()
    stack = px[:, None]  # [1, 1, 2, 128, 128]
    dl, dp, dt, tab = upload(engine, lab, stack)
    assert tab.n_obj == 600 and form(3, 3, 9, 2, 128) == "lds" and form(64, 64, 4096, 2, 128) == "glob"
    assert 512 * need_bytes(64, 64, 4096, 2, 128) < 128 * KIB * KIB
    res = [launch(engine, dl, dp, dt, hinted(tab, hint)) for hint in (None, (64, 64, 4096))]
    assert np.isfinite(res[0]).all() and same_bits(res[0], res[1])
    ks = (0, 299, 599)
    close(res[0][list(ks)], [lr.nuc_conv_3d(lab[0] == k + 1, stack[0, 0]) for k in ks], "stride scene rows 0, 299, 599")


# --------------------------------------------------------------------------------------------------------- cases 13, 14 and 15
@pytest.mark.parametrize("name", ["mixed_u16", "mixed_f32"])
def test_function_equals_the_batched_row(engine, name):
    from aliby_amd.extraction import functions

    s = lr.scenes()[name]
    batched = run(engine, name)
    for i in (0, 7):
        f, l = lr.rows(s)[i]
        assert functions.nuc_conv_3d(s["labels"][f] == l, np.array(s["stack"][f, s["channel"]])) == batched[i]
    assert np.isnan(functions.nuc_conv_3d(np.zeros((8, 8), bool), np.ones((3, 8, 8), np.uint16)))  # an empty mask
    f, l = lr.rows(s)[0]
    with pytest.raises(ValueError):
        functions.nuc_conv_3d(s["labels"][f] == l, np.array(s["stack"][f, s["channel"], 0]))  # a 2-D image
    with pytest.raises(ValueError):
        functions.nuc_conv_3d(s["labels"][f] == l, np.array(s["stack"][f]))  # [C,Z,Y,X]
    if name == "mixed_u16":
        # a float64 stack that holds uint16 values goes up as uint16
        assert functions.nuc_conv_3d(s["labels"][f] == l, s["stack"][f, s["channel"]].astype(np.float64)) == batched[0]
        kw = lr.scenes()["kw_flat"]["kwargs"]
        assert functions.nuc_conv_3d(s["labels"][f] == l, np.array(s["stack"][f, s["channel"]]), **kw) == run(engine, "kw_flat")[0]


def test_through_the_extraction_tree(engine):
    """Case 14: the stack metric under the reducer key "None" beside plane metrics under "max" of the same channel."""
    import torch
    from aliby_amd.extraction.engine import FeatureEngine
    from aliby_amd.extraction.extract import extract_tree, format_extraction, process_tree_masks
    from aliby_amd.extraction.families import PlaneCache

    s = lr.scenes()["mixed_u16"]
    masks = [np.array(s["labels"][f]) for f in range(2)]
    pixels = np.array(s["stack"])  # [F,C,Z,Y,X], Z = 3
    tree = {1: {"None": ["nuc_conv_3d"], "max": ["nuc_est_conv", "median"]}}
    FeatureEngine(0).collect_profile()
    FeatureEngine.shared_profile = {}
    try:
        inst, res = process_tree_masks(tree, masks, pixels, extract_tree, cp_measure_kwargs={"nuc_conv_3d": {"pixel_size": 0.1}})
        prof = FeatureEngine(0).collect_profile()
    finally:
        FeatureEngine.shared_profile = None
    assert prof["nuc_conv_3d"]["launches"] == 1 and prof["cell_metrics"]["launches"] == 1 and prof["nuc_est_conv"]["launches"] == 1, prof
    assert len(inst) == len(res) == 24 and inst[0] == ((0, 1), (1, "None", "nuc_conv_3d"))
    direct = run(engine, "mixed_u16")  # the defaults: the cp_measure_kwargs entry of an in-repo function is not looked at
    dl, dp, dt, tab = device(engine, "mixed_u16")
    plane, pdt = PlaneCache(engine, (dp, dt)).get("max")
    cell = engine.cell_metrics(dl, plane, pdt, 1, tab)
    median = cell[:, engine.CELL_COLUMNS.index("median")]
    out = engine.new_output(tab.n_obj, 1)
    engine.nuc_est_conv(dl, plane, pdt, 1, tab, out, 0, median=median)
    torch.cuda.synchronize()
    assert all(isinstance(r, float) for r in res)
    assert same_bits([res[3 * i] for i in range(8)], direct)
    assert same_bits([res[3 * i + 1] for i in range(8)], out.cpu().numpy()[:, 0])
    assert same_bits([res[3 * i + 2] for i in range(8)], median.cpu().numpy())
    table = format_extraction((inst, res))
    assert {"1/None/nuc_conv_3d/nuc_conv_3d", "1/max/nuc_est_conv/nuc_est_conv", "1/max/median/median"} <= set(table.column_names)
    assert same_bits(table["1/None/nuc_conv_3d/nuc_conv_3d"].to_numpy(), direct)
    for bad in ({1: {"max": ["nuc_conv_3d"]}}, {1: {"add": ["nuc_conv_3d"]}}, {1: {"div": ["nuc_conv_3d"]}}, {"None": {"None": ["nuc_conv_3d"]}}):
        with pytest.raises(Exception, match="un-reduced stack"):
            process_tree_masks(bad, masks, pixels, extract_tree)
    with pytest.raises(Exception, match="invalid reducer"):  # every other metric under "None" with a channel, as before
        process_tree_masks({1: {"None": ["intensity"]}}, masks, pixels, extract_tree)
    with pytest.raises(Exception, match="invalid reducer"):
        process_tree_masks({1: {"None": ["nuc_conv_3d", "median"]}}, masks, pixels, extract_tree)


def test_run_positions_writes_the_column(tmp_path, engine):
    """Case 15."""
    import pyarrow.parquet
    from aliby_amd import synth
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe_builder import build_pipeline_steps
    from tests.test_gpu_configs import _keyed_override

    fovs = [synth.make_fov(2, 70 + i, shape=(224, 256), n_channels=2, n_z=3, n_target=6) for i in range(2)]
    override = _keyed_override(fovs)
    pipes = []
    for f in fovs:
        p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[1], features_to_extract=("median",))
        p["steps"]["extract_nuclei"]["tree"][1] = {"None": ["nuc_conv_3d"], "max": ["median"]}
        p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
        p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
        pipes.append(p)
    names = ["N00__1", "N01__1"]
    got = run_positions(pipes, names, tmp_path, batch_size=2)
    col = "1/None/nuc_conv_3d/nuc_conv_3d"
    for (prof, _), nm, f in zip(got, names, fovs):
        on_disk = pyarrow.parquet.read_table(tmp_path / "profiles" / f"{nm}.parquet")
        assert col in on_disk.column_names and "1/max/median/median" in on_disk.column_names and prof.num_rows > 0
        with np.load(tmp_path / "steps" / nm / "segment_nuclei" / "0000.npz") as z:
            lab = z["arr_0"].reshape(224, 256)
        labels = prof["metadata_label"].to_numpy()
        want = [lr.nuc_conv_3d(lab == l, f["pixels"][1]) for l in labels]
        close(on_disk[col].to_numpy(), want, f"run_positions {nm}")
        assert same_bits(on_disk[col].to_numpy(), prof[col].to_numpy())
