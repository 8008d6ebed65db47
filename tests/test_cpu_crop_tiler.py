"""
The crop tiler without a GPU: tests/crop_tiler_ref.py, the NumPy restatement the GPU tests compare the kernels with, against what
the reference's own CropTiler returned on the same seeded scenes (tests/golden/reference_crop_tiler.npz, written by
tests/golden/make_crop_tiler_golden.py), and the parts of aliby_amd.tile.tiler.CropTiler that do not touch the device.

Integer results (uint16 / uint8) are equal.  pmin / pmax are bit-equal to np.percentile of the installed NumPy on every channel
of every scene (no exception found).  Float results: largest relative error over all scenes and combinations, with the absolute
floor 1.0 of crop_tiler_ref.rel_err, measured 4.48e-16 (exact_fit, clip_outliers + standard_scale; the restatement sums over the
histogram where np.mean / np.std sum over the voxels); asserted at ten times that.
"""
import warnings

import numpy as np
import pytest

from tests import crop_tiler_ref as cr

MEASURED = 4.48e-16
BOUND = 10 * MEASURED

_GOLDEN = {}


def golden():
    if not _GOLDEN:
        from pathlib import Path

        with np.load(Path(__file__).parent / "golden" / "reference_crop_tiler.npz") as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def test_golden_holds_every_scene_and_combination():
    want = {f"{n}/{cr.combo_name(*c)}" for n in cr.scenes() for c in cr.COMBOS}
    assert set(golden()) == want and len(want) == 8 * len(cr.scenes())
    assert golden()["oversized/clip0_bit0_std0"].shape == (0, 2, 1, 16, 16)
    assert golden()["ragged/clip0_bit0_std0"].shape == (6, 3, 2, 16, 16)  # 37 x 53 in 16s: 2 x 3, remainders dropped
    assert golden()["exact_fit/clip0_bit0_std0"].shape == (1, 1, 1, 24, 24)


@pytest.mark.parametrize("name", list(cr.scenes()))
def test_restatement_equals_the_reference(name):
    s = cr.scenes()[name]
    worst = 0.0
    for clip, bit8, std in cr.COMBOS:
        want = golden()[f"{name}/{cr.combo_name(clip, bit8, std)}"]
        got = cr.crop_tiles(s["pixels"], s["ts"], standard_scale=std, convert_8bit=bit8, clip_outliers=clip)
        assert got.shape == want.shape and got.dtype == want.dtype, (clip, bit8, std)
        assert got.dtype == cr.out_dtype(s["pixels"].dtype, clip, bit8, std)
        if got.dtype.kind == "f":
            assert cr.same_nonfinite(got, want), (clip, bit8, std)
            err = cr.rel_err(got, want)
            print(f"{name} {cr.combo_name(clip, bit8, std)}: largest relative error {err:.3e}")
            worst = max(worst, err)
        else:
            assert np.array_equal(got, want), (clip, bit8, std)
    assert worst <= BOUND


@pytest.mark.parametrize("name", list(cr.scenes()))
def test_percentiles_are_numpys(name):
    px = cr.scenes()[name]["pixels"]
    _, stats = cr.normalise(px, True, False, False)
    for c in range(px.shape[0]):
        assert stats[c, 0] == np.percentile(px[c], 0.5) and stats[c, 1] == np.percentile(px[c], 99.5), c
    _, stats = cr.normalise(px, True, False, False, clip_percent=0)
    assert np.array_equal(stats[:, 0], px.min(axis=(1, 2, 3))) and np.array_equal(stats[:, 1], px.max(axis=(1, 2, 3)))


def test_the_scenes_hold_what_they_are_for():
    sp = cr.scenes()["special"]["pixels"]
    assert sp[0].min() == 0 and sp[0].max() == 65535 and len(np.unique(sp[1])) == 1
    n = sp[2].size
    for c, (q, between, t_low) in {2: (0.5, True, True), 3: (99.5, True, False)}.items():
        index = (n - 1) * (q / 100)
        assert (index - np.floor(index) < 0.5) == t_low
        assert (100 < np.percentile(sp[c], q) < 900) == between
    # the constant channel: NaN in float results, 0 after the 8-bit cast
    g = golden()
    assert np.isnan(g["special/clip1_bit0_std0"][:, 1]).all() and np.isnan(g["special/clip0_bit0_std1"][:, 1]).all()
    assert (g["special/clip1_bit1_std0"][:, 1] == 0).all()
    # 8-bit without clip wraps: (255 v) mod 256
    rg = cr.scenes()["ragged"]["pixels"]
    assert np.array_equal(g["ragged/clip0_bit1_std0"][0, :, :, :, :], ((rg[:, :, :16, :16].astype(np.int64) * 255) % 256))


# ------------------------------------------------------------------------------------------------ the tiler, host side
def test_dispatch_returns_the_crop_tilers_constructor():
    from aliby_amd.io.image import ImageArray
    from aliby_amd.tile.tiler import CropTiler, dispatch_tiler

    px = cr.scenes()["ragged"]["pixels"][None]
    make = dispatch_tiler("crop", {"tile_size": 16})
    tiler = make(ImageArray(source=px))
    assert isinstance(tiler, CropTiler) and tiler.pixels is not None and tuple(tiler.pixels.shape) == px.shape
    assert (tiler.tile_size, tiler.standard_scale, tiler.convert_8bit, tiler.clip_outliers) == (16, True, False, False)
    assert tiler.float_source and not tiler.eight_bit and tiler.n_tiles() == (2, 3)
    assert not hasattr(tiler, "tile_locs")
    for attr in ("from_image", "get_fczyx", "run_tp", "_run_tp", "get_fczyx_device", "run_tp_device"):
        assert callable(getattr(tiler, attr))


def test_other_kinds_still_give_the_tiler():
    from aliby_amd.io.image import ImageArray
    from aliby_amd.tile.tiler import Tiler, dispatch_tiler

    px = cr.scenes()["ragged"]["pixels"][None]
    for kind in (None, "tiler", "anything"):
        assert isinstance(dispatch_tiler(kind, {"tile_size": None})(ImageArray(source=px)), Tiler)


def test_kwargs_are_swallowed_and_modes_marked():
    from aliby_amd.io.image import ImageArray
    from aliby_amd.tile.tiler import dispatch_tiler

    img = ImageArray(source=cr.scenes()["ragged"]["pixels"][None])
    raw = dispatch_tiler("crop", {"tile_size": 16, "ref_channel": 1, "ref_z": 0, "track_drift": False, "calculate_drift": True,
                                  "standard_scale": False, "no_such_option": 3})(img)
    assert not raw.float_source and not raw.eight_bit and raw.flags == 0 and not hasattr(raw, "calculate_drift")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # clip + 8-bit does not wrap: no warning
        eight = dispatch_tiler("crop", {"tile_size": 16, "standard_scale": False, "convert_8bit": True, "clip_outliers": True})(img)
    assert eight.eight_bit and not eight.float_source and eight.flags == 3
    img8 = ImageArray(source=cr.scenes()["eight_bit"]["pixels"][None])
    assert dispatch_tiler("crop", {"tile_size": 8, "standard_scale": False})(img8).eight_bit


def test_eight_bit_without_clip_warns_of_the_wrap():
    from aliby_amd.tile.tiler import CropTiler

    with pytest.warns(UserWarning, match="mod 256"):
        CropTiler(cr.scenes()["ragged"]["pixels"][None], 16, standard_scale=False, convert_8bit=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_sources_without_a_histogram_are_refused(dtype):
    from aliby_amd.tile.tiler import CropTiler

    with pytest.raises(NotImplementedError, match="histogram"):
        CropTiler(np.zeros((1, 1, 1, 16, 16), dtype), 16)
