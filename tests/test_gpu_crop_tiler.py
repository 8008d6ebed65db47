"""
The crop tiler on the GPU (aliby_amd/csrc/tile_crop.hip; aliby_amd.tile.tiler.CropTiler) against tests/crop_tiler_ref.py, the
NumPy restatement that tests/test_cpu_crop_tiler.py pins to the reference's own CropTiler: through the C ABI on every scene and
every on/off combination of clip_outliers / convert_8bit / standard_scale, then through CropTiler, run_pipeline_and_post and
run_positions.

Integer outputs are exact, float32 tiles are the float64 tiles rounded once, NaN positions coincide.  Float64 tiles and the [C,4]
statistics: largest relative error (crop_tiler_ref.rel_err, absolute floor 1.0) against the restatement over every comparison of
this file, each printed before it is asserted at ten times the measured value:

    restatement against the reference (tests/test_cpu_crop_tiler.py)    4.48e-16
    kernels against the restatement, measured on an MI355X              6.58e-16 (KERNEL_MEASURED)

Launch geometry, restated from tile_crop.hip: the histogram runs min(64, CUs / 2C) slices of 1024 threads x 8 pixels per
(channel, role) and strides beyond; the tile pass runs at most 64 workgroups of 256 threads per (tile, plane), one item = 8 pixels
on the 16-byte path (ts and X multiples of 8), one pixel otherwise.  The 2048 x 2048 frame passes both caps: 4 194 304 pixels >
64 x 8192, ts = 512 gives 32 768 groups > 16 384, ts = 500 gives 250 000 pixels > 16 384.
"""
import numpy as np
import pytest

from tests import crop_tiler_ref as cr

pytestmark = pytest.mark.gpu

KERNEL_MEASURED = 6.58e-16  # CropTiler ragged, clip_outliers + standard_scale
BOUND = 10 * KERNEL_MEASURED

U16, F32, F64 = 0, 1, 3


def flags_of(clip, bit8, std):
    return (1 if clip else 0) | (2 if bit8 else 0) | (4 if std else 0)


def is_float(clip, bit8, std):
    return bool(std or (clip and not bit8))


_DEVICE = {}


def on_device(key, pixels):
    import torch

    if key not in _DEVICE:
        _DEVICE[key] = torch.from_numpy(np.ascontiguousarray(pixels).astype(np.uint16)).cuda()
    return _DEVICE[key]


def n_tiles(shape, ts):
    Y, X = shape[-2:]
    return ((Y - ts) // ts + 1 if Y >= ts else 0) * ((X - ts) // ts + 1 if X >= ts else 0)


def launch(engine, dev, ts, flags, code, clip=cr.CLIP):
    """aliby_crop_tiles_u16 -> (tiles, stats [C,4]) as NumPy arrays"""
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    C, Z, Y, X = dev.shape
    out = torch.zeros((n_tiles(dev.shape, ts), C, Z, ts, ts), dtype={U16: torch.uint16, F32: torch.float32, F64: torch.float64}[code],
                      device="cuda")
    stats = torch.full((C, 4), -1.0, dtype=torch.float64, device="cuda")
    _lib.check(engine.lib.aliby_crop_tiles_u16(engine.ctx.handle, _ptr(dev), C, Z, Y, X, ts, flags, clip, _ptr(out), code, _ptr(stats),
                                               _stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy()


def histogram(engine, dev):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    C = dev.shape[0]
    hist = torch.full((C, 65536), 7, dtype=torch.int32, device="cuda")  # (stale counts: the call zeroes them)
    _lib.check(engine.lib.aliby_crop_hist_u16(engine.ctx.handle, _ptr(dev), C, dev[0].numel(), _ptr(hist), _stream_ptr()))
    torch.cuda.synchronize()
    return hist.cpu().numpy().view(np.uint32)


def close(got, want, what):
    assert got.shape == want.shape, what
    assert cr.same_nonfinite(got, want), f"{what}: NaN / inf positions differ"
    err = cr.rel_err(got, want)
    print(f"{what}: largest relative error {err:.3e}")
    assert err <= BOUND, what
    return err


_WANT = {}


def want_of(name, combo):
    """the restatement's (tiles, stats) of a scene and combination, computed once"""
    if (name, combo) not in _WANT:
        s = cr.scenes()[name]
        frame, stats = cr.normalise(s["pixels"], *combo)
        _WANT[name, combo] = (cr.cut(frame, s["ts"]), stats)
    return _WANT[name, combo]


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", list(cr.scenes()))
def test_every_combination_against_the_restatement(engine, name):
    s = cr.scenes()[name]
    dev = on_device(name, s["pixels"])
    for combo in cr.COMBOS:
        what = f"{name} {cr.combo_name(*combo)}"
        want, want_stats = want_of(name, combo)
        flags = flags_of(*combo)
        if not is_float(*combo):
            got, stats = launch(engine, dev, s["ts"], flags, U16)
            assert got.shape == want.shape and np.array_equal(got, want.astype(np.uint16)), what
        else:
            got, stats = launch(engine, dev, s["ts"], flags, F64)
            close(got, want, what)
            got32, stats32 = launch(engine, dev, s["ts"], flags, F32)
            assert np.array_equal(got32, got.astype(np.float32), equal_nan=True), what
            assert np.array_equal(stats32, stats, equal_nan=True), what
        if want.shape[0] == 0:
            assert (stats == -1.0).all()  # no tile: no launch, nothing written
        elif flags & 5:
            assert np.array_equal(np.isnan(stats), np.isnan(want_stats)), what
            close(stats, want_stats, what + " statistics")
            if combo[0]:  # the percentiles are NumPy's own, bit for bit
                assert np.array_equal(stats[:, :2], want_stats[:, :2]), what


def test_min_max_when_clip_is_not_positive(engine):
    s = cr.scenes()["ragged"]
    dev = on_device("ragged", s["pixels"])
    frame, want_stats = cr.normalise(s["pixels"], True, False, False, clip_percent=0)
    got, stats = launch(engine, dev, s["ts"], 1, F64, clip=0.0)
    assert np.array_equal(stats[:, :2], want_stats[:, :2]) and np.isnan(stats[:, 2:]).all()
    close(got, cr.cut(frame, s["ts"]), "ragged, clip = 0")
    assert got.min() == 0.0 and got.max() <= 1.0


def test_argument_checks(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    dev = on_device("ragged", cr.scenes()["ragged"]["pixels"])
    C, Z, Y, X = dev.shape
    out = torch.zeros((6, C, Z, 16, 16), dtype=torch.float64, device="cuda")

    def call(flags, code, ts=16, clip=0.5):
        _lib.check(engine.lib.aliby_crop_tiles_u16(engine.ctx.handle, _ptr(dev), C, Z, Y, X, ts, flags, clip, _ptr(out), code, None,
                                                   _stream_ptr()))

    for flags, code in ((0, F64), (2, F32), (3, F64), (4, U16), (1, U16), (8, U16)):
        with pytest.raises(ValueError):
            call(flags, code)
    with pytest.raises(ValueError):
        call(0, U16, ts=0)
    with pytest.raises(ValueError):
        call(5, F64, clip=50.0)
    with pytest.raises(ValueError):  # Z*Y*X of 2^32 voxels: the 32-bit bins could overflow (checked before anything is read)
        _lib.check(engine.lib.aliby_crop_hist_u16(engine.ctx.handle, _ptr(dev), 1, 1 << 32, _ptr(out), _stream_ptr()))
    call(5, F64)  # (stats_out may be NULL)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ bits
def test_the_same_frame_twice_gives_the_same_bytes(engine):
    s = cr.scenes()["ragged"]
    dev = on_device("ragged", s["pixels"])
    for flags, code in ((5, F64), (7, F32), (3, U16)):
        a, sa = launch(engine, dev, s["ts"], flags, code)
        b, sb = launch(engine, dev, s["ts"], flags, code)
        assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
    assert histogram(engine, dev).tobytes() == histogram(engine, dev).tobytes()


def test_tile_size_does_not_change_a_pixel(engine):
    """Normalisation is whole-frame: tiles of 16 and of 32 hold the same values where both cover the frame (64 x 96: all of it)."""
    s = cr.scenes()["vector"]
    dev = on_device("vector", s["pixels"])
    C, Z, Y, X = s["pixels"].shape

    def frame_of(tiles, ts):
        out = np.empty((C, Z, Y, X), tiles.dtype)
        n_tw = X // ts
        for t in range(tiles.shape[0]):
            i, j = divmod(t, n_tw)
            out[:, :, i * ts:(i + 1) * ts, j * ts:(j + 1) * ts] = tiles[t]
        return out

    for flags, code in ((5, F64), (5, F32), (3, U16), (0, U16)):
        a, b = launch(engine, dev, 16, flags, code)[0], launch(engine, dev, 32, flags, code)[0]
        assert a.shape[0] == 24 and b.shape[0] == 6
        assert frame_of(a, 16).tobytes() == frame_of(b, 32).tobytes()


@pytest.mark.parametrize("name", ["ragged", "special", "eight_bit"])
def test_histogram_equals_bincount(engine, name):
    """ragged: 3922 voxels per channel, so channel 1 starts off a 16-byte boundary (pixel by pixel) and channels 0 and 2 end in
    a two-pixel tail; special: both halves of the grey range, i.e. both workgroup roles."""
    px = cr.scenes()[name]["pixels"]
    got = histogram(engine, on_device(name, px))
    assert got.dtype == np.uint32 and np.array_equal(got, np.stack([cr.histogram(px[c]) for c in range(px.shape[0])]))


# ------------------------------------------------------------------------------------------------ past the grid caps
def _large():
    if "large" not in _WANT:
        rng = np.random.default_rng(77)
        px = (200 + rng.integers(0, 3000, (1, 1, 2048, 2048))).astype(np.uint16)
        px[0, 0, 5, 7], px[0, 0, 2000, 2047] = 40000, 65535  # (the upper half of the grey range is not empty)
        _WANT["large"] = px
    return _WANT["large"]


def test_large_frame_histogram(engine):
    px = _large()
    assert px[0].size > 64 * 1024 * 8
    assert np.array_equal(histogram(engine, on_device("large", px))[0], cr.histogram(px[0]))


def test_large_frame_tiles(engine):
    px = _large()
    dev = on_device("large", px)
    assert 512 * 512 // 8 > 64 * 256 and 500 * 500 > 64 * 256
    frame, want_stats = cr.normalise(px, True, False, True)
    got, stats = launch(engine, dev, 512, 5, F64)  # 16-byte path
    close(got, cr.cut(frame, 512), "large, ts 512")
    close(stats, want_stats, "large statistics")
    wide, _ = launch(engine, dev, 500, 5, F64)  # pixel by pixel
    close(wide, cr.cut(frame, 500), "large, ts 500")
    got32, _ = launch(engine, dev, 500, 5, F32)
    assert np.array_equal(got32, wide.astype(np.float32))
    for ts in (512, 500):
        raw, _ = launch(engine, dev, ts, 0, U16)
        assert np.array_equal(raw, cr.cut(px, ts))
    eight, _ = launch(engine, dev, 500, 3, U16)
    assert np.array_equal(eight, cr.cut(cr.normalise(px, True, True, False)[0], 500))


# ------------------------------------------------------------------------------------------------ CropTiler
def _tiler(pixels, ts, combo):
    import warnings

    from aliby_amd.io.image import ImageArray
    from aliby_amd.tile.tiler import dispatch_tiler

    clip, bit8, std = combo
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (8-bit without clip warns of the wrap: tests/test_cpu_crop_tiler.py)
        return dispatch_tiler("crop", {"tile_size": ts, "standard_scale": std, "convert_8bit": bit8, "clip_outliers": clip})(
            ImageArray(source=pixels[None]))


@pytest.mark.parametrize("name", ["ragged", "eight_bit", "oversized"])
def test_crop_tiler_on_an_image(engine, name):
    import torch

    from aliby_amd import devcache

    s = cr.scenes()[name]
    for combo in cr.COMBOS:
        what = f"CropTiler {name} {cr.combo_name(*combo)}"
        want, _ = want_of(name, combo)
        tiler = _tiler(s["pixels"], s["ts"], combo)
        host = tiler.get_fczyx(0)
        assert host.dtype == want.dtype and host.shape == want.shape, what
        if host.dtype.kind == "f":
            close(host, want, what)
        else:
            assert np.array_equal(host, want), what
        dev, meta = devcache.lookup(host)
        if host.dtype.kind == "f":
            assert dev.dtype == torch.float32 and tiler.float_source and not tiler.eight_bit
            assert np.array_equal(dev.cpu().numpy(), host.astype(np.float32), equal_nan=True), what
        else:
            assert dev.dtype == torch.uint16 and not tiler.float_source
            assert meta["eight_bit"] == tiler.eight_bit == (host.dtype == np.uint8)
            assert np.array_equal(dev.cpu().numpy(), host.astype(np.uint16)), what
        block, flags = tiler.get_fczyx_device(0)
        assert block is dev and flags.shape == (want.shape[0],) and not flags.any()
        step = tiler.run_tp(0)
        assert list(step) == ["pixels"] and step["pixels"] is host  # (one cut per timepoint, as Tiler's crop cache)
        assert list(tiler.run_tp_device(0)) == ["pixels"] and tiler.run_tp_device(0)["pixels"] is dev
        assert tiler.get_fczyx(0, tile_size=5).shape == want.shape  # (accepted and unused, as in the reference)


# ------------------------------------------------------------------------------------------------ pipelines
TREE = {"None": {"None": ["sizeshape"]}, 0: {"max": ["intensity"]}, 1: {"max": ["intensity"]}}
MODES = {"raw": dict(standard_scale=False), "scaled": dict(standard_scale=True, clip_outliers=True)}
_PIPES = {}


def _fovs():
    from aliby_amd import synth

    if "fovs" not in _PIPES:
        _PIPES["fovs"] = [synth.make_fov(2, 310 + i, shape=(256, 256), n_channels=2, n_z=1, n_target=12) for i in range(2)]
    return _PIPES["fovs"]


def _override(mode):
    """flows_override for the tiles of both fields of view: every plane the segmenter shows (channel 0 of a tile, uint16 or
    float32) is matched to the restatement's tile it is nearest to and gets the analytic flows of the ground truth under it."""
    import torch

    from aliby_amd import synth
    from oracle import tiler_ref

    planes, flows = [], []
    for f in _fovs():
        tiles = cr.crop_tiles(f["pixels"], 128, **{"convert_8bit": False, "clip_outliers": False, **MODES[mode]})
        truth = cr.cut(f["nuclei"][None, None], 128)
        for t in range(tiles.shape[0]):
            planes.append(tiles[t, 0].max(axis=0).astype(np.float64))
            flows.append(synth.analytic_flows(tiler_ref.relabel_sequential(truth[t, 0, 0])))
    planes = np.stack(planes)

    def override(x):
        host = x.cpu().numpy().astype(np.float64)
        picked = []
        for i in range(host.shape[0]):
            d = np.abs(planes - host[i]).max(axis=(1, 2))
            assert d.min() < 1e-5, "a tile the restatement does not know"
            picked.append(flows[int(d.argmin())])
        return (torch.from_numpy(np.stack([p[0] for p in picked])).cuda(), torch.from_numpy(np.stack([p[1] for p in picked])).cuda())

    return override


def _pipelines(mode):
    override = _override(mode)
    return [{
        "ntps": 1,
        "steps": {
            "tile": {"kind": "crop", "tile_size": 128, "image_kwargs": {"source": f["pixels"][None]}, **MODES[mode]},
            "segment_nuclei": {"segmenter_kwargs": {"kind": "cellpose", "per_tile": True, "setup_params": {"flows_override": override}},
                               "channel_to_segment": 0},
            "extract_nuclei": {"tree": TREE},
        },
        "passed_data": {"extract_nuclei": [("masks", "segment_nuclei"), ("pixels", "tile")]},
        "passed_methods": {"segment_nuclei": ("tile", "get_fczyx")},
        "save": ("segment_nuclei",),
        "save_interval": 1,
    } for f in _fovs()]


@pytest.mark.parametrize("mode", list(MODES))
def test_crop_tiles_through_the_pipeline_and_the_batched_runner(tmp_path, engine, mode):
    """tile (crop) -> segment -> extract on two 256 x 256 two-channel frames, four tiles each: single calls of
    run_pipeline_and_post measure what NumPy measures on the restatement's tiles, and run_positions writes the same labels and
    integer columns bit for bit (float columns: rtol 1e-9, atol 1e-12, the project's rule for the two runners).  The mean
    intensity bar: the device copy is float32, so a mean of values below 10 in size is off by at most 10 x 2^-24 < 1e-5."""
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post

    names = ["C0", "C1"]
    single = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=tmp_path / "s")[0] for p, nm in zip(_pipelines(mode), names)]
    batched = [r[0] for r in run_positions(_pipelines(mode), names, tmp_path / "b", batch_size=2)]
    for i, nm in enumerate(names):
        with np.load(tmp_path / "s" / "steps" / nm / "segment_nuclei" / "0000.npz") as za, \
                np.load(tmp_path / "b" / "steps" / nm / "segment_nuclei" / "0000.npz") as zb:
            labels = za["arr_0"]
            assert labels.shape == (4, 128, 128) and labels.max() > 0 and np.array_equal(labels, zb["arr_0"])
        assert single[i].num_rows == batched[i].num_rows == sum(int(l.max()) for l in labels) > 0
        assert single[i].column_names == batched[i].column_names
        for c in single[i].column_names:
            a, b = single[i][c].to_numpy(zero_copy_only=False), batched[i][c].to_numpy(zero_copy_only=False)
            if a.dtype.kind != "f":
                assert np.array_equal(a, b), c
            else:
                assert np.allclose(a, b, rtol=1e-9, atol=1e-12, equal_nan=True), c
        tiles = cr.crop_tiles(_fovs()[i]["pixels"], 128, **{"convert_8bit": False, "clip_outliers": False, **MODES[mode]})
        rows = zip(single[i]["metadata_tile"].to_numpy(), single[i]["metadata_label"].to_numpy())
        want = np.array([tiles[t, 1, 0][labels[t] == l].astype(np.float64).mean() for t, l in rows])
        got = single[i]["1/max/intensity/Intensity_MeanIntensity"].to_numpy(zero_copy_only=False)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-5), nm
