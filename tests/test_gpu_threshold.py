"""
`FeatureEngine.auto_threshold` on the GPU (aliby_amd/csrc/feat_threshold.hip: k_threshold_search, on the histogram of
aliby_amd/csrc/tile_crop.hip) against tests/threshold_ref.py, the restatement of the definition in include/aliby_hip.h: thresholds and
details are equal, exactly.  The shapes are the smallest at which each path can go wrong: one pixel; 63 pixels (the tail of the
histogram's 8-pixel vector loop); three tiles of 33 x 65 (per-tile indexing; an odd tile size puts tiles 1 and 2 on the unaligned and
the aligned path); 2 x 64 x 128 (aligned); 256 x 256 (every grey level once); a view that starts one pixel into a buffer.
"""
import functools

import numpy as np
import pytest

from tests import threshold_ref as ref

pytestmark = pytest.mark.gpu

OPTIONS = {
    "two": {},
    "three": {"classes": 3},
    "three_background": {"classes": 3, "middle": "background"},
    "half": {"correction": 0.5},
    "0.7_three": {"classes": 3, "correction": 0.7},
    "1.5_background": {"classes": 3, "middle": "background", "correction": 1.5},
    "clamp_low": {"bounds": (40000, 65535)},
    "clamp_high": {"classes": 3, "middle": "background", "bounds": (0, 90)},
}


def _fill(shape, levels, seed=0):
    """A block of `shape` whose tiles hold the given levels, each at least once, in a seeded order."""
    rng = np.random.default_rng(seed)
    F, n = shape[0], shape[1] * shape[2]
    levels = np.asarray(levels, np.uint16)
    out = np.empty((F, n), np.uint16)
    for f in range(F):
        body = np.concatenate([levels, rng.choice(levels, max(n - len(levels), 0))])[:n]
        out[f] = rng.permutation(body)
    return out.reshape(shape)


def _trimodal(shape, seed, scale=1.0, offset=0):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    modes = rng.choice(3, n, p=[0.6, 0.3, 0.1])
    values = rng.normal(np.array([900.0, 5000.0, 21000.0])[modes], np.array([150.0, 900.0, 2500.0])[modes])
    return np.clip(values * scale + offset, 0, 65535).astype(np.uint16).reshape(shape)


def _scaled_tiles():
    base = _trimodal((3, 33, 65), 5)
    return np.stack([base[0], np.clip(base[1].astype(np.int64) * 3 + 700, 0, 65535).astype(np.uint16), base[2] // 16])


def _ties(levels, count, shape):
    """A block of `shape` that holds exactly `count` pixels of each level: every split between levels is a tie candidate."""
    n = shape[1] * shape[2]
    assert n == len(levels) * count
    return np.repeat(np.asarray(levels, np.uint16), count).reshape(shape)


CASES = {
    "one_pixel": lambda: np.array([[[4242]]], np.uint16),
    "constant_7x9": lambda: np.full((1, 7, 9), 32768, np.uint16),
    "two_levels_7x9": lambda: _fill((1, 7, 9), [100, 200], 1),
    "ends_7x9": lambda: _fill((1, 7, 9), [0, 65535], 2),
    "middle_7x9": lambda: _fill((1, 7, 9), [32767, 32768], 3),
    "middle_2x64x128": lambda: _fill((2, 64, 128), [32767, 32768], 4),
    "tie_10_20_30": lambda: _ties([10, 20, 30], 21, (1, 7, 9)),
    "tie_three_spikes": lambda: _ties([100, 200, 300], 2145 // 3, (1, 33, 65)),
    "narrow_7x9": lambda: (np.random.default_rng(6).integers(0, 40, (1, 7, 9)) + 32750).astype(np.uint16),
    "narrow_2x64x128": lambda: (np.random.default_rng(7).integers(0, 200, (2, 64, 128)) + 65336).astype(np.uint16),
    "ramp_256x256": lambda: np.random.default_rng(8).permutation(65536).astype(np.uint16).reshape(1, 256, 256),
    "trimodal_3x33x65": _scaled_tiles,
    "trimodal_2x64x128": lambda: _trimodal((2, 64, 128), 9),
    "dark_2x64x128": lambda: np.stack([_trimodal((64, 128), 10, 0.01), np.zeros((64, 128), np.uint16)]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    image = CASES[name]()
    image.setflags(write=False)
    return image


@functools.lru_cache(maxsize=None)
def want(name, options):
    return ref.otsu_batch(case(name), **OPTIONS[options])


def run(engine, image, **options):
    from aliby_amd.extraction.engine import to_device_u16

    thresholds, details = engine.auto_threshold(to_device_u16(np.array(image)), return_details=True, **options)
    return thresholds.cpu().numpy(), details.cpu().numpy()


@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("name", list(CASES))
def test_exact(engine, name, options):
    import torch

    thresholds, details = run(engine, case(name), **OPTIONS[options])
    exp_t, exp_d = want(name, options)
    print(name, options, thresholds.tolist(), exp_t.tolist(), details.tolist())
    assert thresholds.dtype == np.int32 and details.dtype == np.int32
    assert np.array_equal(details, exp_d), (details, exp_d)
    assert np.array_equal(thresholds, exp_t), (thresholds, exp_t)
    alone = engine.auto_threshold(torch.from_numpy(case(name).copy()).cuda(), **OPTIONS[options])  # without the details
    assert np.array_equal(alone.cpu().numpy(), exp_t)


def test_the_cases_hold_what_they_are_named_for():
    assert want("tie_10_20_30", "three")[1].tolist() == [[10, 30, 11, 21]] and want("tie_10_20_30", "two")[0].tolist() == [11]
    assert want("tie_three_spikes", "three")[1].tolist() == [[100, 300, 101, 201]] and want("tie_three_spikes", "two")[0].tolist() == [101]
    assert want("ends_7x9", "three")[1].tolist() == [[0, 65535, 1, 1]]
    assert want("middle_7x9", "two")[1].tolist() == [[32767, 32768, 32768, 32768]]
    assert want("constant_7x9", "three")[1].tolist() == [[32768] * 4] and want("one_pixel", "two")[0].tolist() == [4242]
    assert want("two_levels_7x9", "half")[0].tolist() == [50]  # 50.5, half to even
    lo, hi = want("narrow_7x9", "two")[1][0, :2]
    assert hi - lo < 256 and lo < 32768 <= hi
    assert want("ramp_256x256", "two")[1][0, :2].tolist() == [0, 65535]
    three = want("trimodal_3x33x65", "three")
    assert len(set(three[0].tolist())) == 3 and (three[1][:, 2] < three[1][:, 3]).all()  # three tiles, three thresholds; t1 < t2
    assert want("dark_2x64x128", "two")[1][1].tolist() == [0, 0, 0, 0]
    assert (want("trimodal_2x64x128", "clamp_low")[0] == 40000).all() and (want("trimodal_2x64x128", "clamp_high")[0] == 90).all()
    assert case("trimodal_3x33x65").shape == (3, 33, 65) and (33 * 65) % 8 == 1


def test_a_view_one_pixel_into_a_buffer(engine):
    """The tile starts 2 bytes past a 16-byte boundary: the histogram takes its pixel-by-pixel path."""
    import torch

    image = case("trimodal_2x64x128")
    flat = torch.zeros(image.size + 8, dtype=torch.uint16, device="cuda")
    flat[1:1 + image.size] = torch.from_numpy(image.copy()).cuda().reshape(-1)
    view = flat[1:1 + image.size].view(image.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 2
    for options in ("two", "0.7_three"):
        thresholds, details = engine.auto_threshold(view, return_details=True, **OPTIONS[options])
        assert np.array_equal(thresholds.cpu().numpy(), want("trimodal_2x64x128", options)[0])
        assert np.array_equal(details.cpu().numpy(), want("trimodal_2x64x128", options)[1])


def test_alone_in_a_batch_and_on_a_side_stream(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    tiles = case("trimodal_3x33x65")
    kw = OPTIONS["0.7_three"]
    exp_t, exp_d = want("trimodal_3x33x65", "0.7_three")
    alone = run(engine, tiles[1:2], **kw)
    batch = run(engine, np.stack([tiles[0], tiles[1], np.zeros_like(tiles[0]), tiles[1], tiles[2]]), **kw)
    for a, b, e in zip(alone, batch, (exp_t, exp_d)):
        assert np.array_equal(a[0], b[1]) and np.array_equal(a[0], b[3]) and np.array_equal(a[0], e[1])
        assert np.array_equal(b[0], e[0]) and np.array_equal(b[4], e[2])
    assert batch[0][2] == 0 and batch[1][2].tolist() == [0, 0, 0, 0]
    side = torch.cuda.Stream()
    dev = to_device_u16(tiles[1:2].copy())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        streamed = engine.auto_threshold(dev, return_details=True, **kw)
    side.synchronize()
    assert np.array_equal(streamed[0].cpu().numpy(), alone[0]) and np.array_equal(streamed[1].cpu().numpy(), alone[1])


def test_arguments(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    image = case("trimodal_3x33x65")
    dev = to_device_u16(image.copy())
    for kw, match in (({"method": "mce"}, "not built"), ({"method": "li"}, "not built"), ({"classes": 4}, "2 or 3"),
                      ({"middle": "background"}, "three classes only"), ({"classes": 3, "middle": "up"}, "'foreground' or 'background'"),
                      ({"correction": 0}, "\\(0, 16\\]"), ({"correction": float("nan")}, "\\(0, 16\\]"), ({"correction": True}, "\\(0, 16\\]"),
                      ({"bounds": (5, 4)}, "0 <= lo <= hi"), ({"bounds": (0, 65536)}, "0 <= lo <= hi"), ({"bounds": ("0", 5)}, "0 <= lo <= hi")):
        with pytest.raises(ValueError, match=match):
            engine.auto_threshold(dev, **kw)
    with pytest.raises(TypeError):
        engine.auto_threshold(dev, klasses=3)
    for bad in (dev[0], dev[None], dev.cpu(), dev.to(torch.int32), image):
        with pytest.raises(ValueError, match="uint16"):
            engine.auto_threshold(bad)
    with pytest.raises(ValueError, match="float32"):
        engine.auto_threshold(dev.to(torch.float32))
    # views that are not contiguous
    view = to_device_u16(np.pad(image, ((0, 0), (0, 3), (5, 0))))[:, :33, 5:]
    assert not view.is_contiguous()
    assert np.array_equal(engine.auto_threshold(view, classes=3).cpu().numpy(), want("trimodal_3x33x65", "three")[0])
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        z = torch.zeros(shape, dtype=torch.uint16, device=dev.device)
        thresholds, details = engine.auto_threshold(z, return_details=True)
        assert tuple(thresholds.shape) == (shape[0],) and thresholds.dtype == torch.int32 and tuple(details.shape) == (shape[0], 4)
        assert not thresholds.cpu().numpy().any()


def test_c_entry(engine):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr, to_device_u16

    lib, h = engine.lib, engine.ctx.handle
    image = case("trimodal_3x33x65")
    dev = to_device_u16(image.copy())
    F, Y, X = image.shape
    need = int(lib.aliby_auto_threshold_workspace_bytes(F))
    assert need == 262144 * F and int(lib.aliby_auto_threshold_workspace_bytes(0)) == 0
    work = torch.full((need // 4 + 4,), 77, dtype=torch.int32, device=dev.device)
    out = torch.full((F,), 77, dtype=torch.int32, device=dev.device)
    details = torch.full((F, 4), 77, dtype=torch.int32, device=dev.device)

    def call(i=None, shape=(F, Y, X), classes=3, middle=0, correction=0.7, lo=0, hi=65535, w=None, nbytes=need, o=None, d=None):
        return lib.aliby_auto_threshold(h, _ptr(dev) if i is None else i, *shape, classes, middle, correction, lo, hi,
                                        _ptr(work) if w is None else w, nbytes, _ptr(out) if o is None else o, _ptr(details) if d is None else d,
                                        _stream_ptr())

    _lib.check(call())
    torch.cuda.synchronize()
    exp_t, exp_d = want("trimodal_3x33x65", "0.7_three")
    assert np.array_equal(out.cpu().numpy(), exp_t) and np.array_equal(details.cpu().numpy(), exp_d)
    assert (work[need // 4:] == 77).all()  # nothing past the stated size
    out.fill_(77)
    _lib.check(call(d=0, middle=1, correction=1.5))  # no details asked
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want("trimodal_3x33x65", "1.5_background")[0])
    out.fill_(77)
    details.fill_(77)
    work.fill_(77)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="workspace"):  # one byte short
        _lib.check(call(nbytes=need - 1))
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(call(w=0))
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.check(call(w=work.data_ptr() + 8))
    for bad in (1, 4, 0, -2):
        with pytest.raises(ValueError, match="classes"):
            _lib.check(call(classes=bad))
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="middle"):
            _lib.check(call(middle=bad))
    for lo, hi in ((-1, 5), (6, 5), (0, 65536)):
        with pytest.raises(ValueError, match="bounds"):
            _lib.check(call(lo=lo, hi=hi))
    for bad in (0.0, -1.0, 16.5, float("nan")):
        with pytest.raises(ValueError, match="correction"):
            _lib.check(call(correction=bad))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(call(o=0))
    with pytest.raises(ValueError, match="65535 tiles"):  # by its arguments alone
        _lib.check(call(shape=(65536, Y, X)))
    with pytest.raises(ValueError, match="2\\^32"):
        _lib.check(call(shape=(1, 65536, 65536)))
    with pytest.raises(ValueError):
        _lib.check(call(shape=(-1, Y, X)))
    for shape in ((0, Y, X), (F, 0, X), (F, Y, 0)):  # zero pixels: a successful no-op with no buffers at all
        _lib.check(lib.aliby_auto_threshold(h, 0, *shape, 2, 0, 1.0, 0, 65535, 0, 0, 0, 0, _stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 77).all() and (details == 77).all() and (work == 77).all()  # no refused call wrote anything
    assert np.array_equal(dev.cpu().numpy(), image)


def test_host_form(engine):
    from aliby_amd.extraction import functions

    tiles = case("trimodal_3x33x65")
    got = functions.auto_threshold(tiles[1], classes=3, correction=0.7)
    assert type(got) is int and got == int(want("trimodal_3x33x65", "0.7_three")[0][1])
    assert functions.auto_threshold(tiles[2]) == int(want("trimodal_3x33x65", "two")[0][2])
    with pytest.raises(ValueError):
        functions.auto_threshold(tiles)  # one tile
    with pytest.raises(ValueError, match="float32"):
        functions.auto_threshold(tiles[0].astype(np.float32))
    with pytest.raises(ValueError, match="no pixel"):
        functions.auto_threshold(np.zeros((0, 4), np.uint16))
