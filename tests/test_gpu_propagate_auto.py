"""
`propagate` with one automatic threshold per tile: FeatureEngine.propagate_labels(thresholds=engine.auto_threshold(...)), the C entry
aliby_propagate_labels_per_tile and the host forms, on a three-tile scene of tests/propagate_cases.py whose stains are scaled so that
the tiles' Otsu thresholds differ.  The expected labels and distances are tests/propagate_ref.py run tile by tile with the threshold
tests/threshold_ref.py gives for that tile: equal bit for bit.  The threshold never leaves the device between the two calls.
"""
import functools

import numpy as np
import pytest

from tests import propagate_cases as pc
from tests import propagate_ref as ref
from tests import threshold_ref

pytestmark = pytest.mark.gpu

AUTO = {"classes": 3, "middle": "foreground", "correction": 0.7}
SHAPE = (3, 48, 80)


@functools.lru_cache(maxsize=None)
def scene():
    primary, image = pc.scene(SHAPE, 18, 11)
    image = np.stack([image[0], np.clip(image[1].astype(np.int64) * 2 + 3000, 0, 65535).astype(np.uint16), image[2] // 4])
    primary.setflags(write=False)
    image.setflags(write=False)
    return primary, image


@functools.lru_cache(maxsize=None)
def want(distance=None):
    """(thresholds [3], labels [3,Y,X], D [3,Y,X]): every tile on its own, at its own threshold."""
    primary, image = scene()
    thresholds = threshold_ref.otsu_batch(image, **AUTO)[0]
    tiles = [ref.propagate_labels(primary[f:f + 1], image[f:f + 1], threshold=int(thresholds[f]), distance=distance) for f in range(SHAPE[0])]
    return thresholds, np.concatenate([t[0] for t in tiles]), np.concatenate([t[1] for t in tiles])


def test_the_scene_holds_what_it_is_for():
    primary, image = scene()
    thresholds, labels, _ = want()
    assert len(set(thresholds.tolist())) == 3  # the tiles' thresholds differ
    for f in range(SHAPE[0]):
        assert primary[f].any() and (labels[f] != 0).sum() > (primary[f] != 0).sum() and (labels[f] == 0).any()
    # a threshold borrowed from another tile gives another result: the per-tile index matters
    other = ref.propagate_labels(primary[:1], image[:1], threshold=int(thresholds[1]))[0]
    assert not np.array_equal(other[0], labels[0])


def test_engine(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    primary, image = scene()
    dp, di = to_device_u16(primary.copy()), to_device_u16(image.copy())
    thresholds = engine.auto_threshold(di, **AUTO)
    assert thresholds.is_cuda and thresholds.dtype == torch.int32
    labels, dist = engine.propagate_labels(dp, di, thresholds=thresholds, return_distances=True)
    exp_t, exp_l, exp_d = want()
    assert np.array_equal(thresholds.cpu().numpy(), exp_t)
    assert np.array_equal(labels.cpu().numpy(), exp_l) and np.array_equal(dist.cpu().numpy(), exp_d)
    # with a distance as well
    near = engine.propagate_labels(dp, di, thresholds=thresholds, distance=6)
    assert np.array_equal(near.cpu().numpy(), want(6)[1])
    # a tile alone equals the tile in the batch
    alone = engine.propagate_labels(dp[2:3], di[2:3], thresholds=engine.auto_threshold(di[2:3], **AUTO))
    assert np.array_equal(alone.cpu().numpy()[0], exp_l[2])


def test_one_value_for_every_tile_is_the_scalar_call(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    primary, image = scene()
    dp, di = to_device_u16(primary.copy()), to_device_u16(image.copy())
    for level in (0, 3000, 65535, 65536):
        filled = torch.full((SHAPE[0],), level, dtype=torch.int32, device=dp.device)
        got = engine.propagate_labels(dp, di, thresholds=filled, return_distances=True)
        if level <= 65535:
            scalar = engine.propagate_labels(dp, di, threshold=level, return_distances=True)
            assert torch.equal(got[0], scalar[0]) and torch.equal(got[1], scalar[1])
        else:  # above every grey level: nothing unlabelled passes
            assert np.array_equal(got[0].cpu().numpy(), primary)
    assert np.array_equal(engine.propagate_labels(dp, di, threshold=3000).cpu().numpy(), ref.propagate_labels(primary, image, threshold=3000)[0])


def test_arguments(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    primary, image = scene()
    dp, di = to_device_u16(primary.copy()), to_device_u16(image.copy())
    good = torch.full((SHAPE[0],), 3000, dtype=torch.int32, device=dp.device)
    with pytest.raises(ValueError, match="threshold or thresholds, not both"):
        engine.propagate_labels(dp, di, threshold=5, thresholds=good)
    for bad in (good.to(torch.int64), good.to(torch.float32), good[:2], good[None], good.cpu(), good.cpu().numpy(), [3000] * 3, 3000):
        with pytest.raises(ValueError, match="thresholds must be an int32 \\[3\\] tensor"):
            engine.propagate_labels(dp, di, thresholds=bad)
    # an explicit threshold of 0 beside it is no conflict; a strided view is taken
    wide = torch.full((SHAPE[0], 2), 3000, dtype=torch.int32, device=dp.device)
    assert not wide[:, 0].is_contiguous()
    a = engine.propagate_labels(dp, di, threshold=0, thresholds=wide[:, 0])
    assert torch.equal(a, engine.propagate_labels(dp, di, threshold=3000))


def test_c_entry(engine):
    import ctypes

    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr, to_device_u16

    lib, h = engine.lib, engine.ctx.handle
    primary, image = scene()
    dp, di = to_device_u16(primary.copy()), to_device_u16(image.copy())
    F, Y, X = SHAPE
    exp_t, exp_l, exp_d = want()
    dt = torch.from_numpy(exp_t.copy()).to(dp.device)
    need = int(lib.aliby_propagate_workspace_bytes(F, Y, X))
    work = torch.empty(need // 8, dtype=torch.int64, device=dp.device)
    out = torch.full_like(dp, 77)
    dist = torch.full(dp.shape, 77, dtype=torch.int64, device=dp.device)
    stats = (ctypes.c_int32 * 2)(-1, -1)

    def call(t=None, shape=(F, Y, X), n=0, nbytes=need, st=None):
        return lib.aliby_propagate_labels_per_tile(h, _ptr(dp), _ptr(di), *shape, _ptr(dt) if t is None else t, ref.lambda2(), n,
                                                   _ptr(work), nbytes, _ptr(out), _ptr(dist), st, _stream_ptr())

    _lib.check(call(st=stats))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), exp_l) and np.array_equal(dist.cpu().numpy().view(np.uint64), exp_d)
    assert stats[0] >= 1 and stats[1] >= 1
    out.fill_(77)
    dist.fill_(77)
    with pytest.raises(ValueError, match="thresholds is NULL"):
        _lib.check(call(t=0))
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(call(nbytes=need - 1))
    with pytest.raises(ValueError, match="distance"):
        _lib.check(call(n=65))
    for shape in ((0, Y, X), (F, 0, X)):  # zero pixels: a no-op that needs no thresholds either
        _lib.check(lib.aliby_propagate_labels_per_tile(h, 0, 0, *shape, 0, ref.lambda2(), 0, 0, 0, 0, 0, None, _stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 77).all() and (dist == 77).all()  # no refused call wrote anything


def test_host_forms(engine):
    from aliby_amd.extraction import extract, functions

    primary, image = scene()
    exp_t, exp_l, _ = want()
    for f in range(SHAPE[0]):
        one = functions.propagate_objects(primary[f], image[f], auto_threshold=AUTO)
        assert one.dtype == np.uint16 and np.array_equal(one, exp_l[f])
        assert functions.auto_threshold(image[f], **AUTO) == int(exp_t[f])
    assert np.array_equal(functions.propagate_objects(primary[0], image[0], threshold=0, auto_threshold=dict(AUTO)), exp_l[0])
    with pytest.raises(ValueError, match="not both"):
        functions.propagate_objects(primary[0], image[0], threshold=10, auto_threshold=AUTO)

    # [F,C,Z,Y,X] pixels whose channel 1, max-projected over Z, is the image
    rng = np.random.default_rng(3)
    pixels = rng.integers(0, 500, (3, 2, 3, *SHAPE[1:])).astype(np.uint16)
    pixels[:, 1] = np.minimum(pixels[:, 1], image[:, None])
    pixels[:, 1, 1] = image
    chosen = []
    per_tile = extract.propagate_masks([t for t in primary], pixels, 1, auto_threshold=AUTO, chosen=chosen)
    assert isinstance(per_tile, list) and len(per_tile) == 3 and chosen == exp_t.tolist() and all(type(t) is int for t in chosen)
    for f, tile in enumerate(per_tile):
        assert tile.dtype == np.uint16 and np.array_equal(tile, exp_l[f])
    tile = extract.propagate_masks(primary[1], pixels[1:2], 1, auto_threshold=AUTO, distance=6)
    assert np.array_equal(tile, want(6)[1][1])
    extract.propagate_masks(primary[1], pixels[1:2], 1, threshold=1234, chosen=chosen)
    assert chosen == [1234]
    with pytest.raises(ValueError, match="a test: .*not both"):
        extract.propagate_masks(primary[1], pixels[1:2], 1, threshold=5, auto_threshold=AUTO, who="a test")
    with pytest.raises(ValueError, match="a test: .*not built"):
        extract.propagate_masks(primary[1], pixels[1:2], 1, auto_threshold={"method": "mce"}, who="a test")


TWO_CLASS = {"default": {}, "corrected": {"correction": 0.7}, "explicit": {"classes": 2, "bounds": [500, 20000]}}


@functools.lru_cache(maxsize=None)
def want_two(name):
    """want() for the two-class options of TWO_CLASS[name]."""
    primary, image = scene()
    thresholds = threshold_ref.otsu_batch(image, **TWO_CLASS[name])[0]
    tiles = [ref.propagate_labels(primary[f:f + 1], image[f:f + 1], threshold=int(thresholds[f]))[0] for f in range(SHAPE[0])]
    return thresholds, np.concatenate(tiles)


@pytest.mark.parametrize("name", list(TWO_CLASS))
def test_two_classes_through_every_surface(engine, name):
    """Two classes are the default ({} is two-class Otsu): the step, propagate_masks and propagate_objects hand their checked options
    down to the engine, which checks them again."""
    from aliby_amd.extraction import extract, functions
    from aliby_amd.extraction.engine import to_device_u16
    from aliby_amd.pipe import init_step

    auto = TWO_CLASS[name]
    primary, image = scene()
    exp_t, exp_l = want_two(name)
    assert len(set(exp_t.tolist())) == 3 and exp_t.tolist() != want()[0].tolist()
    pixels = np.zeros((3, 2, 2, *SHAPE[1:]), np.uint16)
    pixels[:, 1, 0] = image  # channel 1, max-projected over Z, is the image

    dp, di = to_device_u16(primary.copy()), to_device_u16(image.copy())
    got = engine.propagate_labels(dp, di, thresholds=engine.auto_threshold(di, **auto))
    assert np.array_equal(got.cpu().numpy(), exp_l)

    step = init_step("propagate_cell", {"channel": 1, "auto_threshold": dict(auto)})
    for _ in range(2):  # the stored options serve every call
        tiles = step(primary=[t for t in primary], pixels=pixels)
        assert step.thresholds == exp_t.tolist()
        for f, tile in enumerate(tiles):
            assert np.array_equal(tile, exp_l[f])

    chosen = []
    tiles = extract.propagate_masks([t for t in primary], pixels, 1, auto_threshold=dict(auto), chosen=chosen)
    assert chosen == exp_t.tolist() and all(np.array_equal(tile, exp_l[f]) for f, tile in enumerate(tiles))
    for f in range(SHAPE[0]):
        assert np.array_equal(functions.propagate_objects(primary[f], image[f], auto_threshold=dict(auto)), exp_l[f])
        assert functions.auto_threshold(image[f], **auto) == int(exp_t[f])
