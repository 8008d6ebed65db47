"""
FeatureEngine.secondary_labels (csrc/feat_secondary.hip: "Distance - N" of CellProfiler's IdentifySecondaryObjects) against the
brute-force restatement tests/secondary_ref.py, bit for bit in every case: shapes that break the tiling (narrower than a wave, one
row, one column, a tile smaller than the halo, several row segments and several 256-pixel blocks of a row), contents that exercise
the tie rule in every direction, the sentinel and the tile edges, batches, a side stream, the C entry's refusals and the host forms.
Neither kernel caps its grid (the entry refuses a launch it cannot make in one piece), so no case has to reach past a first pass;
the thin wide tile still puts objects into the last of its 274 row blocks.
"""
import functools

import numpy as np
import pytest

from tests import secondary_ref as ref

pytestmark = pytest.mark.gpu


def sprinkle(shape, n_obj, seed, max_side=4):
    """[F,Y,X] uint16: small rectangles of random labels (repeated and non-consecutive labels, 65535 among them)."""
    rng = np.random.default_rng(seed)
    F, Y, X = shape
    lab = np.zeros(shape, np.uint16)
    pool = np.concatenate([np.arange(1, 40), [255, 256, 4097, 65534, 65535]])
    for _ in range(n_obj):
        f, y, x = rng.integers(0, F), rng.integers(0, Y), rng.integers(0, X)
        h, w = rng.integers(1, max_side + 1, 2)
        lab[f, y:y + h, x:x + w] = rng.choice(pool)
    return lab


def _at(shape, *pixels):
    lab = np.zeros(shape, np.uint16)
    for (y, x), v in pixels:
        lab[0, y, x] = v
    return lab


def _wide():
    lab = np.zeros((1, 2, 70000), np.uint16)
    for x, v in ((0, 5), (255, 6), (256, 7), (300, 2), (30000, 9), (65535, 11), (65600, 3), (69990, 8), (69999, 1)):
        lab[0, x % 2, x] = v
    return lab


def _batch_edges():
    lab = np.zeros((3, 9, 40), np.uint16)
    lab[0, 8, 3:30] = 7   # the last row of tile 0
    lab[2, 0, 10:38] = 4  # the first row of tile 2; tile 1 is empty and must stay empty
    return lab


CASES = {
    # shapes
    "37x53": (sprinkle((1, 37, 53), 9, 1), (1, 5, 64)),
    "1x200": (sprinkle((1, 1, 200), 6, 2, max_side=3), (1, 5, 64)),
    "200x1": (sprinkle((1, 200, 1), 6, 3, max_side=3), (1, 5, 64)),
    "5x7_smaller_than_the_halo": (sprinkle((1, 5, 7), 2, 4, max_side=1), (1, 16, 64)),
    "3x64x96": (sprinkle((3, 64, 96), 24, 5), (1, 5, 64)),
    "2x100x300_segments_and_blocks": (sprinkle((2, 100, 300), 40, 6), (1, 5, 16, 64)),
    "2x70000_thin": (_wide(), (1, 5, 64)),
    # contents
    "all_zero": (np.zeros((1, 40, 70), np.uint16), (1, 5, 64)),
    "fully_labelled": ((np.arange(33 * 65, dtype=np.uint32).reshape(1, 33, 65) % 65535 + 1).astype(np.uint16), (1, 5, 64)),
    "1_and_65535": (_at((1, 3, 12), ((1, 2), 1), ((1, 9), 65535), ((0, 9), 65535)), (1, 3, 5, 64)),
    "65535_alone": (_at((1, 70, 70), ((35, 35), 65535)), (1, 5, 64)),
    "four_corners": (_at((1, 41, 67), ((0, 0), 3), ((0, 66), 1), ((40, 0), 65535), ((40, 66), 2)), (1, 5, 64)),
    "vertical_tie_smaller_below": (_at((1, 70, 9), ((10, 4), 9), ((20, 4), 2), ((33, 2), 8), ((36, 2), 3)), (1, 5, 64)),
    "vertical_tie_smaller_above": (_at((1, 70, 9), ((10, 4), 2), ((20, 4), 9), ((31, 2), 3), ((34, 2), 8)), (1, 5, 64)),
    "horizontal_tie_smaller_right": (_at((1, 5, 300), ((2, 10), 9), ((2, 20), 2), ((3, 250), 8), ((3, 262), 3)), (1, 5, 64)),
    "horizontal_tie_smaller_left": (_at((1, 5, 300), ((2, 10), 2), ((2, 20), 9), ((3, 250), 3), ((3, 262), 8)), (1, 5, 64)),
    # (5, 5) is 5 from (2, 1) and from (5, 10): 9 + 16 = 25 = 0 + 25; and from (1, 2) and (8, 9): 16 + 9 = 9 + 16
    "diagonal_tie": (_at((1, 12, 14), ((2, 1), 9), ((5, 10), 4)), (5, 64)),
    "diagonal_tie_mirrored": (_at((1, 12, 14), ((1, 2), 4), ((8, 9), 9)), (5, 64)),
    # (5, 5) has (2, 5) in its own column and (5, 8) in its own row, both at 3
    "column_against_row_tie": (_at((1, 12, 14), ((2, 5), 9), ((5, 8), 4)), (3, 5, 64)),
    "column_against_row_tie_swapped": (_at((1, 12, 14), ((2, 5), 4), ((5, 8), 9)), (3, 5, 64)),
    # batch
    "batch_edges": (_batch_edges(), (1, 5, 64)),
}
PAIRS = [(name, n) for name, (_, ns) in CASES.items() for n in ns]


@functools.lru_cache(maxsize=None)
def want(name, n):
    out = ref.secondary_labels(CASES[name][0], n)
    out.setflags(write=False)
    return out


def run(engine, labels, n):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    dev = to_device_u16(labels)
    got = engine.secondary_labels(dev, n)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint16 and got.shape == dev.shape and got.data_ptr() != dev.data_ptr()
    assert np.array_equal(dev.cpu().numpy(), labels)  # the input is left alone
    return got.cpu().numpy()


@pytest.mark.parametrize("name, n", PAIRS)
def test_exact(engine, name, n):
    labels = CASES[name][0]
    got, exp = run(engine, labels, n), want(name, n)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{name} N={n}: {len(bad)} pixels differ, first at {bad[0]}: got {got[tuple(bad[0])]}, want {exp[tuple(bad[0])]}"
    assert np.array_equal(got[labels != 0], labels[labels != 0])


def test_the_cases_hold_what_they_are_named_for():
    """The restatement on the content cases: the ties are ties and go to the smaller label, tile 1 of the batch stays empty."""
    assert not want("all_zero", 64).any() and np.array_equal(want("fully_labelled", 64), CASES["fully_labelled"][0])
    assert want("1_and_65535", 3)[0, 1].tolist() == [1, 1, 1, 1, 1, 1, 65535, 65535, 65535, 65535, 65535, 65535]
    assert want("vertical_tie_smaller_below", 5)[0, 15, 4] == 2 and want("vertical_tie_smaller_above", 5)[0, 15, 4] == 2
    assert want("vertical_tie_smaller_below", 1)[0, 15, 4] == 0
    assert want("horizontal_tie_smaller_right", 64)[0, 3, 256] == 3 and want("horizontal_tie_smaller_left", 64)[0, 3, 256] == 3
    assert want("diagonal_tie", 5)[0, 5, 5] == 4 and want("diagonal_tie_mirrored", 5)[0, 5, 5] == 4
    assert want("column_against_row_tie", 3)[0, 5, 5] == 4 and want("column_against_row_tie_swapped", 3)[0, 5, 5] == 4
    for n in (1, 5, 64):
        assert not want("batch_edges", n)[1].any() and want("batch_edges", n)[0].any() and want("batch_edges", n)[2].any()
    assert want("2x70000_thin", 5)[0, 1, 69995] == 1 and want("2x70000_thin", 5)[0, 0, 65537] == 11


@pytest.mark.parametrize("n", [1, 5, 64])
def test_alone_in_a_batch_and_on_a_side_stream(engine, n):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    tile = CASES["3x64x96"][0][1]
    other = CASES["3x64x96"][0][0]
    alone = engine.secondary_labels(to_device_u16(tile[None]), n)
    batch = engine.secondary_labels(to_device_u16(np.stack([other, tile, np.zeros_like(tile), tile])), n)
    torch.cuda.synchronize()
    assert torch.equal(alone[0].view(torch.int16), batch[1].view(torch.int16))
    assert torch.equal(alone[0].view(torch.int16), batch[3].view(torch.int16)) and not batch[2].cpu().numpy().any()
    side = torch.cuda.Stream()
    dev = to_device_u16(tile[None])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        streamed = engine.secondary_labels(dev, n)
    side.synchronize()
    assert torch.equal(alone.view(torch.int16), streamed.view(torch.int16))
    assert np.array_equal(alone[0].cpu().numpy(), want("3x64x96", n)[1])


def test_arguments(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    dev = to_device_u16(CASES["37x53"][0])
    for bad in (0, 65, -3, True, 2.5, None, "5"):
        with pytest.raises(ValueError, match="1..64"):
            engine.secondary_labels(dev, bad)
    for bad in (dev[0], dev[None], dev.cpu(), dev.to(torch.int32), CASES["37x53"][0]):
        with pytest.raises(ValueError, match="uint16"):
            engine.secondary_labels(bad, 5)
    assert np.array_equal(engine.secondary_labels(dev, 5.0).cpu().numpy(), want("37x53", 5))  # a float that holds an integer
    view = to_device_u16(np.pad(CASES["37x53"][0], ((0, 0), (0, 0), (0, 11))))[:, :, :53]  # not contiguous
    assert np.array_equal(engine.secondary_labels(view, 5).cpu().numpy(), want("37x53", 5))
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        empty = engine.secondary_labels(torch.zeros(shape, dtype=torch.uint16, device=dev.device), 3)
        assert tuple(empty.shape) == shape and empty.dtype == torch.uint16


def test_c_entry(engine):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr, to_device_u16

    lib, h = engine.lib, engine.ctx.handle
    labels = CASES["37x53"][0]
    dev = to_device_u16(labels)
    F, Y, X = labels.shape
    need = int(lib.aliby_secondary_workspace_bytes(F, Y, X))
    assert need == 4 * F * Y * X and int(lib.aliby_secondary_workspace_bytes(0, Y, X)) == 0
    work = torch.empty(need // 4, dtype=torch.int32, device=dev.device)
    out = torch.full_like(dev, 77)
    _lib.check(lib.aliby_secondary_labels(h, _ptr(dev), F, Y, X, 5, _ptr(work), need, _ptr(out), _stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want("37x53", 5))
    # the workspace need only be 4-byte aligned
    even = to_device_u16(CASES["3x64x96"][0])
    spare = torch.empty(3 * 64 * 96 + 1, dtype=torch.int32, device=dev.device)
    assert spare.data_ptr() % 8 == 0
    out_even = torch.empty_like(even)
    _lib.check(lib.aliby_secondary_labels(h, _ptr(even), 3, 64, 96, 5, spare.data_ptr() + 4, 4 * 3 * 64 * 96, _ptr(out_even), _stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(out_even.cpu().numpy(), want("3x64x96", 5))
    out.fill_(77)
    with pytest.raises(ValueError, match="alias"):  # out == primary
        _lib.check(lib.aliby_secondary_labels(h, _ptr(dev), F, Y, X, 5, _ptr(work), need, _ptr(dev), _stream_ptr()))
    with pytest.raises(ValueError, match="workspace"):  # a workspace one word short
        _lib.check(lib.aliby_secondary_labels(h, _ptr(dev), F, Y, X, 5, _ptr(work), need - 4, _ptr(out), _stream_ptr()))
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(lib.aliby_secondary_labels(h, _ptr(dev), F, Y, X, 5, 0, need, _ptr(out), _stream_ptr()))
    for bad in (0, 65):
        with pytest.raises(ValueError, match="distance"):
            _lib.check(lib.aliby_secondary_labels(h, _ptr(dev), F, Y, X, bad, _ptr(work), need, _ptr(out), _stream_ptr()))
    with pytest.raises(ValueError):
        _lib.check(lib.aliby_secondary_labels(h, _ptr(dev), -1, Y, X, 5, _ptr(work), need, _ptr(out), _stream_ptr()))
    # zero pixels: a successful no-op that touches nothing, with no buffers at all
    for shape in ((0, Y, X), (F, 0, X), (F, Y, 0)):
        _lib.check(lib.aliby_secondary_labels(h, 0, *shape, 5, 0, 0, 0, _stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 77).all() and np.array_equal(dev.cpu().numpy(), labels)  # no refused call wrote anything


def test_host_forms(engine):
    from aliby_amd import devcache
    from aliby_amd.extraction import extract, functions

    tiles = CASES["3x64x96"][0]
    exp = want("3x64x96", 5)
    one = functions.secondary_objects(tiles[0], 5)
    assert isinstance(one, np.ndarray) and one.dtype == np.uint16 and np.array_equal(one, exp[0])
    with pytest.raises(ValueError):
        functions.secondary_objects(tiles, 5)  # one tile
    with pytest.raises(ValueError):
        functions.secondary_objects(tiles[0], 0)

    image = extract.secondary_masks(tiles[1], 5)
    assert isinstance(image, np.ndarray) and image.shape == tiles[1].shape and np.array_equal(image, exp[1])
    per_tile = extract.secondary_masks([t for t in tiles], 5, who="a test")
    assert isinstance(per_tile, list) and len(per_tile) == 3
    for k, t in enumerate(per_tile):
        assert t.dtype == np.uint16 and np.array_equal(t, exp[k])
    for t in (image, *per_tile):  # the device copy travels with the host image, as a segment step's does
        hit = devcache.lookup(t)
        assert hit is not None and np.array_equal(hit[0].cpu().numpy().reshape(t.shape), t)
    with pytest.raises(ValueError):
        extract.secondary_masks([], 5)
    with pytest.raises(ValueError):
        extract.secondary_masks(tiles[0], 65)
