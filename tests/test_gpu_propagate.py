"""
FeatureEngine.propagate_labels (csrc/feat_propagate.hip: "Propagation" and "Distance - B" of CellProfiler's IdentifySecondaryObjects
on an exact integer metric) against the restatement tests/propagate_ref.py, labels and distances bit for bit in every case: shapes
around the 32 x 32 region of a workgroup (31, 32, 33, 63, 64, 65, 129 on either axis, one row, one column, a tile smaller than a
region), contents that exercise the tie rule, the threshold, the clamp at the tile edges and the largest weights, the reach mask,
batches, a side stream, the C entry's refusals and the host forms.  The serpentine corridor needs far more rounds than one chunk
holds, so the loop across reads of the change flags is what produced the compared result.
"""
import functools

import numpy as np
import pytest

from tests import propagate_cases as pc
from tests import propagate_ref as ref

pytestmark = pytest.mark.gpu

FLAT_ROW = (pc.at((1, 1, 9), ((0, 0), 7), ((0, 8), 3)), pc.flat((1, 1, 9)))


def _touching():
    lab = np.zeros((1, 20, 40), np.uint16)
    lab[0, 5:12, 10:18] = 6
    lab[0, 5:12, 18:25] = 2  # edge to edge with 6
    lab[0, 12:15, 10:25] = 65535
    return lab, pc.scene((1, 20, 40), 3, 50)[1]


def _full(Y=33, X=65):
    return (np.arange(Y * X, dtype=np.uint32).reshape(1, Y, X) % 65535 + 1).astype(np.uint16), pc.scene((1, Y, X), 4, 51)[1]


_DEFAULT = ({}, {"threshold": 3000})
_AXES = {f"{y}x{x}": (y, x) for y, x in ((31, 40), (32, 32), (33, 65), (63, 34), (64, 64), (65, 31), (129, 33), (40, 129), (40, 63))}

CASES = {
    # shapes
    "37x53": (pc.scene((1, 37, 53), 5, 1), _DEFAULT),
    "1x200": (pc.scene((1, 1, 200), 4, 2), _DEFAULT),
    "200x1": (pc.scene((1, 200, 1), 4, 3), _DEFAULT),
    "5x7": (pc.scene((1, 5, 7), 2, 4), _DEFAULT),
    **{name: (pc.scene((1, y, x), 5, 10 + k), ({"threshold": 2500},)) for k, (name, (y, x)) in enumerate(_AXES.items())},
    "3x64x96": (pc.scene((3, 64, 96), 14, 5), _DEFAULT),
    "2x100x300": (pc.scene((2, 100, 300), 30, 6), ({"threshold": 2000},)),
    # contents
    "all_zero": ((np.zeros((1, 40, 70), np.uint16), pc.scene((1, 40, 70), 3, 7)[1]), ({},)),
    "fully_labelled": (_full(), ({}, {"threshold": 65535})),
    "1_and_65535": ((pc.at((1, 3, 12), ((1, 2), 1), ((1, 9), 65535), ((0, 9), 65535)), pc.flat((1, 3, 12))), ({},)),
    "touching_seeds": (_touching(), _DEFAULT),
    "flat_row_tie": (FLAT_ROW, ({},)),
    "flat_column_tie": ((FLAT_ROW[0].transpose(0, 2, 1).copy(), pc.flat((1, 9, 1))), ({},)),
    "flat_diagonal_tie": ((pc.at((1, 9, 9), ((0, 0), 7), ((8, 8), 3)), pc.flat((1, 9, 9))), ({},)),
    "flat_ties_across_regions": ((pc.at((1, 70, 70), ((2, 2), 9), ((66, 66), 4), ((2, 66), 5), ((66, 2), 65535)), pc.flat((1, 70, 70))), ({},)),
    "ridge": (pc.ridge(), ({},)),
    "ridge_flat": ((pc.ridge()[0], pc.flat((1, 21, 40), 2000)), ({},)),
    "wall_with_island": (pc.wall(), ({"threshold": 1000},)),
    "lambda_zero_flat": ((pc.scene((1, 37, 53), 5, 8)[0], pc.flat((1, 37, 53))), ({"regularization": 0.0},)),
    "checkerboard": (pc.checkerboard(), ({}, {"regularization": 16.0, "image_max": 65535})),
    "gradient_into_every_edge": (pc.gradient(), ({}, {"regularization": 0.0})),
    "distance": (pc.scene((1, 70, 90), 4, 9), tuple({"distance": n, "threshold": t} for n in (1, 5, 64) for t in (0, 3000))),
    "serpentine_70x300": (pc.serpentine(70, 300, 8), ({"threshold": 1},)),
}
PAIRS = [(name, k) for name, (_, kws) in CASES.items() for k in range(len(kws))]


@functools.lru_cache(maxsize=None)
def want(name, k):
    primary, image = CASES[name][0]
    out, D = ref.propagate_labels(primary, image, **CASES[name][1][k])
    out.setflags(write=False)
    D.setflags(write=False)
    return out, D


def run(engine, primary, image, **kw):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    dp, di = to_device_u16(primary), to_device_u16(image)
    got, dist = engine.propagate_labels(dp, di, return_distances=True, **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint16 and got.shape == dp.shape and got.data_ptr() != dp.data_ptr()
    assert dist.dtype == torch.uint64 and dist.shape == dp.shape
    assert np.array_equal(dp.cpu().numpy(), primary) and np.array_equal(di.cpu().numpy(), image)  # the inputs are left alone
    return got.cpu().numpy(), dist.cpu().numpy()


@pytest.mark.parametrize("name, k", PAIRS)
def test_exact(engine, name, k):
    primary, image = CASES[name][0]
    (got, dist), (exp, exp_dist) = run(engine, primary, image, **CASES[name][1][k]), want(name, k)
    bad = np.argwhere((got != exp) | (dist != exp_dist))
    assert bad.size == 0, (f"{name} {CASES[name][1][k]}: {len(bad)} pixels differ, first at {bad[0]}: got {got[tuple(bad[0])]} at "
                           f"{dist[tuple(bad[0])]}, want {exp[tuple(bad[0])]} at {exp_dist[tuple(bad[0])]}")
    assert np.array_equal(got[primary != 0], primary[primary != 0])
    rounds, reads = engine.propagate_stats
    assert reads >= 1 and 0 <= rounds <= 8 * reads
    if name in ("all_zero", "fully_labelled"):
        assert rounds == 0 and reads == 1
    if name == "serpentine_70x300":
        assert reads > 1 and rounds > 8  # the loop across chunks produced the compared result
        assert got[0, 69, 150] == 5  # ... and it reached the last corridor


def test_the_cases_hold_what_they_are_named_for():
    """The restatement on the content cases (no device needed for this one's claims)."""
    assert not want("all_zero", 0)[0].any() and (want("all_zero", 0)[1] == ref.NONE).all()
    assert np.array_equal(want("fully_labelled", 1)[0], CASES["fully_labelled"][0][0]) and not want("fully_labelled", 1)[1].any()
    assert want("flat_row_tie", 0)[0][0, 0].tolist() == [7, 7, 7, 7, 3, 3, 3, 3, 3]
    assert want("flat_row_tie", 0)[1][0, 0].tolist() == [0, 52428, 104856, 157284, 209712, 157284, 104856, 52428, 0]
    assert want("flat_column_tie", 0)[0][0, :, 0].tolist() == [7, 7, 7, 7, 3, 3, 3, 3, 3]
    assert want("flat_diagonal_tie", 0)[0][0, 4, 4] == 3 and want("flat_diagonal_tie", 0)[1][0, 4, 4] == 4 * 74144
    out = want("wall_with_island", 0)[0][0]
    assert (out[:, :30] == 3).all() and not out[:, 30:].any()
    assert (want("ridge_flat", 0)[0][0, 10, :20] == 4).all() and (want("ridge_flat", 0)[0][0, 10, 20:] == 9).all()
    assert (want("ridge", 0)[0][0, 10, :12] == 4).all() and (want("ridge", 0)[0][0, 10, 13:] == 9).all()
    assert want("checkerboard", 0)[1][want("checkerboard", 0)[0] != 0].max() < 1 << 48
    for k, kw in enumerate(CASES["distance"][1]):
        if kw["threshold"] == 0:
            from tests import secondary_ref

            assert np.array_equal(want("distance", k)[0] != 0, secondary_ref.secondary_labels(CASES["distance"][0][0], kw["distance"]) != 0)


def test_alone_in_a_batch_and_on_a_side_stream(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    primary, image = CASES["3x64x96"][0]
    kw = {"threshold": 3000, "return_distances": True}
    alone = engine.propagate_labels(to_device_u16(primary[1:2]), to_device_u16(image[1:2]), **kw)
    zero = np.zeros_like(primary[1])
    batch = engine.propagate_labels(to_device_u16(np.stack([primary[0], primary[1], zero, primary[1]])),
                                    to_device_u16(np.stack([image[0], image[1], image[2], image[1]])), **kw)
    torch.cuda.synchronize()
    for a, b in zip(alone, batch):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a[0], b[1]) and np.array_equal(a[0], b[3])
    assert not batch[0][2].cpu().numpy().any()
    side = torch.cuda.Stream()
    dp, di = to_device_u16(primary[1:2]), to_device_u16(image[1:2])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        streamed = engine.propagate_labels(dp, di, **kw)
    side.synchronize()
    assert np.array_equal(alone[0].cpu().numpy(), streamed[0].cpu().numpy()) and np.array_equal(alone[1].cpu().numpy(), streamed[1].cpu().numpy())
    assert np.array_equal(alone[0][0].cpu().numpy(), want("3x64x96", 1)[0][1]) and np.array_equal(alone[1][0].cpu().numpy(), want("3x64x96", 1)[1][1])


def test_arguments(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    primary, image = CASES["37x53"][0]
    dp, di = to_device_u16(primary), to_device_u16(image)
    for kw, match in (({"threshold": -1}, "0..65535"), ({"threshold": 65536}, "0..65535"), ({"threshold": True}, "0..65535"),
                      ({"threshold": 2.5}, "0..65535"), ({"regularization": -0.1}, ">= 0"), ({"regularization": float("nan")}, ">= 0"),
                      ({"regularization": float("inf")}, ">= 0"), ({"regularization": 17.0}, "2\\^20"), ({"distance": 0}, "1..64"),
                      ({"distance": 65}, "1..64"), ({"distance": 2.5}, "1..64"), ({"image_max": 0}, "1..65535"), ({"image_max": 65536}, "1..65535")):
        with pytest.raises(ValueError, match=match):
            engine.propagate_labels(dp, di, **kw)
    for bad in (dp[0], dp[None], dp.cpu(), dp.to(torch.int32), primary):
        with pytest.raises(ValueError, match="uint16"):
            engine.propagate_labels(bad, di)
    with pytest.raises(ValueError, match="float32"):
        engine.propagate_labels(dp, di.to(torch.float32))
    with pytest.raises(ValueError, match="share one shape"):
        engine.propagate_labels(dp, di[:, :, :50])
    # a float that holds an integer; views that are not contiguous
    assert np.array_equal(engine.propagate_labels(dp, di, threshold=3000.0).cpu().numpy(), want("37x53", 1)[0])
    vp = to_device_u16(np.pad(primary, ((0, 0), (0, 0), (0, 11))))[:, :, :53]
    vi = to_device_u16(np.pad(image, ((0, 0), (0, 3), (5, 0))))[:, :37, 5:]
    assert not vp.is_contiguous() and not vi.is_contiguous()
    assert np.array_equal(engine.propagate_labels(vp, vi, threshold=3000).cpu().numpy(), want("37x53", 1)[0])
    for shape in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        z = torch.zeros(shape, dtype=torch.uint16, device=dp.device)
        empty, dist = engine.propagate_labels(z, z.clone(), return_distances=True)
        assert tuple(empty.shape) == shape and empty.dtype == torch.uint16 and tuple(dist.shape) == shape and dist.dtype == torch.uint64
        assert engine.propagate_stats == (0, 0)


def test_c_entry(engine):
    import ctypes

    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr, to_device_u16

    lib, h = engine.lib, engine.ctx.handle
    primary, image = CASES["37x53"][0]
    dp, di = to_device_u16(primary), to_device_u16(image)
    F, Y, X = primary.shape
    L = ref.lambda2()
    need = int(lib.aliby_propagate_workspace_bytes(F, Y, X))
    assert need == 32 * F * Y * X + 256 and int(lib.aliby_propagate_workspace_bytes(0, Y, X)) == 0
    work = torch.empty(need // 8 + 1, dtype=torch.int64, device=dp.device)
    out = torch.full_like(dp, 77)
    dist = torch.full(dp.shape, 77, dtype=torch.int64, device=dp.device)
    stats = (ctypes.c_int32 * 2)(-1, -1)

    def call(p=None, i=None, shape=(F, Y, X), thr=3000, lam=L, n=0, w=None, nbytes=need, o=None, d=None, st=None):
        return lib.aliby_propagate_labels(h, _ptr(dp) if p is None else p, _ptr(di) if i is None else i, *shape, thr, lam, n,
                                          _ptr(work) if w is None else w, nbytes, _ptr(out) if o is None else o, _ptr(dist) if d is None else d,
                                          st, _stream_ptr())

    _lib.check(call(st=stats))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want("37x53", 1)[0]) and np.array_equal(dist.cpu().numpy().view(np.uint64), want("37x53", 1)[1])
    assert stats[0] >= 1 and stats[1] >= 1
    out.fill_(77)
    _lib.check(call(d=0))  # no distances asked
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want("37x53", 1)[0])
    out.fill_(77)
    dist.fill_(77)
    with pytest.raises(ValueError, match="alias"):
        _lib.check(call(o=_ptr(dp)))
    with pytest.raises(ValueError, match="workspace"):  # one byte short
        _lib.check(call(nbytes=need - 1))
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(call(w=0))
    with pytest.raises(ValueError, match="8-byte aligned"):
        _lib.check(call(w=work.data_ptr() + 4))
    for bad in (-1, 65536):
        with pytest.raises(ValueError, match="threshold"):
            _lib.check(call(thr=bad))
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="distance"):
            _lib.check(call(n=bad))
    with pytest.raises(ValueError, match="lambda2"):
        _lib.check(call(lam=(1 << 40) + 1))
    with pytest.raises(ValueError, match="2\\^23"):  # by its arguments alone: nothing of that size exists
        _lib.check(call(shape=(1, 4096, 2049)))
    with pytest.raises(ValueError):
        _lib.check(call(shape=(-1, Y, X)))
    # zero pixels: a successful no-op that touches nothing, with no buffers at all
    for shape in ((0, Y, X), (F, 0, X), (F, Y, 0)):
        _lib.check(lib.aliby_propagate_labels(h, 0, 0, *shape, 0, L, 0, 0, 0, 0, 0, None, _stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 77).all() and (dist == 77).all()  # no refused call wrote anything
    assert np.array_equal(dp.cpu().numpy(), primary) and np.array_equal(di.cpu().numpy(), image)


def test_host_forms(engine):
    from aliby_amd import devcache
    from aliby_amd.extraction import extract, functions

    primary, image = CASES["3x64x96"][0]
    exp = want("3x64x96", 1)[0]
    one = functions.propagate_objects(primary[0], image[0], threshold=3000)
    assert isinstance(one, np.ndarray) and one.dtype == np.uint16 and np.array_equal(one, exp[0])
    with pytest.raises(ValueError):
        functions.propagate_objects(primary, image[0])  # one tile
    with pytest.raises(ValueError, match="float32"):
        functions.propagate_objects(primary[0], image[0].astype(np.float32))
    with pytest.raises(ValueError):
        functions.propagate_objects(primary[0], image[0], distance=0)

    # [F,C,Z,Y,X] pixels whose channel 1, max-projected over Z, is the image
    rng = np.random.default_rng(3)
    pixels = rng.integers(0, 500, (3, 2, 3, 64, 96)).astype(np.uint16)
    pixels[:, 1] = np.minimum(pixels[:, 1], image[:, None])
    pixels[:, 1, 1] = image
    tile = extract.propagate_masks(primary[1], pixels[1:2], 1, threshold=3000)
    assert isinstance(tile, np.ndarray) and tile.shape == primary[1].shape and np.array_equal(tile, exp[1])
    per_tile = extract.propagate_masks([t for t in primary], pixels, 1, threshold=3000, who="a test")
    assert isinstance(per_tile, list) and len(per_tile) == 3
    for k, t in enumerate(per_tile):
        assert t.dtype == np.uint16 and np.array_equal(t, exp[k])
    for t in (tile, *per_tile):  # the device copy travels with the host image, as a segment step's does
        hit = devcache.lookup(t)
        assert hit is not None and np.array_equal(hit[0].cpu().numpy().reshape(t.shape), t)
    with pytest.raises(ValueError):
        extract.propagate_masks([], pixels, 1)
    with pytest.raises(ValueError, match="channel"):
        extract.propagate_masks([t for t in primary], pixels, 2)
    with pytest.raises(ValueError, match="float32"):
        extract.propagate_masks([t for t in primary], pixels.astype(np.float32), 1)
    with pytest.raises(ValueError, match="do not match"):
        extract.propagate_masks([t for t in primary[:2]], pixels, 1)
    with pytest.raises(ValueError, match="1..64"):
        extract.propagate_masks(primary[0], pixels[:1], 1, distance=65)
