"""
csrc/stager.hip (aliby_crop_pad_u16, aliby_reduce_z) and segnet.hip's aliby_select_project_u16 through the C ABI, bit for bit
against tests/stager_ref.py, at shapes that reach every launch path: the 16-byte copy and its partial groups, the second pass of
every grid-stride loop, sort lines longer than the block, lines without a sort sentinel, every reduce_z instantiation.

Every output block starts as a sentinel the stack cannot hold (the tiler allocates with torch.empty): none is left in a tile that
is not flagged, and a flagged tile is still all sentinel.
"""

import functools

import numpy as np
import pytest

from tests import stager_ref

pytestmark = pytest.mark.gpu


def crop_call(engine, dev, shape, rects, h, w, sentinel):
    """aliby_crop_pad_u16 on the device stack `dev` ([C,Z,Y,X] = shape) -> (status, out [F,C,Z,h,w], flags)."""
    import torch
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    C, Z, Y, X = shape
    rects = np.ascontiguousarray([[r[0], r[1], h, w] for r in rects], dtype=np.int32)
    out = torch.from_numpy(np.full((len(rects), C, Z, h, w), sentinel, np.uint16)).cuda()
    flags = np.zeros(len(rects), np.int32)
    rc = engine.lib.aliby_crop_pad_u16(engine.ctx.handle, _ptr(dev), C, Z, Y, X, _ptr(rects), len(rects), h, w, _ptr(out), _ptr(flags),
                                       _stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), flags


def check_crop(engine, stack, windows, h, w, sentinel=65535, dev=None):
    """Every window (y0, x0) of `stack` equals the reference's tile, or is flagged and untouched.  Returns the flags."""
    import torch
    from aliby_amd import _lib

    assert not (stack == sentinel).any()
    if dev is None:
        dev = torch.from_numpy(stack).cuda()
    rc, got, flags = crop_call(engine, dev, stack.shape, windows, h, w, sentinel)
    _lib.check(rc)
    for f, (y0, x0) in enumerate(windows):
        want = stager_ref.crop_pad(stack, (y0, x0, h, w))
        if want is None:
            assert flags[f] == 1 and (got[f] == sentinel).all(), (f, y0, x0)
        else:
            assert flags[f] == 0, (f, y0, x0)
            assert not (got[f] == sentinel).any(), (f, y0, x0, "pixels never written")
            assert np.array_equal(got[f], want), (f, y0, x0, np.argwhere(got[f] != want)[:4].tolist())
    return flags.tolist()


def unaligned_copy(stack):
    """The same stack on the device behind a data pointer that is 2-byte but not 16-byte aligned."""
    import torch

    flat = torch.zeros(stack.size + 1, dtype=torch.uint16, device="cuda")
    view = flat[1:].view(stack.shape)
    view.copy_(torch.from_numpy(stack))
    assert view.data_ptr() % 16 == 2
    return view


# ------------------------------------------------------------------------------------------------------------ crop + median pad
VECTOR_WINDOWS = [(y0, x0) for y0 in (0, -8, 72) for x0 in (0, 8, 96, -8, 104)]


@functools.lru_cache(maxsize=None)
def vector_stack():
    return np.random.default_rng(21).integers(0, 65535, size=(2, 1, 96, 128), dtype=np.uint16)


def test_crop_vector_path_and_partial_groups(engine):
    """k_crop_copy's 16-byte path (w, X, x0 multiples of 8, aligned bases): x0 = -8 and 104 put a whole group across the frame's
    left / right edge — the partial-group branch; y0 = -8 and 72 add the row test above and below."""
    flags = check_crop(engine, vector_stack(), VECTOR_WINDOWS, 32, 32)
    assert flags == [0] * 15  # 8 of 32 outside: exactly the 25 % the reference still pads


def test_crop_scalar_fallback_odd_origin(engine):
    """The same windows one pixel to the right: x0 % 8 != 0 sends every tile down the pixel loop (x0 = 105 hangs 9 of 32 over
    the edge: flagged, left untouched)."""
    flags = check_crop(engine, vector_stack(), [(y0, x0 + 1) for y0, x0 in VECTOR_WINDOWS], 32, 32)
    assert flags == [0, 0, 0, 0, 1] * 3


def test_crop_scalar_fallback_unaligned_stack(engine):
    """The vector windows on a stack whose data pointer is only 2-byte aligned: the base test of the 16-byte path fails."""
    stack = vector_stack()
    assert check_crop(engine, stack, VECTOR_WINDOWS, 32, 32, dev=unaligned_copy(stack)) == [0] * 15


@functools.lru_cache(maxsize=None)
def big_stack():
    return np.random.default_rng(22).integers(0, 65535, size=(1, 1, 400, 400), dtype=np.uint16)


def test_crop_grid_stride_vector_and_long_sort_lines(engine):
    """Tile 368 x 368 = 135 424 pixels > the 131 072 one pass of k_crop_copy's vector loop covers (64 blocks x 256 lanes x 8).
    Hanging 40 rows over the top leaves 328 inside rows in a 512-slot sort line: 256 pairs for 128 threads, the pair loop of
    block_bitonic_sort strides.  Windows over no edge, one edge, and two adjacent edges (x lines of 344 and 352)."""
    windows = [(16, 16), (-40, 16), (32, 56), (-40, -16), (72, 56), (72, -24)]
    assert check_crop(engine, big_stack(), windows, 368, 368) == [0] * 6


def test_crop_sort_line_without_sentinel(engine):
    """Tile 320 x 320 hanging 64 over an edge leaves exactly 256 inside rows / columns: n == n2, no 0xFFFF fills the sort line.
    (A 368-row tile cannot get there: 112 rows outside is past the 25 % rule.)"""
    windows = [(-64, 40), (144, 40), (40, -64), (40, 144), (-64, 144)]
    assert check_crop(engine, big_stack(), windows, 320, 320) == [0] * 5


def test_crop_grid_stride_scalar(engine):
    """Tile 136 x 136 = 18 496 pixels > the 16 384 one pass of the pixel loop covers (64 blocks x 256), at odd x0."""
    windows = [(10, 11), (-30, 11), (100, -33), (284, 285), (-34, 285), (264, 1)]
    assert check_crop(engine, big_stack(), windows, 136, 136) == [0] * 6


def rounding_stacks():
    rng = np.random.default_rng(23)
    shape = (1, 2, 40, 48)
    yy, xx = np.mgrid[:40, :48]
    half = rng.integers(0, 10, size=shape).astype(np.uint16)
    half[..., (yy + xx) % 2 == 0] = 0xFFFF  # every line: half its values are 0xFFFF
    return {
        "low": rng.integers(0, 4, size=shape).astype(np.uint16),
        "high": rng.integers(65533, 65536, size=shape).astype(np.uint16),
        "all_ffff": np.full(shape, 0xFFFF, np.uint16),
        "half_ffff": half,
    }


@pytest.mark.parametrize("kind", ["low", "high", "all_ffff", "half_ffff"])
def test_crop_median_rounding_and_the_sort_sentinel(engine, kind):
    """median_round_u16 on ties and x.5 sums (half to even, at both ends of the range), and real 0xFFFF values next to the 0xFFFF
    that fills a sort line up to its power of two.  Inside counts 19 (odd) and 18 (even) per axis, alone and at the corners."""
    stack = rounding_stacks()[kind]
    windows = [(-5, 8), (-6, 8), (21, 8), (22, 8), (8, -5), (8, -6), (8, 29), (8, 30), (-5, 30), (22, -6), (-6, -5), (21, 29)]
    assert check_crop(engine, stack, windows, 24, 24, sentinel=1234) == [0] * 12


def test_crop_corner_takes_the_x_median_of_the_padded_rows(engine):
    """Over a corner the x pass must see the rows the y pass made.  On a random stack every row and column has its own median
    and the median of the column medians is not the median of the row medians, so the other order of the passes gives other
    corner pixels: checked on the reference first."""
    stack = np.random.default_rng(24).integers(0, 65535, size=(1, 1, 50, 60), dtype=np.uint16)
    h = w = 32
    for y0, x0 in ((-7, -6), (-8, 34), (25, -5), (24, 35)):
        want = stager_ref.crop_pad(stack, (y0, x0, h, w))
        other = np.swapaxes(stager_ref.crop_pad(np.swapaxes(stack, -1, -2), (x0, y0, w, h)), -1, -2)  # x pass first
        assert not np.array_equal(want, other)
    assert check_crop(engine, stack, [(-7, -6), (-8, 34), (25, -5), (24, 35)], h, w) == [0] * 4


@pytest.mark.parametrize("h,w,bad", [(64, 16, (0, -16)), (16, 64, (96, 0))])
def test_crop_refuses_a_window_off_the_frame_that_is_no_nan_tile(engine, h, w, bad):
    """Wholly left of the frame with h >= 4 w, wholly below it with w >= 4 h: past the NaN rule (before-pads meet h, after-pads
    meet w) with nothing to take a median of.  The host refuses the call, alone and among valid windows; nothing is written."""
    import torch

    stack = vector_stack()
    dev = torch.from_numpy(stack).cuda()
    with pytest.raises(ValueError):
        stager_ref.crop_pad(stack, (*bad, h, w))
    assert stager_ref.nan_rule(96, 128, (*bad, h, w))[0] is False
    for windows in ([bad], [(8, 8), bad, (16, 40)]):
        rc, got, flags = crop_call(engine, dev, stack.shape, windows, h, w, 65535)
        assert rc == 1  # ALIBY_ERR_INVALID
        msg = engine.lib.aliby_last_error().decode()
        assert f"window {windows.index(bad)} (y0={bad[0]}, x0={bad[1]}, h={h}, w={w})" in msg, msg
        assert (got == 65535).all()
    # the same valid windows alone go through
    assert check_crop(engine, stack, [(8, 8), (16, 40)], h, w, dev=dev) == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ reduce_z
REDUCE_SHAPES = [(3, 5, 1551), (1, 1, 77), (2, 2, 1), (1, 2, 2_100_000)]
# (input dtype, operator, output dtype code name, NumPy's own result dtype)
INSTANTIATIONS = [
    ("u16", "max", "U16"), ("u16", "add", "U64"), ("u16", "add", "F32"), ("u16", "div", "F64"), ("u16", "div", "F32"),
    ("f32", "max", "F32"), ("f32", "add", "F32"), ("f32", "div", "F32"),
]
OUT_NP = {"U16": np.uint16, "U64": np.uint64, "F32": np.float32, "F64": np.float64}


def nan_positions(shape):
    """(outer, z, inner) of a NaN in the first, a middle and the last plane of three different pixels."""
    outer, Z, inner = shape
    return [(0, 0, 10 % inner), (outer - 1, Z // 2, 20 % inner), (outer // 2, Z - 1, 30 % inner)]


@functools.lru_cache(maxsize=None)
def reduce_input(shape, dtype):
    rng = np.random.default_rng(31)
    outer, Z, inner = shape
    if dtype == "u16":
        a = rng.integers(0, 65536, size=shape).astype(np.uint16)
        a.reshape(-1)[::5] = 0  # x / 0 and 0 / 0 in the divide chains
        a.reshape(-1)[3::7] = 65535
        return a
    a = (rng.standard_normal(shape) * 100).astype(np.float32)
    a.reshape(-1)[::5] = 0
    a[0, 0, 40 % inner] = np.inf
    a[outer - 1, :, 50 % inner] = -np.inf
    a[0, Z - 1, 60 % inner] = -np.inf
    for o, z, k in nan_positions(shape):  # (last: on the one-pixel shape they share pixels with the infinities)
        a[o, z, k] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def reduce_reference(shape, dtype, op):
    want = stager_ref.reduce_fold(reduce_input(shape, dtype), op, axis=1)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,op,out", INSTANTIATIONS, ids=lambda v: str(v))
def test_reduce_z_every_instantiation(engine, shape, dtype, op, out):
    """Each k_reduce_z<TI, TO, OP> against the explicit left fold: (3, 5, 1551) is the usual multi-block shape, (1, 1, 77) has
    Z == 1 (the fold loops never run), (2, 2, 1) has inner == 1, and (1, 2, 2 100 000) > 2 097 152 = 8 192 blocks x 256 reaches
    the second pass of the grid-stride loop.  uint16 data holds 0 and 65535 (x / 0, 0 / 0), f32 data NaN, +inf and -inf.  The
    f32-narrowed outputs round NumPy's u64 / f64 result once, as the kernel does."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    a = reduce_input(shape, dtype)
    outer, Z, inner = shape
    want = reduce_reference(shape, dtype, op)
    np_out = OUT_NP[out]
    with np.errstate(over="ignore"):
        want = want.astype(np_out)  # (a no-op unless the output is the f32 narrowing)
    dev = torch.from_numpy(a).cuda()
    buf = torch.from_numpy(np.full(outer * inner * np.dtype(np_out).itemsize, 0xA5, np.uint8)).cuda()
    _lib.check(engine.lib.aliby_reduce_z(engine.ctx.handle, _ptr(dev), _lib.U16 if dtype == "u16" else _lib.F32, outer, Z, inner,
                                         {"max": _lib.RED_MAX, "add": _lib.RED_ADD, "div": _lib.RED_DIV}[op], _ptr(buf),
                                         getattr(_lib, out), _stream_ptr()))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np_out).reshape(outer, inner)
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4].tolist()
    if dtype == "f32" and op == "max":
        for o, z, k in nan_positions(shape):
            assert np.isnan(got[o, k]), (o, z, k)


def test_reduce_z_host_function_propagates_nan(engine):
    """functions.reduce_z promises ufunc.reduce: np.maximum.reduce gives NaN wherever a plane holds one."""
    from aliby_amd.extraction.functions import reduce_z

    a = np.moveaxis(reduce_input((3, 5, 1551), "f32"), 1, 0).reshape(5, 3 * 33, 47).copy()  # [Z, Y, X]
    want = np.maximum.reduce(a, axis=0)
    assert np.isnan(want).sum() == 3
    got = reduce_z(a, np.maximum)
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    line = np.array([1, np.nan, 2], np.float32).reshape(3, 1, 1) * np.ones((1, 2, 2), np.float32)
    assert np.isnan(reduce_z(line, np.maximum)).all()


# ------------------------------------------------------------------------------------------------------------ select_project
def select_project(engine, pixels, channel, sentinel=65535):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    F, C, Z, Y, X = pixels.shape
    dev = pixels if isinstance(pixels, torch.Tensor) else torch.from_numpy(pixels).cuda()
    out = torch.from_numpy(np.full((F, Y, X), sentinel, np.uint16)).cuda()
    _lib.check(engine.lib.aliby_select_project_u16(engine.ctx.handle, _ptr(dev), F, C, Z, Y, X, channel, _ptr(out), _stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_select_project_every_channel(engine):
    import torch

    pixels = np.random.default_rng(41).integers(0, 65535, size=(2, 3, 4, 33, 47), dtype=np.uint16)
    dev = torch.from_numpy(pixels).cuda()
    for c in range(3):
        assert np.array_equal(select_project(engine, dev, c), pixels[:, c].max(axis=1)), c


def test_select_project_grid_stride(engine):
    """[1, 2, 2, 2048, 2056]: 4 210 688 outputs > 4 194 304 = 16 384 blocks x 256, the second pass of k_select_project."""
    pixels = np.random.default_rng(42).integers(0, 65535, size=(1, 2, 2, 2048, 2056), dtype=np.uint16)
    assert np.array_equal(select_project(engine, pixels, 1), pixels[:, 1].max(axis=1))
