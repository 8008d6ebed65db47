"""
The plain references of tests/stager_ref.py held against independent code: NumPy's own np.pad (through
oracle/tiler_ref.if_out_of_bounds_pad), ufunc.reduce where NumPy folds left, scipy.ndimage.find_objects and np.bincount.
No GPU: what the GPU suites compare the kernels with has to be right first.
"""

import numpy as np
import pytest

from oracle import tiler_ref
from tests import stager_ref


def value_stacks(rng, shape):
    """Stacks whose lines tie and whose even medians land on x.5 at both ends of the uint16 range, and a generic one."""
    return {
        "low": rng.integers(0, 4, size=shape).astype(np.uint16),
        "high": rng.integers(65533, 65536, size=shape).astype(np.uint16),
        "wide": rng.integers(0, 65536, size=shape).astype(np.uint16),
    }


@pytest.mark.parametrize("kind", ["low", "high", "wide"])
def test_crop_pad_is_np_pad_median(kind):
    rng = np.random.default_rng({"low": 1, "high": 2, "wide": 3}[kind])
    n_pad = n_nan = n_raise = 0
    for trial in range(120):
        Y, X = int(rng.integers(5, 40)), int(rng.integers(5, 40))
        stack = value_stacks(rng, (2, 2, Y, X))[kind]
        # every fourth trial: a tall or a wide window, the shapes at which a window off the frame can escape the NaN rule
        h, w = (int(rng.integers(2, 24)), int(rng.integers(2, 24))) if trial % 4 else [(32, 4), (4, 32)][(trial // 4) % 2]
        y0, x0 = int(rng.integers(-h, Y + 1)), int(rng.integers(-w, X + 1))
        if trial % 3:  # two in three: a little over one edge per axis or none, the padded and unflagged case
            y0 = [-int(rng.integers(0, h // 4 + 1)), Y - h + int(rng.integers(0, w // 4 + 1))][int(rng.integers(2))]
            x0 = [-int(rng.integers(0, h // 4 + 1)), X - w + int(rng.integers(0, w // 4 + 1))][int(rng.integers(2))]
        rg = (slice(y0, y0 + h), slice(x0, x0 + w))
        if y0 + h < 0 or x0 + w < 0:
            # a negative slice stop counts from the far edge in Python: the restated reference no longer cuts this window (the
            # tile it returns has another shape).  Only the rule itself is left to check: flagged, or refused.
            if stager_ref.nan_rule(Y, X, (y0, x0, h, w))[0]:
                assert stager_ref.crop_pad(stack, (y0, x0, h, w)) is None
            else:
                with pytest.raises(ValueError, match="does not overlap"):
                    stager_ref.crop_pad(stack, (y0, x0, h, w))
            continue
        try:
            want = [tiler_ref.if_out_of_bounds_pad(stack[c], rg) for c in range(2)]
        except ValueError:
            with pytest.raises(ValueError, match="does not overlap"):
                stager_ref.crop_pad(stack, (y0, x0, h, w))
            n_raise += 1
            continue
        got = stager_ref.crop_pad(stack, (y0, x0, h, w))
        if np.isnan(want[0]).any():
            assert got is None, (trial, y0, x0, h, w, Y, X)
            n_nan += 1
            continue
        assert got is not None and got.dtype == np.uint16 and got.shape == (2, 2, h, w)
        for c in range(2):
            assert want[c].dtype == np.uint16 and np.array_equal(got[c], want[c]), (trial, c, y0, x0, h, w, Y, X)
        n_pad += stager_ref.nan_rule(Y, X, (y0, x0, h, w))[1] != (0, 0, 0, 0)
    assert n_pad >= 25 and n_nan >= 10, (n_pad, n_nan, n_raise)  # (the draw reaches every branch)


def test_crop_pad_refuses_what_np_pad_refuses():
    stack = np.arange(2 * 100 * 80, dtype=np.uint16).reshape(2, 1, 100, 80)
    for rect in ((0, -16, 64, 16), (100, 0, 16, 64), (7, -4, 16, 4), (100, 3, 4, 16), (101, 3, 4, 64)):
        y0, x0, h, w = rect
        with pytest.raises(ValueError):
            tiler_ref.if_out_of_bounds_pad(stack[0], (slice(y0, y0 + h), slice(x0, x0 + w)))
        with pytest.raises(ValueError, match="does not overlap"):
            stager_ref.crop_pad(stack, rect)
    # wholly above / right of the frame, and the near misses of the two cases above: NaN tiles, no error
    for rect in ((-64, 0, 64, 16), (0, 80, 16, 64), (0, -16, 63, 16), (100, 0, 16, 63)):
        assert stager_ref.crop_pad(stack, rect) is None
        y0, x0, h, w = rect
        assert np.isnan(tiler_ref.if_out_of_bounds_pad(stack[0], (slice(y0, y0 + h), slice(x0, x0 + w)))).all()


def test_corner_sees_the_rows_the_y_pass_made():
    """Hanging over a corner, the x pass takes the median of a padded row from the y pass's values: the corner differs
    from what medians of the original columns alone would give."""
    yy, xx = np.mgrid[:12, :12]
    stack = (1000 * yy * yy + 7 * xx * xx * xx).astype(np.uint16)[None, None]
    rect = (-2, -2, 8, 8)
    got = stager_ref.crop_pad(stack, rect)
    want = tiler_ref.if_out_of_bounds_pad(stack[0], (slice(-2, 6), slice(-2, 6)))
    assert np.array_equal(got[0], want)
    col_med = stager_ref._line_median(stack[..., 0:6, 0:6], axis=-2)  # the y pass's values
    assert got[0, 0, 0, 0] == stager_ref._line_median(col_med, axis=-1)[0, 0, 0, 0]
    assert got[0, 0, 0, 0] != stager_ref._line_median(stack[..., 0:1, 0:6], axis=-1)[0, 0, 0, 0]  # not row 0's own median


def test_half_to_even_table():
    pairs = [(1, 2), (2, 3), (3, 4), (65534, 65535), (0, 1)]
    want = [2, 2, 4, 65534, 0]
    assert [int(stager_ref.round_half_even_mean(a, b)) for a, b in pairs] == want
    for (a, b), m in zip(pairs, want):
        line = np.array([[b, a]], np.uint16)
        assert int(stager_ref._line_median(line, axis=-1)[0, 0]) == m
        assert int(np.pad(np.array([a, b], np.uint16), (1, 0), "median")[0]) == m  # NumPy's own rounding
    assert int(stager_ref._line_median(np.array([[5, 1, 9]], np.uint16), axis=-1)[0, 0]) == 5
    assert int(stager_ref._line_median(np.array([[65535, 65535, 0, 65535]], np.uint16), axis=-1)[0, 0]) == 65535


@pytest.mark.parametrize("op,ufunc", [("max", np.maximum), ("add", np.add), ("div", np.divide)])
def test_reduce_fold_is_ufunc_reduce_where_numpy_folds_left(op, ufunc):
    rng = np.random.default_rng(4)
    for shape in ((3, 5, 40), (1, 1, 7), (2, 2, 3), (2, 9, 4, 5)):
        u = rng.integers(0, 65536, size=shape).astype(np.uint16)
        u.flat[::7] = 0
        u.flat[3::11] = 65535
        f = (rng.standard_normal(shape) * 1e3).astype(np.float32)
        f.flat[::13] = 0
        for a in (u, f):
            with np.errstate(all="ignore"):
                want = ufunc.reduce(a, axis=1)
            got = stager_ref.reduce_fold(a, op, axis=1)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert np.array_equal(got, want, equal_nan=True), (op, shape, a.dtype)


def test_reduce_fold_max_propagates_nan_and_add_is_not_pairwise():
    a = np.array([[1, np.nan, 2], [np.nan, 1, 2], [1, 2, np.nan], [np.inf, -np.inf, 3], [-np.inf, -np.inf, -np.inf]], np.float32).T[None]
    got = stager_ref.reduce_fold(a, "max", axis=1)  # [1, 5]
    assert np.isnan(got[0, :3]).all() and got[0, 3] == np.inf and got[0, 4] == -np.inf
    assert np.array_equal(got, np.maximum.reduce(a, axis=1), equal_nan=True)
    # over a contiguous last axis NumPy adds pairwise: the explicit fold is the definition the kernel is held to
    rng = np.random.default_rng(0)
    b = (rng.standard_normal((3, 64, 1)) * 1e4).astype(np.float32)
    fold = b[:, 0].copy()
    for z in range(1, 64):
        fold = fold + b[:, z]
    assert np.array_equal(stager_ref.reduce_fold(b, "add", axis=1), fold)


def test_object_rows_is_find_objects_and_bincount():
    from scipy import ndimage as ndi

    rng = np.random.default_rng(6)
    for trial in range(30):
        F, Y, X = int(rng.integers(1, 4)), int(rng.integers(1, 30)), int(rng.integers(1, 30))
        lab = rng.integers(0, int(rng.integers(1, 12)), size=(F, Y, X)).astype(np.uint16)
        lab[lab == 3] = 0  # a gap
        if trial % 5 == 0:
            lab[F - 1] = 0
        true_max = [int(l.max()) for l in lab]
        for mx in (None, [m + 2 for m in true_max], [max(m - 2, 0) for m in true_max]):
            rows, off = stager_ref.object_rows(lab, mx)
            use = true_max if mx is None else mx
            assert off.tolist() == [0] + np.cumsum(use).tolist() and len(rows) == sum(use)
            for f in range(F):
                r = rows[off[f]:off[f + 1]]
                assert (r["tile"] == f).all() and r["label"].tolist() == list(range(1, use[f] + 1))
                sl = ndi.find_objects(lab[f].astype(np.int32), max_label=use[f])
                counts = np.bincount(lab[f].ravel(), minlength=use[f] + 1)
                for row, s in zip(r, sl):
                    assert row["area"] == counts[row["label"]]
                    if s is None:
                        assert row["area"] == 0 and (row["y0"], row["x0"], row["y1"], row["x1"]) == (-1, -1, -1, -1)
                    else:
                        assert (row["y0"], row["x0"], row["y1"], row["x1"]) == (s[0].start, s[1].start, s[0].stop, s[1].stop)
