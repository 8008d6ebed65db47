"""
TEST INFRASTRUCTURE — a NumPy restatement of `projection3d` (include/aliby_hip.h, aliby_features_projection3d), written from the
definitions and sharing no code with the kernels, and the hand cases both tests/test_cpu_projection3d_ref.py and
tests/test_gpu_projection3d.py run.

For a column (f, y, x) of volume labels [F, Z, Y, X], `top` is the maximum over z.  Per label L of 1..counts[f]:
  Projection_Area            columns that hold a voxel of L (once per column)
  Projection_VisibleArea     columns whose top is L
  Projection_VisibleFraction VisibleArea / Area in float64, NaN when Area is 0
  Projection_Label           the 1-based rank of L among the distinct non-zero tops of the stack, 0 when L is no column's top
`projection3d` checks its labels against the collapse itself: max(axis=0), then the oracle's sequential relabel.
"""
import numpy as np

from oracle import tiler_ref


def collapse(stack):
    """[Z,Y,X] -> [Y,X]: what a 3-D segment step returns (segment/dispatch.py:218-223)."""
    return tiler_ref.relabel_sequential(np.asarray(stack).max(axis=0))


def projection3d_stack(stack, count):
    """One stack [Z,Y,X] -> float64 [count, 4]."""
    stack = np.asarray(stack).astype(np.int64)
    top = stack.max(axis=0)
    present = [int(v) for v in np.unique(top) if v != 0]
    flat = collapse(stack)
    out = np.zeros((int(count), 4), np.float64)
    for L in range(1, int(count) + 1):
        area = int((stack == L).any(axis=0).sum())
        visible = int((top == L).sum())
        label = present.index(L) + 1 if L in present else 0
        # the rank is the value the object carries in the collapsed image: the columns whose top it is hold exactly that value
        assert (label == 0 and visible == 0) or np.array_equal(flat == label, top == L)
        out[L - 1] = (area, visible, np.float64(visible) / np.float64(area) if area else np.nan, label)
    return out


def projection3d(volume, counts):
    """[F,Z,Y,X], counts [F] -> float64 [sum counts, 4], rows in (stack, label) order."""
    volume = np.asarray(volume)
    blocks = [projection3d_stack(volume[f], counts[f]) for f in range(volume.shape[0])]
    return np.concatenate(blocks, 0) if blocks else np.zeros((0, 4))


# ------------------------------------------------------------------------------------------------ hand cases
def _stack(shape=(4, 5, 6)):
    return np.zeros(shape, np.uint16)


def hand_cases():
    """name -> (volume uint16 [F,Z,Y,X], counts [F], expected float64 [sum counts, 4] written out by hand).  Stacks of at most
    4 x 5 x 6."""
    nan = float("nan")
    c = {}

    v = _stack()
    v[2, 3, 4] = 1
    c["single_voxel"] = (v[None], [1], [[1, 1, 1.0, 1]])

    v = _stack()
    v[0, 1:3, 1:4] = 1  # six columns, every one of them under label 2
    v[2, 0:4, 0:5] = 2
    c["lower_value_fully_hidden"] = (v[None], [2], [[6, 0, 0.0, 0], [20, 20, 1.0, 1]])

    v = _stack()
    v[1, 0:2, 0:4] = 1  # eight columns, the four at x 2..3 under label 3
    v[3, 0:2, 2:6] = 3
    v[0, 4, 5] = 2
    c["partly_hidden"] = (v[None], [3], [[8, 4, 0.5, 1], [1, 1, 1.0, 2], [8, 8, 1.0, 3]])

    v = _stack()
    v[0, 2, 2] = v[2, 2, 2] = 2  # background in between
    v[0, 2, 3] = v[3, 2, 3] = 2  # another label in between, which hides it there
    v[1, 2, 3] = v[2, 2, 3] = 3
    v[0:4, 0, 0] = (1, 2, 3, 1)  # a third and a fourth label of a column, the fourth a re-entry
    c["reentry_counts_once"] = (v[None], [3], [[1, 0, 0.0, 0], [3, 1, 1 / 3, 1], [2, 2, 1.0, 2]])

    v = _stack()
    v[1, 1, 1:3] = 1
    v[1, 3, 1:4] = 3
    c["label_without_voxels"] = (v[None], [4], [[2, 2, 1.0, 1], [0, 0, nan, 0], [3, 3, 1.0, 2], [0, 0, nan, 0]])

    v = _stack()
    v[0, 0, 0:3] = 1
    v[1, 0, 2] = 2
    v[2, 0, 1:3] = 9   # above counts: hides label 1 at x 1 and labels 1, 2 at x 2
    v[0, 4, 0:2] = 3
    v[3, 4, 5] = 2
    c["value_above_counts"] = (v[None], [3], [[3, 1, 1 / 3, 1], [2, 1, 0.5, 2], [2, 2, 1.0, 3]])

    v = _stack((1, 5, 6))
    v[0, 0, 0:2] = 2
    v[0, 2, 0:3] = 5
    v[0, 4, 5] = 3
    c["one_plane"] = (v[None], [5], [[0, 0, nan, 0], [2, 2, 1.0, 1], [1, 1, 1.0, 2], [0, 0, nan, 0], [3, 3, 1.0, 3]])

    a, b = _stack(), _stack()
    a[0, 0, 0:2] = 1
    a[1, 0, 1:3] = 2
    b[3, 4, 0:6] = 1
    b[0, 4, 0] = 3  # above the second stack's count: hides label 1 in one column
    b[1, 1, 1] = 3
    c["two_stacks"] = (np.stack([a, b]), [2, 1], [[2, 1, 0.5, 1], [2, 2, 1.0, 2], [6, 5, 5 / 6, 1]])

    c["no_objects"] = (_stack()[None], [0], np.zeros((0, 4)))
    return {k: (vol, np.asarray(cnt, np.int64), np.asarray(exp, np.float64).reshape(-1, 4)) for k, (vol, cnt, exp) in c.items()}


def same_rows(got, want) -> bool:
    """Bit for bit: integers exact, the fraction compared with ==, NaN where NaN is expected."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
