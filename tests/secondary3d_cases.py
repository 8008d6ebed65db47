"""The label volumes that tests/test_gpu_secondary3d.py runs through the kernels and tests/test_cpu_secondary3d_ref.py checks by hand
against the restatement (tests/secondary3d_ref.py): name -> (uint16 [F,Z,Y,X], ((N, (sz, sy, sx)), ...)).  A few dozen labelled
voxels per case, so the brute force takes a second at most.  Coordinates are (z, y, x)."""
import functools

import numpy as np

from tests import secondary3d_ref as ref

UNIT = (1, 1, 1)


def at(shape, *voxels):
    vol = np.zeros((1, *shape), np.uint16)
    for zyx, v in voxels:
        vol[(0, *zyx)] = v
    return vol


def sprinkle(shape, n_obj, seed, max_side=3):
    """[F,Z,Y,X] uint16: small boxes of random labels (repeated and non-consecutive labels, 65535 among them)."""
    rng = np.random.default_rng(seed)
    F, Z, Y, X = shape
    vol = np.zeros(shape, np.uint16)
    pool = np.concatenate([np.arange(1, 40), [255, 256, 4097, 65534, 65535]])
    for _ in range(n_obj):
        f, z, y, x = (rng.integers(0, n) for n in shape)
        d, h, w = rng.integers(1, max_side + 1, 3)
        vol[f, z:z + d, y:y + h, x:x + w] = rng.choice(pool)
    return vol


def _corners():
    vol = np.zeros((1, 5, 9, 11), np.uint16)
    for k, (z, y, x) in enumerate(np.ndindex(2, 2, 2)):
        vol[0, z * 4, y * 8, x * 10] = 65535 if k == 5 else k + 1
    return vol


def _batch_edges():
    vol = np.zeros((3, 4, 9, 40), np.uint16)
    vol[0, 3, 2:7, 3:30] = 7   # the last plane of stack 0
    vol[2, 0, 1:5, 10:38] = 4  # the first plane of stack 2; stack 1 is empty and must stay empty
    return vol


def _axis_tie(axis, first, second):
    """Two voxels 6 apart along `axis` of a 13 x 13 x 13 stack, labelled `first` and `second`: (6, 6, 6) is 3 from either."""
    a, b = [6, 6, 6], [6, 6, 6]
    a[axis], b[axis] = 3, 9
    return at((13, 13, 13), (tuple(a), first), (tuple(b), second))


def _two_axes(axis_a, axis_b, first, second):
    """(5, 5, 5) has a voxel 3 back along axis_a and one 3 on along axis_b."""
    a, b = [5, 5, 5], [5, 5, 5]
    a[axis_a], b[axis_b] = 2, 8
    return at((11, 11, 11), (tuple(a), first), (tuple(b), second))


THREE = ((3, UNIT), (5, UNIT), (64, UNIT))
ONE_FIVE_64 = ((1, UNIT), (5, UNIT), (64, UNIT))

CASES = {
    # shapes
    "one_plane": (sprinkle((1, 1, 37, 53), 9, 1), ONE_FIVE_64),
    "column_along_z": (at((40, 1, 1), ((3, 0, 0), 9), ((4, 0, 0), 2), ((20, 0, 0), 65535), ((33, 0, 0), 5), ((39, 0, 0), 1)),
                       (*ONE_FIVE_64, (6, (3, 1, 1)), (16, UNIT))),
    "column_along_y": (sprinkle((1, 1, 200, 1), 6, 3), (*ONE_FIVE_64, (60, (1, 13, 1)))),
    "column_along_x": (sprinkle((1, 1, 1, 200), 6, 2), (*ONE_FIVE_64, (60, (1, 1, 13)))),
    "3x5x7_smaller_than_every_halo": (at((3, 5, 7), ((0, 0, 0), 8), ((2, 4, 6), 3)), ((64, UNIT), (255, (4, 4, 4)), (2, UNIT))),
    "6x5x7_narrower_than_a_wave": (sprinkle((1, 6, 5, 7), 3, 4, max_side=1), ((1, UNIT), (3, UNIT), (6, (3, 1, 1)))),
    # Z crosses a z segment (32), Y a row group (8), X a 256-block
    "2x34x10x260_batch": (sprinkle((2, 34, 10, 260), 20, 6, max_side=2), ((1, UNIT), (5, UNIT), (16, UNIT), (50, (13, 5, 5)), (40, (1, 5, 5)))),
    # contents
    "all_zero": (np.zeros((1, 4, 10, 70), np.uint16), ONE_FIVE_64),
    "fully_labelled": ((np.arange(3 * 9 * 65, dtype=np.uint32).reshape(1, 3, 9, 65) % 65535 + 1).astype(np.uint16), ONE_FIVE_64),
    "65535_alone": (at((9, 20, 20), ((4, 10, 10), 65535)), ((1, UNIT), (5, UNIT), (12, (3, 1, 1)))),
    "65535_beside_1": (at((3, 3, 12), ((1, 1, 2), 1), ((1, 1, 9), 65535), ((0, 1, 9), 65535)), ((1, UNIT), (3, UNIT), (5, UNIT))),
    "eight_corners": (_corners(), ONE_FIVE_64),
    **{f"tie_along_{'zyx'[axis]}_smaller_{side}": (_axis_tie(axis, *((2, 9) if side == "first" else (9, 2))), THREE)
       for axis in range(3) for side in ("first", "second")},
    **{f"tie_{'zyx'[a]}_against_{'zyx'[b]}{'_swapped' if swap else ''}": (_two_axes(a, b, *((4, 9) if swap else (9, 4))), THREE)
       for a, b in ((0, 1), (0, 2), (1, 2)) for swap in (False, True)},
    # (1, 1, 1) is (1, 2, 2) from the first and (3, 0, 0) from the second: 1 + 4 + 4 = 9 = 9 + 0 + 0
    "diagonal_tie": (at((6, 5, 5), ((2, 3, 3), 9), ((4, 1, 1), 4)), ((3, UNIT), (2, UNIT), (64, UNIT))),
    "diagonal_tie_swapped": (at((6, 5, 5), ((2, 3, 3), 4), ((4, 1, 1), 9)), ((3, UNIT), (64, UNIT))),
    # spacing (3, 1, 1): (1, 5, 5) is one plane from the first (9) and three pixels from the second (9)
    "anisotropic_tie": (at((3, 11, 12), ((0, 5, 5), 7), ((1, 5, 8), 2)), ((3, (3, 1, 1)), (2, (3, 1, 1)), (9, (3, 1, 1)))),
    "anisotropic_tie_swapped": (at((3, 11, 12), ((0, 5, 5), 2), ((1, 5, 8), 7)), ((3, (3, 1, 1)),)),
    # N = 5: (4, 6, 6) is (4, 3, 0) from the first, 16 + 9 = 25, and (0, 0, 5) from the second, 25: the x scan has to take its last
    # step although its best distance is 25 already; (4, 6, 16) has one on either side at the last step
    "tie_at_the_last_step": (at((9, 12, 22), ((0, 3, 6), 9), ((4, 6, 11), 4), ((4, 6, 21), 6), ((8, 1, 2), 7), ((8, 11, 2), 3)),
                             ((5, UNIT), (10, (2, 2, 2)))),
    # N = 5: (0, 0, 0) is (4, 4, 0) from the one label, 32 > 25 after two axes; N = 255 on (4, 4, 4): 63 planes and 63 rows give
    # 2 * 252^2 = 127 008, more than the 16-bit field holds
    "partial_sum_above_the_limit": (at((5, 5, 3), ((4, 4, 0), 6)), ((5, UNIT), (6, UNIT))),
    "n255_on_4_4_4": (at((64, 64, 3), ((0, 0, 0), 6)), ((255, (4, 4, 4)),)),
    # N = 255 on (5, 5, 5): (0, 0, 0) is 51 voxels along x from the first, m = 65025 = N^2, and (0, 24, 45) from the second, m =
    # 25 (576 + 2025) = 65025 again: a tie at the very limit, to the smaller label
    "m_65025_is_reached": (at((1, 30, 56), ((0, 0, 51), 9), ((0, 24, 45), 4)), ((255, (5, 5, 5)), (254, (5, 5, 5)))),
    # batch
    "batch_edges": (_batch_edges(), ((1, UNIT), (5, UNIT), (6, (3, 1, 1)))),
}
PAIRS = [(name, n, spacing) for name, (_, runs) in CASES.items() for n, spacing in runs]


@functools.lru_cache(maxsize=None)
def want(name, n, spacing=UNIT):
    """The restatement of a case, computed once and read-only."""
    out = ref.secondary_volume(CASES[name][0], n, spacing)
    out.setflags(write=False)
    return out
