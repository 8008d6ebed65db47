"""
Pins tests/track_ref.py, the literal reference of the IoU stitcher, without a GPU:

  * on cases worked by hand, the expected labels written out (`track_ref.hand_cases`): the two duplicate-label cases in which
    stitch3D on the relabelled frame and a per-object reading of the rule differ, IoU exactly at the threshold, a row tie of
    2/6 against 1/3, a column tie, an absent current label, a previous row tracked as 0, `max_label` on both sides of the
    largest tracked label;
  * against oracle/track_restated.py, on the same cases and on seeded random lapses.  The two files were written apart and
    count differently (relabelled image and dense matrix here, per-object overlaps summed per tracked label there).  The
    oracle used to keep previous objects that share a tracked label as separate columns; then the two agreed only on lapses
    that never hand on a duplicate, and such lapses had to be at least 90 % of the seeds for the agreement to mean anything.
    The oracle now aggregates those columns, so agreement is asserted on EVERY seed and that cap is gone; instead the test
    asserts that lapses with a duplicate do occur, so that the aggregated path is compared too.
"""
import inspect

import numpy as np
import pytest

from tests import track_ref
from oracle import track_restated, volume_restated

CASES = track_ref.hand_cases()
N_SEEDS = 200


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_on_hand_worked_cases(name):
    prev, cur, tracked, mx, thr, want, want_mx = CASES[name]
    got, got_mx = track_ref.stitch_pair(prev, cur, tracked, mx, thr)
    assert got.dtype == np.int64 and got.tolist() == want and got_mx == want_mx
    info = None if tracked is None else {0: {"labels": tracked, "max_label": mx}}
    assert track_ref.stitch_rois([[prev, cur]], info, thr) == {0: {"labels": want, "max_label": want_mx}}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_on_hand_worked_cases(name):
    prev, cur, tracked, mx, thr, want, want_mx = CASES[name]
    got, got_mx = track_restated.stitch_pair(prev, cur, tracked, mx, thr)
    assert got.tolist() == want and got_mx == want_mx


def test_hand_cases_are_what_their_names_say():
    """The ratios the cases rest on, computed here from the frames: an edit to a frame cannot turn a tie into a near miss."""
    def iou(prev, cur, p, c):
        ov = int(((prev == p) & (cur == c)).sum())
        return ov, int((cur == c).sum()), int((prev == p).sum())

    prev, cur = CASES["iou_equals_threshold"][:2]
    assert iou(prev, cur, 1, 1) == (4, 10, 10) and 4 / (10 + 10 - 4) == 0.25
    prev, cur = CASES["row_tie_own_labels"][:2]
    assert iou(prev, cur, 1, 1) == (2, 3, 5) and iou(prev, cur, 2, 1) == (1, 3, 1) and 2 / 6 == 1 / 3
    prev, cur = CASES["column_tie"][:2]
    assert iou(prev, cur, 1, 1) == (16, 16, 32) and iou(prev, cur, 1, 2) == (16, 16, 32)
    prev, cur = CASES["duplicate_bite"][:2]
    assert iou(prev, cur, 1, 1) == (16, 40, 16) and iou(prev, cur, 2, 1) == (16, 40, 16)
    prev, cur = CASES["duplicate_wide"][:2]
    assert iou(prev, cur, 1, 1) == (16, 64, 16) and iou(prev, cur, 2, 1) == (16, 64, 16)


def test_a_longer_label_list_is_cut_and_a_shorter_one_refused():
    prev, cur = CASES["column_tie"][:2]
    assert track_ref.stitch_pair(prev, cur, [3, 8, 9], 3, 0.25)[0].tolist() == [3, 3]
    assert track_ref.stitch_pair(prev, cur, [3, 8, 9], 3, 0.25)[1] == 3  # (the cut entries do not raise the running maximum)
    with pytest.raises(AssertionError):
        track_ref.stitch_pair(cur, prev, [3], 3, 0.25)


def test_reference_stands_alone():
    src = inspect.getsource(track_ref)
    assert "import oracle" not in src and "from oracle" not in src and "aliby_amd" not in src.split('"""')[2]


def test_agrees_with_the_oracle_on_random_lapses():
    """Every seed, every step, labels and running maximum (see the module docstring for the cap that this replaces)."""
    with_duplicates = 0
    for seed in range(N_SEEDS):
        frames, thr = track_ref.random_lapse(seed)
        want = track_ref.run_lapse(track_ref.stitch_rois, frames, threshold=thr)
        got = track_ref.run_lapse(track_restated.stitch_rois, frames, stitch_threshold=thr)
        assert got == want, (seed, thr)
        with_duplicates += track_ref.has_duplicates(want)
    assert with_duplicates >= N_SEEDS // 10, with_duplicates  # the generator divides cells: the aggregated path is compared


def test_stitch3d_sees_the_two_halves_as_one_object():
    """oracle/volume_restated.stitch3d sits on the oracle's stitch_pair.  `split_merge_planes`: an object splits in plane 1 and
    both halves keep label 1; in plane 2 the halves are ONE previous object of area 32, so only the better of M (24 / 80 = 0.3)
    and N (8 / 32 = 0.25) keeps label 1 and N is a second object.  Taken apart, M would win the left half's column and N the
    right half's, and both would be label 1."""
    planes, want, n_want = track_ref.split_merge_planes()
    vol, n = volume_restated.stitch3d(planes, 0.01)
    assert n == n_want and np.array_equal(vol, want)
