"""
The IoU stitcher (`aliby_track_stitch`, aliby_amd/csrc/track.hip) against its literal reference tests/track_ref.py, on the paths
the random lapses of the other tests never reach: exact ties, more than 256 current objects in a tile (the chunk carry of
k_track_newids), the 1024-slot hash of k_track_candidates (probing, full, overflowing), the 16-slot candidate list, previous
objects that share a tracked label (one group: one key, summed overlap and area, one column), recovery after a refusal, awkward
shapes and the Python front end.  Every comparison is integer equality, through `StitchTracker` and through
`engine.track_stitch`; the limits 1024 and 16 are TRK_SLOTS and TRK_K of the source.

The overflow cases provoke no fault: the kernel's probing is bounded by the table size, a candidate slot is written only below
TRK_K, and the entry reports a status.
"""
import numpy as np
import pytest
import torch

from aliby_amd._lib import AlibyHipError
from aliby_amd.extraction.engine import to_device_u16
from aliby_amd.track.stitch import StitchTracker
from oracle import volume_restated
from tests import track_ref
from tests.track_ref import _frame

pytestmark = pytest.mark.gpu


def _through_engine(engine, masks, info, thr):
    """`engine.track_stitch` itself, tables and tracked labels laid out as StitchTracker lays them out."""
    prev = to_device_u16(np.stack([m[0] for m in masks]))
    cur = to_device_u16(np.stack([m[1] for m in masks]))
    tp, tc = engine.object_table(prev), engine.object_table(cur)
    tracked = mx = None
    if info:
        flat = np.zeros(max(tp.n_obj, 1), np.int32)
        mx = np.zeros(len(masks), np.int32)
        for k in range(len(masks)):
            n_k = int(tp.offsets[k + 1] - tp.offsets[k])
            flat[tp.offsets[k]: tp.offsets[k + 1]] = np.asarray(info[k]["labels"], np.int32)[:n_k]
            mx[k] = info[k]["max_label"]
        tracked = torch.from_numpy(flat).cuda()
    out, mx_out = engine.track_stitch(prev, cur, tp, tc, tracked, mx, thr)
    host = out.cpu().numpy()
    return {k: {"labels": [int(v) for v in host[tc.offsets[k]: tc.offsets[k + 1]]], "max_label": int(mx_out[k])}
            for k in range(len(masks))}


def _both(engine, masks, info, thr):
    got = dict(StitchTracker(stitch_threshold=thr, engine=engine)(masks, info))
    assert _through_engine(engine, masks, info, thr) == got
    return got


def check(engine, masks, info=None, thr=0.25):
    """Both entries equal the literal reference; returns the result."""
    want = track_ref.stitch_rois(masks, info, thr)
    assert _both(engine, masks, info, thr) == want
    return want


def _info(case):
    return None if case[2] is None else {"labels": list(case[2]), "max_label": case[3]}


# ------------------------------------------------------------------------------------------------------------------ ties
CASES = track_ref.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_case_alone(engine, name):
    prev, cur, tracked, mx, thr, want, want_mx = CASES[name]
    info = None if tracked is None else {0: _info(CASES[name])}
    assert check(engine, [[prev, cur]], info, thr) == {0: {"labels": want, "max_label": want_mx}}


def test_hand_worked_cases_as_tiles_of_one_call(engine):
    """One call per threshold and per kind of state (with tracked labels, without): every tile's answer is the literal one,
    which the test above shows to be its answer alone."""
    for thr in sorted({c[4] for c in CASES.values()}):
        for with_info in (False, True):
            names = [n for n in sorted(CASES) if CASES[n][4] == thr and (CASES[n][2] is not None) == with_info]
            if not names:
                continue
            masks = [[CASES[n][0], CASES[n][1]] for n in names]
            info = {k: _info(CASES[n]) for k, n in enumerate(names)} if with_info else None
            got = _both(engine, masks, info, thr)
            for k, n in enumerate(names):
                assert got[k] == {"labels": CASES[n][5], "max_label": CASES[n][6]}, (n, thr)


# ------------------------------------------------------------------------------------------- more than 256 objects a tile
def _dots(n, first=0, shift=0, shape=(40, 40)):
    """n single-pixel objects, label k on the k-th (counting from `first`) second pixel of the frame, `shift` pixels right."""
    f = np.zeros(shape, np.uint16)
    k = np.arange(n) + first
    f[k // (shape[1] // 2), 2 * (k % (shape[1] // 2)) + shift] = np.arange(1, n + 1)
    return f


def test_new_labels_carry_across_chunks_of_256_rows(engine):
    dots, empty = _dots(400), np.zeros((40, 40), np.uint16)
    got = check(engine, [[empty, dots]])
    assert got[0] == {"labels": list(range(1, 401)), "max_label": 400}
    got = check(engine, [[_dots(400, shift=1), dots]])
    assert got[0] == {"labels": list(range(401, 801)), "max_label": 800}
    # previous: the even labels only, tracked as 1000 + label; current: every third label removed.  Absent rows stay 0, even
    # labels are matched, odd ones are new: the three kinds alternate all the way across row 256
    prev, cur = dots.copy(), dots.copy()
    prev[prev % 2 == 1] = 0
    cur[cur % 3 == 0] = 0
    info = {0: {"labels": [1000 + k for k in range(1, 401)], "max_label": 1500}}
    got = check(engine, [[prev, cur]], info)
    lab = got[0]["labels"]
    assert lab[2::3] == [0] * 133 and lab[1] == 1002 and lab[255] == 1256 and lab[0] == 1501 and lab[256] > 1500
    assert got[0]["max_label"] == 1500 + sum(1 for k in range(1, 401) if k % 3 and k % 2)


def test_tiles_of_very_different_sizes_in_one_call(engine):
    rng = np.random.default_rng(5)
    n_cur, n_prev = (0, 1, 257, 600), (5, 0, 300, 200)
    masks = [[_dots(p, first=3 * k), _dots(c)] for k, (c, p) in enumerate(zip(n_cur, n_prev))]
    info = {k: {"labels": [int(v) for v in rng.permutation(np.arange(1, p + 1)) + 10 * k], "max_label": p + 10 * k + k}
            for k, p in enumerate(n_prev)}
    batched = check(engine, masks, info)
    assert [len(batched[k]["labels"]) for k in range(4)] == list(n_cur)
    for k in range(4):
        assert check(engine, [masks[k]], {0: info[k]})[0] == batched[k], k
    check(engine, masks)  # (and with the previous frames' own labels: the entry's NULL table of tracked labels)


# ------------------------------------------------------------------------------------------------------------ hash table
def _colliding(w1):
    """64x64; previous: 1030 labels, 1 and 1025 (same hash slot: 40503 mod 1024 == 1025 * 40503 mod 1024 == 567) as blocks of
    4 x w1 and 4 x (8 - w1) side by side, all others single pixels in the lower half; current: one 4x8 block over the two."""
    prev = np.zeros((64, 64), np.uint16)
    rest = [k for k in range(1, 1031) if k not in (1, 1025)]
    idx = np.arange(len(rest))
    prev[32 + idx // 64, idx % 64] = rest
    prev[0:4, 0:w1] = 1
    prev[0:4, w1:8] = 1025
    return prev, _frame((64, 64), (1, 0, 4, 0, 8))


def test_two_labels_in_one_hash_slot_are_counted_apart(engine):
    assert (1 * 40503) & 1023 == (1025 * 40503) & 1023 == 567
    plus7 = {0: {"labels": [k + 7 for k in range(1, 1031)], "max_label": 1037}}
    for info, a, b in ((None, 1, 1025), (plus7, 8, 1032)):
        assert check(engine, [list(_colliding(4))], info)[0]["labels"] == [a]  # 16/32 both: the smaller label by the row tie
        assert check(engine, [list(_colliding(3))], info)[0]["labels"] == [b]  # 12/32 against 20/32
        assert check(engine, [list(_colliding(5))], info)[0]["labels"] == [a]  # 20/32 against 12/32


def _pixels(rows):
    """64x64; previous: rows x 32 single-pixel labels; current: one object over all of them."""
    prev = np.zeros((64, 64), np.uint16)
    prev[:rows, :32] = np.arange(1, rows * 32 + 1).reshape(rows, 32)
    return prev, _frame((64, 64), (1, 0, rows, 0, 32))


def _stripes(n):
    """current: an n x 4 block; previous: its n rows, one label each: IoU 4 / (4 n + 4 - 4) = 1/n for every one of them."""
    prev = np.zeros((64, 64), np.uint16)
    prev[:n, :4] = np.arange(1, n + 1)[:, None]
    return prev, _frame((64, 64), (1, 0, n, 0, 4))


def test_hash_and_candidate_limits_and_recovery(engine):
    """At the limit: an answer.  One past it: ALIBY_ERR_TOO_LARGE naming the limit, and the next call on the same engine gives an
    earlier case its earlier answer again (the overflow flag is cleared; nothing in the scratch is trusted between calls)."""
    earlier_masks = [list(_colliding(3))]
    earlier = check(engine, earlier_masks)

    full = check(engine, [list(_pixels(32))], thr=0.01)  # 1024 distinct previous labels, IoU 1/1024 each: a new label
    assert full[0] == {"labels": [1025], "max_label": 1025}
    for info in (None, {0: {"labels": list(range(2000, 2000 + 1056)), "max_label": 0}}):
        with pytest.raises(AlibyHipError, match="1024"):
            StitchTracker(stitch_threshold=0.01, engine=engine)([list(_pixels(33))], info)
        assert _both(engine, earlier_masks, None, 0.25) == earlier
    # 1056 previous objects in 1024 groups (the last 33 share one tracked label): the limit counts groups
    grouped = {0: {"labels": list(range(1, 1024)) + [5000] * 33, "max_label": 5000}}
    assert check(engine, [list(_pixels(33))], grouped, thr=0.01)[0]["labels"] == [5000]  # 33 / 1056 = 1/32 >= 0.01

    assert check(engine, [list(_stripes(16))], thr=0.05)[0] == {"labels": [1], "max_label": 16}  # 16 candidates of 1/16, a 16-way tie
    tracked17 = {0: {"labels": list(range(30, 47)), "max_label": 50}}
    for info in (None, tracked17):
        with pytest.raises(AlibyHipError, match="16"):
            StitchTracker(stitch_threshold=0.05, engine=engine)([list(_stripes(17))], info)  # 1/17 >= 0.05 seventeen times
        assert _both(engine, earlier_masks, None, 0.25) == earlier
    # 17 stripes in 16 groups: 15 of 1/17 and one of 8 / 68 = 2/17, which wins
    grouped = {0: {"labels": list(range(30, 46)) + [33], "max_label": 50}}
    assert check(engine, [list(_stripes(17))], grouped, thr=0.05)[0] == {"labels": [33], "max_label": 50}
    assert check(engine, [list(_stripes(16))], thr=0.05)[0]["labels"] == [1]


# ---------------------------------------------------------------------------------------------------------------- shapes
def test_shapes(engine):
    whole = np.ones((24, 24), np.uint16)
    quarters = _frame((24, 24), (1, 0, 12, 0, 12), (2, 0, 12, 12, 24), (3, 12, 24, 0, 12), (4, 12, 24, 12, 24))
    ring = _frame((24, 24), (1, 2, 22, 2, 22), (0, 6, 18, 6, 18), (2, 9, 15, 9, 15))  # object 2 inside object 1's box
    disc = _frame((24, 24), (1, 7, 17, 7, 17))
    border = _frame((24, 24), (1, 0, 24, 0, 1), (2, 0, 1, 1, 24), (3, 1, 24, 23, 24), (4, 23, 24, 1, 23))
    for prev, cur in ((whole, whole), (quarters, whole), (whole, quarters), (ring, disc), (disc, ring), (ring, ring),
                      (border, quarters), (quarters, border), (border, border)):
        check(engine, [[prev, cur]], thr=0.05)
        check(engine, [[prev, cur]], {0: {"labels": [3, 3, 9, 2][: int(prev.max())], "max_label": 9}}, thr=0.05)
    odd = [track_ref.random_lapse(s, n_frames=2, shape=(23, 37))[0] for s in range(3)]  # X = 37: an odd row stride
    check(engine, odd, thr=0.05)
    row = np.zeros((1, 64), np.uint16), np.zeros((1, 64), np.uint16)  # a frame of one row
    row[0][0, 3:20], row[0][0, 40:64], row[1][0, 0:10], row[1][0, 12:30], row[1][0, 63:] = 1, 2, 1, 2, 3
    # 7/20 and 8/27 in the column of previous 1: the second loses and is new; 1/24 is below the threshold
    assert check(engine, [list(row)], thr=0.05)[0] == {"labels": [1, 3, 4], "max_label": 4}


# ------------------------------------------------------------------------------------------- duplicate tracked labels
def test_split_merge_split_follows_the_relabelled_frame(engine):
    """Whole, its two halves (16/32 each: a column tie, both keep label 1), whole again with a bite (the halves are one object:
    32/40 = 0.8 at threshold 0.5, label 1; taken apart it would be 0.4 twice and a new label), the halves again (16/40 each, below
    0.5: two new labels).  Then random lapses of dividing rectangles, three tiles a call."""
    S = (8, 20)
    halves = _frame(S, (1, 0, 4, 0, 4), (2, 0, 4, 4, 8))
    frames = [_frame(S, (1, 0, 4, 0, 8)), halves, _frame(S, (1, 0, 4, 0, 8), (1, 4, 6, 0, 4)), halves]
    trk = StitchTracker(stitch_threshold=0.5, engine=engine)
    steps = track_ref.run_lapse(lambda m, i: trk(m, i), frames)
    assert steps == track_ref.run_lapse(track_ref.stitch_rois, frames, threshold=0.5)
    assert [s[0] for s in steps] == [{"labels": [1, 1], "max_label": 1}, {"labels": [1], "max_label": 1}, {"labels": [2, 3], "max_label": 3}]
    seen = 0
    for seed in range(0, 12, 3):
        lapses = [track_ref.random_lapse(seed + k) for k in range(3)]
        thr = lapses[0][1]
        info = None
        for t in range(1, 4):
            masks = [[frames[t - 1], frames[t]] for frames, _ in lapses]
            seen += info is not None and any(len(set(v["labels"]) - {0}) < sum(x > 0 for x in v["labels"]) for v in info.values())
            info = check(engine, masks, info, thr)
    assert seen > 0  # some call did start from duplicate tracked labels


def test_stitch_planes_sees_the_two_halves_as_one_object(engine):
    planes, want, n_want = track_ref.split_merge_planes()
    stacks = np.stack([planes, planes[::-1]])
    vol, counts = engine.stitch_planes(torch.from_numpy(stacks.copy()).cuda(), threshold=0.01)
    got = vol.cpu().numpy()
    assert int(counts[0]) == n_want and np.array_equal(got[0], want)  # the volume worked by hand
    for f in range(2):
        ref, n = volume_restated.stitch3d(stacks[f], 0.01)
        assert int(counts[f]) == n and np.array_equal(got[f], ref), f


# ---------------------------------------------------------------------------------------------------- Python front end
def test_front_end_checks_its_arguments(engine):
    prev, cur = CASES["column_tie"][:2]
    trk = StitchTracker(engine=engine)
    long = trk([[prev, cur]], {0: {"labels": [3, 8, 9], "max_label": 3}})
    assert dict(long) == {0: {"labels": [3, 3], "max_label": 3}} == track_ref.stitch_rois([[prev, cur]], {0: {"labels": [3, 8, 9], "max_label": 3}})
    with pytest.raises(ValueError, match="tracked labels"):
        trk([[cur, prev]], {0: {"labels": [3], "max_label": 3}})  # two previous objects, one label: refused before the stitch is launched
    with pytest.raises(AssertionError, match="wrong dimensions"):
        trk([[prev, np.zeros((8, 21), np.uint16)]])
