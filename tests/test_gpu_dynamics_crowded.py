"""
The mask dynamics (aliby_amd/csrc/dynamics.hip) on crowded frames: every case puts a kernel past a capacity above which it works
in several passes, and compares labels, counts and end points exactly with the CPU restatement (oracle/cellpose_restated.py,
tests/cellpose3d_ref.py).  The inputs are the patterns of tests/crowded_flows.py; tests/test_cpu_crowded_flows.py holds, without
a GPU, that the restatement gives the counts they are named for.  That a limit is crossed is asserted from the restatement's
output and the inputs, never from what the kernels return.

  k_grow / k3_grow       256 / 1024 workgroups per frame, further seeds in rounds of k += gridDim.x
  k_rank_ids             256 seeds per round, the others' first positions through LDS 1024 at a time
  k_final_ids            1024 threads per frame, ceil(n / 1024) rows each ahead of the prefix sum
  k_zero_boxes           8192 workgroups, strided over the masks of a call
  k_follow, k_assign,    16384 x 256 items per round: 4 194 304 foreground pixels or padded histogram cells
  k_apply_ids, k_seeds
  k_diffuse<true>,       256 workgroups with one slab of global scratch each, walking the masks of a call, once one box is
  k_fill<4, true>        beyond LDS (17 bytes x padded cells > 128 KiB; padded cells > 131 072)
"""
import numpy as np
import pytest

from tests import crowded_flows as cf

pytestmark = pytest.mark.gpu

ROUND = 16384 * 256  # items per round of the capped per-pixel grids


def run(engine, names):
    """One call on the frames (volumes) `names` with their keywords -> (labels, counts, end points) as numpy."""
    import torch

    from aliby_amd.segment.dynamics import masks_from_flows, masks_from_flows_3d

    kws = [cf.keywords(n) for n in names]
    assert all(k == kws[0] for k in kws)
    dP = torch.from_numpy(np.stack([cf.inputs(n)[1] for n in names])).cuda()
    prob = torch.from_numpy(np.stack([cf.inputs(n)[2] for n in names])).cuda()
    fn = masks_from_flows_3d if prob.ndim == 4 else masks_from_flows
    labels, n, pf = fn(engine, dP, prob, return_endpoints=True, **kws[0])
    torch.cuda.synchronize()
    return labels.cpu().numpy(), np.asarray(n).copy(), pf.cpu().numpy()


def check(got, names):
    """Labels, counts and end points of every frame equal the restatement's."""
    labels, n, pf = got
    assert len(n) == len(names)
    for k, name in enumerate(names):
        want, pf_want = cf.restated(name)
        assert int(want.max()) == cf.count(name), name
        assert int(n[k]) == cf.count(name), (k, name, int(n[k]))
        assert np.array_equal(pf[k], pf_want), (k, name, "end points differ")
        assert np.array_equal(labels[k], want), (k, name, f"{int((labels[k] != want).sum())} pixels differ")


# ------------------------------------------------------------------------------------------------ 1. seeds per frame
@pytest.mark.parametrize("name", ["g256", "g259", "g361", "g440", "g1156", "g1681"])
def test_seeds_per_frame_around_256_and_above_1024(engine, name):
    """One frame with exactly 256 masks (the last count one round of k_grow and k_rank_ids takes), a few more, and beyond the
    1024 of k_rank_ids' LDS batch and of k_final_ids' one row per thread.  The seeds are appended in atomic order, so the
    first-appearance numbering is k_rank_ids' own work: nothing is sorted before the comparison."""
    assert cf.count(name) in (256, 259, 361, 440, 1156, 1681)
    check(run(engine, [name]), [name])


def test_one_call_with_frames_of_very_different_counts(engine):
    """1, 1156, 0 and 300 masks in four frames of one shape: per-frame seed lists, offsets and counts.  Every frame also equals
    its run alone."""
    names = ["one208", "g1156", "empty208", "g300_208"]
    assert [cf.count(n) for n in names] == [1, 1156, 0, 300]
    got = run(engine, names)
    check(got, names)
    for k, name in enumerate(names):
        alone = run(engine, [name])
        assert all(np.array_equal(a[0], b[k]) for a, b in zip(alone, got)), name


# ------------------------------------------------------------------------------------------------ 3. rows dropped mid-table
def dropped_on_both_sides(name, **before_kw):
    before, _ = cf.restated(name, **before_kw)
    after, _ = cf.restated(name)
    assert int(before.max()) > 1024 and int(after.max()) == cf.count(name)
    return cf.on_both_sides(cf.dropped_rows(before, after))


def test_small_masks_dropped_in_the_middle_of_a_long_table(engine):
    """Every third square 4 x 4 among 5 x 5 ones and min_size=20: k_final_ids renumbers across two rows per thread, with gaps."""
    assert dropped_on_both_sides("mixed1156", min_size=0)
    check(run(engine, ["mixed1156"]), ["mixed1156"])


@pytest.mark.parametrize("name", ["noisy1156_qc", "noisy1156_noqc"])
def test_flow_qc_drops_rows_above_1024(engine, name):
    """Every 7th square's flows replaced by noise: with the default flow_threshold the QC sets bad[] at rows on both sides of
    1024 (and min_size drops the specks the noise leaves); with flow_threshold=0.0 only the latter."""
    assert dropped_on_both_sides(name, flow_threshold=0.0, min_size=0)
    if name == "noisy1156_qc":  # the QC alone
        before, _ = cf.restated(name, flow_threshold=0.0, min_size=0)
        after, _ = cf.restated(name, min_size=0)
        assert cf.on_both_sides(cf.dropped_rows(before, after))
    check(run(engine, [name]), [name])


def test_large_masks_dropped_in_a_dense_frame(engine):
    """11 x 11 squares among 5 x 5 ones with a max_size_fraction between the two: k_rank_ids ranks the kept seeds past the
    dropped ones, above 1024 seeds."""
    assert dropped_on_both_sides("quad1102", max_size_fraction=0.4)
    check(run(engine, ["quad1102"]), ["quad1102"])


# ------------------------------------------------------------------------------------------------ 4. volumes
@pytest.mark.parametrize("names", [["v1156"], ["v450"], ["v450_of_1156", "v1156"]], ids="+".join)
def test_volumes_with_more_seeds_than_workgroups(engine, names):
    """1156 cubes in one volume (k3_grow has 1024 workgroups per volume; k_rank_ids and k_final_ids as for images), 450 in two
    layers, and a batch of two volumes with 450 and 1156."""
    assert [cf.count(n) for n in names] in ([1156], [450], [450, 1156])
    check(run(engine, names), names)


def test_small_cubes_dropped_in_a_crowded_volume(engine):
    """min_size=28 among 3 x 3 x 3 cubes: only the 3 x 7 x 7 boxes placed among them survive, on both sides of row 1024."""
    assert dropped_on_both_sides("vmixed", min_size=0)
    check(run(engine, ["vmixed"]), ["vmixed"])


# ------------------------------------------------------------------------------------------------ 5. global-scratch forms
def box_and_holes(name):
    want, _ = cf.restated(name)
    holes = cf.holes(name)
    gt = cf.inputs(name)[0]
    big = gt == gt.max()
    assert int(want.max()) == cf.count(name) > 256
    assert (holes & big).sum() == 1 and (holes & ~big).sum() > 100 and (want[holes] > 0).all()  # holes exist and are filled
    return (cf.largest_padded_box(want) + 15) // 16 * 16


def test_diffusion_in_global_scratch_walks_several_masks_per_workgroup(engine):
    """A disc whose padded box is beyond LDS for the QC (17 bytes per cell) with 360 small squares: k_diffuse<true> has 256
    workgroups, so slabs are used again for a second mask."""
    assert box_and_holes("qc_crowd") * 17 > 128 * 1024
    check(run(engine, ["qc_crowd"]), ["qc_crowd"])


def test_hole_fill_in_global_scratch_walks_several_masks_per_workgroup(engine):
    """A disc whose padded box passes the 131 072 cells the 2-D hole fill keeps in LDS, with 932 small squares, every third with
    a hole: k_fill<4, true> has 256 workgroups with one slab each.  (flow_threshold=0.0: the restatement's diffusion of the
    disc alone would take 20 s.)"""
    assert box_and_holes("fill_crowd") > 128 * 1024 and cf.keywords("fill_crowd")["flow_threshold"] == 0.0
    check(run(engine, ["fill_crowd"]), ["fill_crowd"])


# ------------------------------------------------------------------------------------------------ 6. the capped grids
@pytest.mark.parametrize("reverse", [False, True], ids=["", "reversed_list"])
def test_more_foreground_than_one_round_of_the_capped_grids(engine, monkeypatch, reverse):
    """80 frames of 256 x 256 tiled with 11 x 11 squares: 4 268 880 foreground pixels (k_follow, k_assign with its run folding,
    k_apply_ids take a second round), 7 009 280 padded histogram cells (k_seeds) and 35 280 masks (k_zero_boxes).  Three tilings
    that differ in offset are cycled through the batch, so neighbouring frames differ.  The restatement checks each tiling
    alone; the frames of the batch are then compared with the run of their tiling alone.  With ALIBY_DEBUG_FG_REVERSE=1 one
    workgroup of k_prep_compact walks all 1280 chunks, last to first."""
    import torch

    from aliby_amd.segment.dynamics import masks_from_flows

    monkeypatch.delenv("ALIBY_DEBUG_FG_REVERSE", raising=False)
    tilings = ["t256_0", "t256_1", "t256_2"]
    F = 80
    alone = {}
    for name in tilings:
        alone[name] = run(engine, [name])
        check(alone[name], [name])
    names = [tilings[k % 3] for k in range(F)]
    probs = [cf.inputs(n)[2] for n in tilings]
    assert all(not np.array_equal(a, b) for a, b in zip(probs, probs[1:] + probs[:1]))
    assert sum(int((cf.inputs(n)[2] > 0).sum()) for n in names) == 4268880 > ROUND  # the list's length
    assert F * (256 + 40) * (256 + 40) > ROUND and sum(cf.count(n) for n in names) == 35280 > 8192
    if reverse:
        monkeypatch.setenv("ALIBY_DEBUG_FG_REVERSE", "1")
    dP = torch.from_numpy(np.stack([cf.inputs(n)[1] for n in names])).cuda()
    prob = torch.from_numpy(np.stack([cf.inputs(n)[2] for n in names])).cuda()
    labels, n, pf = masks_from_flows(engine, dP, prob, return_endpoints=True)
    torch.cuda.synchronize()
    assert n.tolist() == [441] * F
    want = {k: [torch.from_numpy(a[0]).cuda() for a in (v[0], v[2])] for k, v in alone.items()}
    for k, name in enumerate(names):
        assert torch.equal(labels[k], want[name][0]), (k, name)
        assert torch.equal(pf[k], want[name][1]), (k, name, "end points")


# ------------------------------------------------------------------------------------------------ 7. more seeds than labels
def test_more_seeds_than_uint16_labels_are_refused(engine):
    """256 x 257 squares in one frame: more seeds than the 65 536 slots of a frame's seed list.  k_seeds stores only below the
    list's end, k_grow and k_rank_ids walk min(count, 65536) seeds, k_apply_ids clamps the id; the host then refuses the frame
    as the reference's finish_labels does.  The next call on the same workspace is unharmed."""
    import torch

    from aliby_amd import synth
    from aliby_amd.segment import dynamics
    from oracle import cellpose_restated as cr

    gt = cf.grid_labels(cf.OVERFLOW_SHAPE, cf.OVERFLOW_SIDE, cf.OVERFLOW_PITCH)
    assert int(gt.max()) > 65536
    with pytest.raises(OverflowError, match="uint16 cast unsafe"):
        cr.finish_labels(gt)
    dP, prob = synth.analytic_flows(gt)
    with pytest.raises(OverflowError, match=r"Segmentation produced \d+ seeds in one tile; uint16 cast unsafe"):
        dynamics.masks_from_flows(engine, torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda())
    assert len(dynamics._workspaces) == 1
    for name in ("g259", "g1156"):
        check(run(engine, [name]), [name])
