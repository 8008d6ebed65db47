"""
The crowded patterns of tests/crowded_flows.py under the CPU restatement alone: every pattern gives the number of masks it is
named for, with the input's foreground, and the drops, boxes and holes that tests/test_gpu_dynamics_crowded.py relies on are
really there.  No GPU.
"""
import numpy as np
import pytest

from tests import crowded_flows as cf

CLEAN_2D = ["g256", "g259", "g361", "g440", "g1156", "g1681", "empty208", "one208", "g300_208", "t256_0", "t256_1", "t256_2"]
CLEAN_3D = ["v450", "v1156", "v450_of_1156"]


@pytest.mark.parametrize("name", CLEAN_2D + CLEAN_3D)
def test_one_mask_per_square(name):
    gt, _, prob = cf.inputs(name)
    labels, pf = cf.restated(name)
    assert int(gt.max()) == cf.count(name) == int(labels.max())
    assert len(np.unique(labels)) == cf.count(name) + 1
    assert np.array_equal(labels > 0, gt > 0) and np.array_equal(prob > 0, gt > 0)
    # (one mask per square, not just as many: no label spans two squares)
    pairs = np.unique(np.stack([gt[gt > 0], labels[gt > 0].astype(np.int64)]), axis=1)
    assert pairs.shape[1] == cf.count(name)
    assert not pf[:, gt == 0].any()


def test_counts_sit_where_the_cases_need_them():
    """256 is the last count one round of the growth and of the ranking takes, 259 the first few beyond it; 1024 the last one LDS
    batch of the ranking and one row per thread of the final ids take."""
    c = cf.count
    assert c("g256") == 256 < c("g259") < c("g361") < c("g440") < 1024 < c("g1156") < c("g1681")
    assert c("v450") < 1024 < c("v1156")
    assert c("one208") == 1 and c("empty208") == 0 and 256 < c("g300_208") < 1024
    shapes = {cf.inputs(n)[0].shape for n in ("empty208", "one208", "g300_208", "g1156")}
    assert len(shapes) == 1
    assert cf.inputs("v450_of_1156")[0].shape == cf.inputs("v1156")[0].shape


@pytest.mark.parametrize("name,before_kw", [("mixed1156", dict(min_size=0)),
                                            ("noisy1156_qc", dict(flow_threshold=0.0, min_size=0)),
                                            ("noisy1156_noqc", dict(min_size=0)),
                                            ("quad1102", dict(max_size_fraction=0.4)),
                                            ("vmixed", dict(min_size=0))])
def test_rows_are_dropped_on_both_sides_of_row_1024(name, before_kw):
    gt, _, _ = cf.inputs(name)
    before, _ = cf.restated(name, **before_kw)
    after, _ = cf.restated(name)
    assert int(after.max()) == cf.count(name) < int(before.max()) and int(before.max()) > 1024
    assert ((after > 0) <= (gt > 0)).all()
    assert cf.on_both_sides(cf.dropped_rows(before, after))


def test_the_flow_qc_itself_drops_rows_on_both_sides_of_row_1024():
    before, _ = cf.restated("noisy1156_qc", flow_threshold=0.0, min_size=0)
    after, _ = cf.restated("noisy1156_qc", min_size=0)
    assert cf.on_both_sides(cf.dropped_rows(before, after))


def test_mixed_grid_keeps_the_larger_squares():
    gt, _, _ = cf.inputs("mixed1156")
    after, _ = cf.restated("mixed1156")
    sizes = np.bincount(gt.ravel())
    assert np.array_equal(after > 0, np.isin(gt, np.nonzero(sizes >= 20)[0][1:]))


@pytest.mark.parametrize("name,cells_over,bytes_per_cell", [("qc_crowd", 128 * 1024, 17), ("fill_crowd", 128 * 1024, 1)])
def test_one_box_passes_lds_among_more_than_256_masks(name, cells_over, bytes_per_cell):
    gt, _, prob = cf.inputs(name)
    labels, _ = cf.restated(name)
    assert int(labels.max()) == cf.count(name) == int(gt.max()) > 256
    cells = (cf.largest_padded_box(labels) + 15) // 16 * 16
    assert cells * bytes_per_cell > cells_over
    # the holes (every third square's, and the one in the big mask) are background in the input and filled in the output
    holes = cf.holes(name)
    big = gt == gt.max()
    assert (holes & ~big).sum() >= cf.count(name) // 3 - 1 and (holes & big).sum() == 1
    assert (labels[holes] > 0).all()
    assert np.array_equal(labels > 0, gt > 0)


def test_overflow_frame_has_more_squares_than_seed_slots():
    gt = cf.grid_labels(cf.OVERFLOW_SHAPE, cf.OVERFLOW_SIDE, cf.OVERFLOW_PITCH)
    assert int(gt.max()) == 256 * 257 > 65536
    from oracle import cellpose_restated as cr

    with pytest.raises(OverflowError, match="uint16 cast unsafe"):
        cr.finish_labels(gt)
