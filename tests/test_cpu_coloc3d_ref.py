"""
Pins tests/coloc3d_ref.py (the float64 reference the GPU family `coloc3d` is compared with) independently of the oracle where a
closed form or another route exists: numpy.corrcoef / polyfit for Pearson and slope, an affine pair of channels, Manders of
identical and of disjoint channels, RWC of channels in the same rank order, a one-plane volume against the oracle's own 2-D
numbers, and invariance under a permutation of Z.  It also shows that the inputs of tests/test_gpu_coloc3d.py are not degenerate
for Costes' discrete search, and that the new C entry is declared and bound.  cp_measure / CellProfiler are not vendored: parity
with MeasureColocalization on volumes stays unpinned.
"""
import re
import warnings
from pathlib import Path

import numpy as np
import pytest

from tests import coloc3d_ref as ref

ROOT = Path(__file__).resolve().parents[1]
COL = {k: i for i, k in enumerate(ref.NAMES)}


@pytest.fixture(autouse=True)
def _quiet_numpy():
    with warnings.catch_warnings():  # (the oracle's one-voxel variance: numpy warns, the value is the NaN that is wanted)
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def test_the_c_entry_is_declared_bound_and_named():
    header = (ROOT / "include" / "aliby_hip.h").read_text()
    assert re.search(r"\bint aliby_features_coloc3d\s*\(", header) and re.search(r"\bint aliby_coloc3d_lds_voxels\s*\(", header)
    from aliby_amd import _lib
    from aliby_amd.extraction import features

    assert {"aliby_features_coloc3d", "aliby_coloc3d_lds_voxels"} <= set(_lib.exported_symbols())
    names = features.coloc3d_names([(0, 1), (2, 1)])
    assert names[:8] == [f"(0, 1)/{m}/{n}" for m in ref.METRICS for n in ref.COLUMNS[m]]
    assert names[8] == "(2, 1)/pearson/Correlation_Pearson" and len(names) == 16
    assert features.coloc3d_names([(1, 0)], ("costes", "pearson")) == ["(1, 0)/costes/Correlation_Costes_1", "(1, 0)/costes/Correlation_Costes_2",
                                                                      "(1, 0)/pearson/Correlation_Pearson", "(1, 0)/pearson/Correlation_Slope"]
    for bad in (dict(pairs=[(1, 1)]), dict(pairs=[(0, 1)], metrics=("pearson", "spearman")), dict(pairs=[(0, 1)], metrics=()),
                dict(pairs=[(0, 1)], metrics=("rwc", "rwc")), dict(pairs=[(0, -1)]), dict(pairs=[(0, 1, 2)])):
        with pytest.raises(ValueError):
            features.coloc3d_names(**bad)


def test_pearson_and_slope_equal_numpy():
    vol, n, px = ref.irregular()
    for p in (px, ref.unit_float(px)):
        got = ref.coloc3d(vol, p[0], p[2], n, metrics=("pearson",))
        for lab in range(1, n + 1):
            x, y = p[0][vol == lab].astype(np.float64), p[2][vol == lab].astype(np.float64)
            assert np.isclose(got[lab - 1, 0], np.corrcoef(x, y)[0, 1], rtol=1e-10, atol=0)
            assert np.isclose(got[lab - 1, 1], np.polyfit(x, y, 1)[0], rtol=1e-8, atol=0)


def test_an_affine_pair_has_pearson_one_and_its_slope():
    vol, n, px = ref.irregular(2, (7, 61, 83))
    c0 = ref.unit_float(px)[0]
    for a, b in ((0.5, 0.125), (2.0, 0.0), (-0.25, 0.75)):
        got = ref.coloc3d(vol, c0, a * c0.astype(np.float64) + b, n, metrics=("pearson",))
        assert np.allclose(got[:, 0], np.sign(a), rtol=0, atol=1e-12) and np.allclose(got[:, 1], a, rtol=1e-10, atol=0)


def test_manders_of_identical_and_of_disjoint_channels():
    vol, n, px = ref.irregular(3, (9, 17, 130))
    c0 = px[0]
    same = ref.coloc3d(vol, c0, c0, n, metrics=("manders_fold", "rwc"))
    assert np.array_equal(same, np.ones_like(same))  # identical channels: all of each above both thresholds, rank difference 0
    # disjoint support above the threshold: channel 1 is bright only where channel 0 is dark, inside every object
    bright0 = c0 >= 0.5 * np.asarray([c0[vol == k].max() if k else 0 for k in range(n + 1)])[vol]
    c1 = np.where(bright0, 1, 1000).astype(np.uint16)
    lo = np.where(bright0, c0, 1).astype(np.uint16)  # channel 0 far below 15 % of its maximum wherever channel 1 is bright
    apart = ref.coloc3d(vol, lo, c1, n, metrics=("manders_fold",), thr=15)
    assert np.array_equal(apart, np.zeros_like(apart))


def test_rwc_equals_manders_when_the_rank_order_is_the_same():
    vol, n, px = ref.irregular(4, (8, 8, 64), n_seeds=5)
    c0 = px[0].astype(np.float64)
    c1 = np.sqrt(c0) * 3.0 + 1.0  # strictly increasing in c0: the same dense ranks, every weight 1
    got = ref.coloc3d(vol, c0, c1, n, metrics=("manders_fold", "rwc"))
    assert np.allclose(got[:, 2:], got[:, :2], rtol=1e-14, atol=0) and (got[:, :2] > 0).all()


def test_a_one_plane_volume_gives_the_oracles_2d_numbers():
    from oracle import cp_measure_restated as cpm

    vol, n, px = ref.irregular(31, (1, 64, 72), n_seeds=8)
    p = ref.unit_float(px)
    got = ref.coloc3d(vol, p[0], p[1], n)
    for lab in range(1, n + 1):
        one = (vol[0] == lab).astype(np.uint16)
        want = []
        for m in ref.METRICS:
            res = cpm.get_correlation_measurements()[m](p[0][0], p[1][0], one)
            want += [res[k][0] for k in ref.COLUMNS[m]]
        assert np.array_equal(got[lab - 1], np.asarray(want), equal_nan=True)


def test_permuting_z_changes_nothing():
    """Labels and pixels permuted together: the voxel lists are the same sets in another order.  Pearson's sums, the Manders and
    Costes fractions and the ranks do not depend on the order beyond the rounding of a float64 sum."""
    vol, n, px = ref.irregular(5, (16, 16, 128))
    p = ref.unit_float(px)
    perm = np.random.default_rng(0).permutation(vol.shape[0])
    a = ref.coloc3d(vol, p[0], p[1], n)
    b = ref.coloc3d(vol[perm], p[0][perm], p[1][perm], n)
    assert np.allclose(a, b, rtol=1e-11, atol=1e-13, equal_nan=True)


def test_absent_labels_and_column_layout():
    vols, counts, px = ref.split_batch()
    want = ref.coloc3d_batch(vols, ref.unit_float(px), [(0, 1), (1, 0)], counts, metrics=("costes", "pearson"))
    assert want.shape == (sum(counts), 8)
    assert np.isnan(want[-2:]).all() and np.isfinite(want[:-2]).all()
    full = ref.coloc3d(vols[2], ref.unit_float(px[2])[1], ref.unit_float(px[2])[0], counts[2])
    assert np.array_equal(want[counts[0]:, 4:6], full[:, 6:8], equal_nan=True) and np.array_equal(want[counts[0]:, 6:8], full[:, 0:2], equal_nan=True)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def _check_probes(name, vol, n, px, pairs, scale_max, degenerate=()):
    worst = np.inf
    for a, b in pairs:
        for lab, log in enumerate(ref.costes_probes(vol, px[a], px[b], n, scale_max), 1):
            v = np.asarray(log, float)
            if lab in degenerate:  # built to have no defined correlation: every probe over more than two voxels is NaN on purpose
                v = v[np.isfinite(v)]
            assert not np.isnan(v).any(), (name, (a, b), lab)
            if v.size:
                worst = min(worst, float(np.abs(v).min()))
                assert np.abs(v).min() >= ref.PROBE_MARGIN, (name, (a, b), lab, float(np.abs(v).min()))
    print(f"coloc3d probes, {name}: smallest |Pearson| of a Costes probe {worst:.2e}")
    return worst


@pytest.mark.parametrize("case", ref.cases(), ids=[c[0] for c in ref.cases()])
def test_no_costes_probe_of_a_gpu_test_input_is_near_a_sign_change(case):
    """Every object, pair and dtype of tests/test_gpu_coloc3d.py: the Pearson value of every probe of the reference's bisection
    stays PROBE_MARGIN clear of zero, so two correct implementations take the same path.  A seed that fails is replaced."""
    _check_probes(*case)


def test_the_segmenters_labels_are_not_degenerate_either():
    from tests import cellpose3d_ref

    f, gt, dP, prob = ref.segmenter_case()
    labels, n, _ = cellpose3d_ref.compute_masks_3d(dP, prob)
    assert n > 0
    _check_probes("segmenter", labels, n, f["pixels"], [(0, 1)], 255.0)
    _check_probes("segmenter unit f32", labels, n, ref.unit_float(f["pixels"]), [(0, 1)], 255.0)


def test_the_budget_volume_has_objects_on_both_sides():
    vol, n, px, counts = ref.budget_volume(8192)
    assert list(counts[:3]) == [8192, 8193, 7192] and counts[3] > 2 * 8192 and counts[4] == 9
