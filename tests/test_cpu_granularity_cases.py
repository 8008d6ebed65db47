"""
The preconditions of tests/granularity_cases.py, checked against the oracle alone (no GPU): that each case is the edge it claims
to be, that the division / reciprocal cases can tell the two apart, that the serpentine needs nearly as many sweeps as the
kernel allows, and that every case satisfies the bound behind the tolerance of tests/test_gpu_granularity.py.
"""
import inspect

import numpy as np
import pytest

from oracle import granularity_restated as gr
from tests import granularity_cases as gc


def _matrix(d):
    return np.stack([d[k] for k in d], axis=1)


def _last_sample(n, size):
    """index of the last sampling point along an axis of n pixels"""
    return int(np.ceil(n * size)) - 1


@pytest.mark.parametrize("name", list(gc.NONDYADIC))
def test_nondyadic_shapes_sit_on_the_edge(name):
    """On the stated axes the last sampling point is outside the frame when divided and inside when multiplied by the
    reciprocal; on every other axis, and in the control, both agree."""
    shape, kw, sub_axes, back_axes = gc.NONDYADIC[name]
    _, sub, _ = gc.geometry(shape, kw)
    for src, size, axes in ((shape, kw["subsample_size"], sub_axes), (sub, kw["image_sample_size"], back_axes)):
        for axis, n in enumerate(src):
            i = _last_sample(n, size)
            divided, multiplied = i / size, i * (1.0 / size)
            if axis in axes:
                assert divided > n - 1 >= multiplied, (name, axis, n, size)
            else:
                assert (divided > n - 1) == (multiplied > n - 1), (name, axis, n, size)
                every = np.arange(i + 1)
                assert np.array_equal((every / size > n - 1), (every * (1.0 / size) > n - 1))


@pytest.mark.parametrize("name", list(gc.OVERSHOOT))
def test_overshoot_shapes_overshoot(name):
    """(n - 1) * ((m - 1) / (n - 1)) > m - 1 on the stated axes of the stated resize, and on no other."""
    shape, kw, sub_axes, back_axes = gc.OVERSHOOT[name]
    _, sub, back = gc.geometry(shape, kw)
    for dst, src, axes in ((shape, sub, sub_axes), (sub, back, back_axes)):
        for axis, (n, m) in enumerate(zip(dst, src)):
            last = float(n - 1) * (float(m - 1) / float(n - 1))
            assert (last > m - 1) == (axis in axes), (name, axis, n, m)
    lab = gc.overshoot(name)[0][0]
    last_row_only = [l for l in range(1, int(lab.max()) + 1) if (lab[-1] == l).any() and not (lab[:-1] == l).any()]
    assert last_row_only and (lab[-1] > 0).any() and (lab[:, -1] > 0).any()


def _reciprocal_variant():
    """the oracle with `/ size` replaced by `* (1.0 / size)` in its two samplings: what the kernel computed before the fix"""
    src = inspect.getsource(gr)
    changed = src
    for size in ("subsample_size", "image_sample_size"):
        old = f".astype(float) / {size}"
        assert changed.count(old) == 1, old
        changed = changed.replace(old, f".astype(float) * (1.0 / {size})")
    assert changed != src
    ns = {"__name__": "granularity_reciprocal_variant"}
    exec(compile(changed, "granularity_reciprocal_variant", "exec"), ns)
    return ns["get_granularity"]


@pytest.mark.parametrize("image_mask", ["frame", "objects"])
def test_division_cases_discriminate(image_mask):
    """The oracle and its reciprocal-multiply variant differ by more than 1e-3 on every division / reciprocal case and agree
    within the GPU tests' tolerance on the control.  Every case has the border objects the issue asks for."""
    variant = _reciprocal_variant()
    for name in gc.NONDYADIC:
        labels, planes, kw = gc.nondyadic(name)
        assert labels.shape[0] == 2 and planes.dtype == np.uint16
        worst = 0.0
        for f in range(labels.shape[0]):
            assert (labels[f, -1] > 0).any() and (labels[f, :, -1] > 0).any()
            for c in range(planes.shape[1]):
                a = _matrix(gr.get_granularity(labels[f], planes[f, c], image_mask=image_mask, mask_order=1, **kw))
                b = _matrix(variant(labels[f], planes[f, c], image_mask=image_mask, mask_order=1, **kw))
                assert not np.isnan(a).any()
                if name == "control":
                    assert np.allclose(a, b, rtol=gc.RTOL, atol=gc.ATOL)
                worst = max(worst, float(np.abs(a - b).max()))
        assert (worst < 1e-9) if name == "control" else (worst > 1e-3), (name, worst)


def test_serpentine_needs_most_of_the_sweeps_the_kernel_allows(monkeypatch):
    labels, planes, kw = gc.serpentine()
    _, (sh, sw), _ = gc.geometry(labels.shape[1:], kw)
    sweeps = []

    def counted(seed, mask, footprint):
        """gr.reconstruction_by_dilation, counting the dilations that changed something"""
        rec = np.minimum(seed, mask).astype(np.float64)
        n = 0
        while True:
            grown = np.minimum(gr.ndi.grey_dilation(rec, footprint=footprint, mode="constant", cval=-np.inf), mask)
            if np.array_equal(grown, rec):
                sweeps.append(n)
                return rec
            rec = grown
            n += 1

    plain = _matrix(gr.get_granularity(labels[0], planes[0, 0], **kw))
    monkeypatch.setattr(gr, "reconstruction_by_dilation", counted)
    res = _matrix(gr.get_granularity(labels[0], planes[0, 0], **kw))
    assert np.array_equal(res, plain)  # the counting copy computes what the oracle's own loop computes
    cap = sh * sw // 2 + 64  # feat_granularity.hip: max_total
    assert len(sweeps) == kw["granular_spectrum_length"]
    for n in sweeps[:2]:
        assert 0.75 * (sh * sw / 2) <= n < cap, (sweeps, cap)
    # 16 sweeps per chunk, and one more chunk that changes nothing: still under the cap, so the kernel must not give up
    assert all((n // 16 + 1) * 16 < cap for n in sweeps)
    far = gc.SERPENTINE_FAR_END - 1
    assert 0.0 < res[far, 0] < 10.0  # about 100 if the propagation stopped before the path's end
    assert np.allclose(res[:, 0], [0.0, 1.6393, 4.4586, 1.3158], atol=5e-5)
    assert np.allclose(res[:, 2], [100.0, 98.36, 95.54, 98.68], atol=5e-3)
    assert (res[:, 1] == 0).all() and (res[:, 3] == 0).all()


def test_degenerate_cases_are_what_they_claim():
    labels, planes, kw = gc.degenerate()
    assert not (labels[0] == gc.DEGENERATE_ABSENT).any() and labels[0].max() > gc.DEGENERATE_ABSENT
    assert len(np.unique(planes[0, 0])) == 1 and len(np.unique(planes[0, 1])) == 2
    assert sorted((labels[0] == l).sum() for l in (5, 6, 7)) == [1, 1, 1] and labels[0, 0, 0] and labels[0, -1, -1]
    for f, l in gc.DEGENERATE_DARK:
        assert (labels[f] == l).any() and not planes[f][:, labels[f] == l].any()
        for c in range(planes.shape[1]):
            for mask in (dict(image_mask="frame"), dict(image_mask="objects", mask_order=1)):
                res = _matrix(gr.get_granularity(labels[f], planes[f, c], **kw, **mask))
                assert (res[l - 1] == 0.0).all()  # exactly: 0 * 100 / eps
    res = _matrix(gr.get_granularity(labels[0], planes[0, 0], **kw))  # the flat plane: everything goes in the first step
    present = np.arange(1, int(labels[0].max()) + 1) != gc.DEGENERATE_ABSENT
    assert (res[present, 0] == 100.0).all() and (res[present, 1:] == 0.0).all() and np.isnan(res[~present]).all()
    lab, _, _ = gc.whole_frame()
    assert (lab == 1).all()
    lab, _, _ = gc.label_65535()
    assert set(np.unique(lab)) == {0, 2, 65535}


def test_stride_case_exceeds_both_grid_caps():
    labels, planes, kw = gc.stride()
    F, Y, X = labels.shape
    _, (sh, sw), (bh, bw) = gc.geometry((Y, X), kw)
    assert F * sh * sw > 16384 * 256  # grid_for's cap: the [F, sh, sw] kernels must stride
    assert F * bh * bw <= 16384 * 256 < F * sh * sw
    assert sum(int(l.max()) for l in labels) > 65535  # k_gran_means' grid cap
    assert all((np.bincount(l.ravel())[1:] == gc.STRIDE_BLOCK ** 2).all() for l in labels[:2])
    flat = planes.reshape(F, -1)
    assert all(not np.array_equal(flat[a], flat[b]) for a in range(F) for b in range(a + 1, F))
    keep = gc.stride_subset()
    side = Y // gc.STRIDE_BLOCK
    assert len(keep) == len(set(keep)) == 256 and {1, side, side * (side - 1) + 1, side * side} <= set(keep)
    sub = gc.subset_labels(labels[0], keep)
    assert all(np.array_equal(sub == k + 1, labels[0] == l) for k, l in list(enumerate(keep))[::37])


@pytest.mark.parametrize("name", list(gc.BUILDERS))
def test_tolerance_bound(name):
    """4 * 100 * area_max * 2^-53 * (max pixel / min start) < 1e-9 (gc.tolerance_bound): the summation-order error of a
    float64 mean, as a percentage of the start value, stays under the tolerance the GPU tests compare with."""
    labels, planes, _ = gc.BUILDERS[name]()
    assert labels.dtype == np.uint16 and labels.ndim == 3 and planes.ndim == 4 and planes.shape[0] == labels.shape[0]
    assert planes.shape[2:] == labels.shape[1:]
    bound = gc.tolerance_bound(labels, planes, gc.STRIDE_ORACLE_FRAMES if name == "stride" else None)
    assert 0 < bound < 1e-9 and gc.RTOL == gc.ATOL == 1e-9, (name, bound)


def test_builders_are_deterministic():
    for name, build in gc.BUILDERS.items():
        if name == "stride":
            continue  # (its determinism is the seeded generator's, shown by the others; building it twice costs a second)
        a, b = build(), build()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], name
    a, b = gc.nondyadic("sub_both", 0), gc.nondyadic("sub_both", 1)
    assert not np.array_equal(a[1], b[1])
