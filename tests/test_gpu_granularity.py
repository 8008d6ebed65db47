"""
The granularity kernels (aliby_amd/csrc/feat_granularity.hip) on the edge cases of tests/granularity_cases.py, against
oracle/granularity_restated.py.  tests/test_cpu_granularity_cases.py shows, without a GPU, that each case is the edge it claims
to be and that its objects satisfy the bound under which the tolerance below is justified.

Both sides work in float64 and differ only in the order of sums and of the interpolation's products, so the comparison is
rtol = atol = 1e-9 on the percentages (granularity_cases.RTOL / ATOL; the older test_granularity_matches_oracle allows 1e-4).
Where the oracle gives NaN (absent label) or an exact 0 the kernel must give the same, exactly.

Every call writes into a matrix filled with a sentinel, with one foreign column before its own and two after, and the foreign
columns must come back untouched.
"""
import functools

import numpy as np
import pytest

from oracle import granularity_restated as gr
from tests import granularity_cases as gc

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
COL0, EXTRA = 1, 2


@functools.lru_cache(maxsize=None)
def case(name):
    labels, planes, kw = gc.BUILDERS[name]()
    for a in (labels, planes):
        a.setflags(write=False)
    return labels, planes, kw


def on_device(engine, labels, planes):
    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    dl = to_device_u16(labels)
    dp, dt = to_device_planes(planes)
    return dl, dp, dt, engine.object_table(dl)


def run(engine, dev, channel, **kw):
    """-> [n_obj, L] of one launch; checks the return value and the sentinel columns"""
    import torch

    dl, dp, dt, tab = dev
    L = kw.get("granular_spectrum_length", 16)
    out = engine.new_output(tab.n_obj, COL0 + L + EXTRA)
    out.fill_(SENTINEL)
    assert out.stride(0) > L
    assert engine.granularity(dl, dp, dt, channel, tab, out, COL0, **kw) == L  # (_lib.check raises unless the call returns OK)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, :COL0] == SENTINEL).all() and (got[:, COL0 + L:] == SENTINEL).all()
    return got[:, COL0:COL0 + L]


def oracle(labels, planes, channel, **kw):
    """-> [n_obj, L]: the oracle frame by frame, rows in the order of the object table"""
    rows = []
    for f in range(labels.shape[0]):
        res = gr.get_granularity(labels[f], planes[f, channel], **kw)
        rows.append(np.stack([res[k] for k in gr.names(kw["granular_spectrum_length"])], axis=1).reshape(int(labels[f].max()), len(res)))
    return np.concatenate(rows)


def compare(got, ref, what):
    assert got.shape == ref.shape, what
    nan, zero = np.isnan(ref), ref == 0.0
    assert np.array_equal(np.isnan(got), nan), what
    assert (got[zero] == 0.0).all(), (what, np.abs(got[zero]).max())
    rest = ~nan & ~zero
    err = np.abs(got[rest] - ref[rest]) - gc.RTOL * np.abs(ref[rest])
    assert (err <= gc.ATOL).all(), (what, "worst excess over rtol", float(err.max()), "worst abs", float(np.abs(got[rest] - ref[rest]).max()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


MASKS = {"frame": dict(image_mask="frame"), "objects": dict(image_mask="objects", mask_order=1)}


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name", list(gc.NONDYADIC))
def test_nondyadic_sample_sizes(engine, name, mask):
    """Sample sizes of 0.7 at shapes where i / 0.7 leaves the frame at the far edge and i * (1 / 0.7) does not (k_gran_sample_frame
    and k_gran_sample_mask in sub_*, k_gran_resample and k_gran_resample_mask in back_both), with objects on the last rows and
    columns.  Before the kernels divided as the reference does, every case but the control missed the oracle by tens of
    percentage points (the oracle's own reciprocal variant differs from it by 52 to 83 on these inputs)."""
    labels, planes, kw = case(f"nondyadic-{name}")
    dev = on_device(engine, labels, planes)
    for ch in range(planes.shape[1]):
        compare(run(engine, dev, ch, **kw, **MASKS[mask]), oracle(labels, planes, ch, **kw, **MASKS[mask]), (name, mask, ch))


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name", list(gc.OVERSHOOT))
def test_overshoot_shapes(engine, name, mask):
    """Shapes at which the up-resize coordinate of the last row / column rounds above the source's last index, so that the
    resized image reads 0 there, in the oracle and in the kernel alike; objects on the last row and column see it."""
    labels, planes, kw = case(f"overshoot-{name}")
    dev = on_device(engine, labels, planes)
    compare(run(engine, dev, 0, **kw, **MASKS[mask]), oracle(labels, planes, 0, **kw, **MASKS[mask]), (name, mask))


def test_serpentine_reconstruction(engine):
    """A path of about half the image's pixels: steps 1 and 2 need 985 and 986 Jacobi sweeps (62 chunks of 16, ping-pong buffers
    throughout) where the kernel gives up at 1216.  Then the same frame between two ordinary ones: a batch converges as one, and
    the extra sweeps of the other frames' fixed points change nothing."""
    labels, planes, kw = case("serpentine")
    alone = run(engine, on_device(engine, labels, planes), 0, **kw)
    ref = oracle(labels, planes, 0, **kw)
    compare(alone, ref, "serpentine")
    assert 0.0 < alone[gc.SERPENTINE_FAR_END - 1, 0] < 10.0
    around = [gc.ordinary_frame(labels.shape[1:], s) for s in (1, 2)]
    bl = np.stack([around[0][0], labels[0], around[1][0]])
    bp = np.stack([around[0][1], planes[0, 0], around[1][1]])[:, None]
    batch = run(engine, on_device(engine, bl, bp), 0, **kw)
    n0, n1 = int(bl[0].max()), int(bl[1].max())
    assert np.array_equal(bits(batch[n0:n0 + n1]), bits(alone))
    compare(batch, oracle(bl, bp, 0, **kw), "serpentine in a batch")


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("sizes", gc.MATRIX_SAMPLES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_mask_and_type_matrix(engine, sizes, mask):
    """float32 pixels, F = 3 with an empty middle frame, C = 3 (channels 0 and 2), both image masks, every combination of
    sampling and not sampling (with image_sample_size = 1 the background shares the subsampled mask)."""
    labels, planes, kw = case("matrix")
    assert planes.dtype == np.float32 and not labels[1].any()
    kw = dict(kw, subsample_size=sizes[0], image_sample_size=sizes[1])
    dev = on_device(engine, labels, planes)
    assert dev[3].n_obj == int(labels[0].max()) + int(labels[2].max())
    for ch in (0, 2):
        compare(run(engine, dev, ch, **kw, **MASKS[mask]), oracle(labels, planes, ch, **kw, **MASKS[mask]), (sizes, mask, ch))


@pytest.mark.parametrize("mask", list(MASKS))
def test_degenerate_pixels_and_labels(engine, mask):
    """A flat plane, two-level planes, all-zero objects (start = eps: exactly 0.0), an absent label (a NaN row), one-pixel
    objects, an object that is the whole frame, a label of 65535, and a batch without any label."""
    import torch

    labels, planes, kw = case("degenerate")
    dev = on_device(engine, labels, planes)
    n0 = int(labels[0].max())
    for ch in range(planes.shape[1]):
        got = run(engine, dev, ch, **kw, **MASKS[mask])
        compare(got, oracle(labels, planes, ch, **kw, **MASKS[mask]), ("degenerate", mask, ch))
        assert np.isnan(got[gc.DEGENERATE_ABSENT - 1]).all() and np.isnan(got).sum() == got.shape[1]
        for f, l in gc.DEGENERATE_DARK:
            assert (got[(n0 if f else 0) + l - 1] == 0.0).all()
    labels, planes, kw = case("whole_frame")
    dev = on_device(engine, labels, planes)
    for ch in range(planes.shape[1]):
        compare(run(engine, dev, ch, **kw, **MASKS[mask]), oracle(labels, planes, ch, **kw, **MASKS[mask]), ("whole frame", mask, ch))
    labels, planes, kw = case("label_65535")
    dev = on_device(engine, labels, planes)
    assert dev[3].n_obj == 65535
    got = run(engine, dev, 0, **kw, **MASKS[mask])
    compare(got, oracle(labels, planes, 0, **kw, **MASKS[mask]), ("label 65535", mask))
    assert not np.isnan(got[[1, 65534]]).any() and np.isnan(got).sum() == 65533 * got.shape[1]
    # no label at all: the call returns OK and writes nothing
    dev = on_device(engine, np.zeros_like(labels), planes)
    assert dev[3].n_obj == 0
    out = torch.full((4, 6), SENTINEL, dtype=torch.float64, device="cuda")
    assert engine.granularity(dev[0], dev[1], dev[2], 0, dev[3], out[:0], COL0, **kw, **MASKS[mask]) == kw["granular_spectrum_length"]
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_stride_loops(engine):
    """17 frames of 512 x 512: 4 456 448 elements where the capped grids of the image kernels cover 4 194 304 in one pass
    (k_gran_sample_frame, k_gran_subtract, k_gran_morph of the spectrum and k_gran_recon_sweep stride; the kernels on the
    background grid, a quarter of that here, do not), and 69 632 objects where k_gran_means has 65 535 blocks.  The batch must
    give the bits of 17 single-frame calls.  Frames 0 and 16 are compared with the oracle on 256 of their 4096 objects
    (granularity_cases.stride_subset: the oracle's loop over every label of a full-frame mask is too slow for all of them,
    and with the whole frame as image mask an object's result does not depend on the other labels)."""
    labels, planes, kw = case("stride")
    batch = run(engine, on_device(engine, labels, planes), 0, **kw)
    per = int(labels[0].max())
    assert batch.shape[0] == per * labels.shape[0] > 65535 and not np.isnan(batch).any()
    for f in range(labels.shape[0]):
        single = run(engine, on_device(engine, labels[f:f + 1], planes[f:f + 1]), 0, **kw)
        assert np.array_equal(bits(single), bits(batch[f * per:(f + 1) * per])), f
    keep = gc.stride_subset()
    rows = np.asarray(keep) - 1
    for f in gc.STRIDE_ORACLE_FRAMES:
        sub = gc.subset_labels(labels[f], keep)[None]
        compare(batch[f * per + rows], oracle(sub, planes[f:f + 1], 0, **kw), ("stride", f))


def test_refusals(engine):
    """Every ARG_CHECK of aliby_features_granularity that a caller of the engine can reach raises through _lib.check with the
    kernel's message and leaves the output alone; the call after a refusal works."""
    import torch

    labels, planes, kw = case("whole_frame")
    dev = on_device(engine, labels, planes)
    L = kw["granular_spectrum_length"]
    good = run(engine, dev, 1, **kw)

    def refused(message, on=dev, channel=1, cols=COL0 + L + EXTRA, col0=COL0, **over):
        out = torch.full((on[3].n_obj, cols), SENTINEL, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError, match=message):
            engine.granularity(on[0], on[1], on[2], channel, on[3], out, col0, **dict(kw, **over))
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENTINEL).all()
        assert np.array_equal(bits(run(engine, dev, 1, **kw)), bits(good))  # the next call works

    row = on_device(engine, np.ones((1, 1, 16), np.uint16), np.full((1, 1, 1, 16), 500, np.uint16))
    assert row[3].n_obj == 1
    refused("bad shape", on=row, channel=0)                                         # Y = 1
    column = on_device(engine, np.ones((1, 16, 1), np.uint16), np.full((1, 1, 16, 1), 500, np.uint16))
    refused("bad shape", on=column, channel=0)                                      # X = 1
    refused("frame too small for these sample sizes", subsample_size=0.25, image_sample_size=0.25)  # 12 x 16 -> 3 x 4 -> 1 x 1
    refused("frame too small for these sample sizes", subsample_size=0.05)           # sh = 1
    for bad in (0.0, -0.5, 1.5):
        refused(r"sample sizes must be in \(0, 1\]", subsample_size=bad)
        refused(r"sample sizes must be in \(0, 1\]", image_sample_size=bad)
    for bad in (0, 65):
        refused("element_size / spectrum length out of range", element_size=bad)
        refused("element_size / spectrum length out of range", granular_spectrum_length=bad, cols=80)
    refused("columns exceed row stride", cols=COL0 + L - 1)                          # col0 + L > ld
    refused("columns exceed row stride", col0=-1)
    for bad in (-1, planes.shape[1]):
        refused("channel out of range", channel=bad)
