"""
GPU parity of `FeatureEngine.intensity3d` (aliby_amd/csrc/feat_intensity3d.hip): the intensity moments of volume labels [F,Z,Y,X].
Compared with the exact reference tests/intensity3d_ref.py (Python integers and correctly rounded quotients; pinned to float64
NumPy and closed forms by tests/test_cpu_intensity3d_ref.py, which also checks the stated precondition of every input built here).
Parity with cp_measure / CellProfiler on volumes stays unpinned.

Rule (tests/intensity3d_ref.check): Volume, IntegratedIntensity, Min and Max bit for bit; mean and both centres bit for bit
wherever both operands of the quotient are below 2^53 (the kernel divides two exactly converted doubles, IEEE division is correctly
rounded, and the build has neither fast-math nor contraction), else within 1e-10; the std within 1e-10 and exactly 0.0 where the
variance is 0.  Every comparison prints the worst relative error of each float column.
"""
import numpy as np
import pytest

from tests import intensity3d_ref as ref
from tests.sizeshape3d_ref import random_labels

pytestmark = pytest.mark.gpu

C = ref.COL
XV = "Location_CenterMassIntensity_X"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run(engine, vols, pixels, channel=0, counts=None):
    """vols [F][Z,Y,X], pixels uint16 [F,C,Z,Y,X] -> (float64 [sum counts, 12] from the GPU, counts)."""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    counts = [int(v.max()) for v in stack] if counts is None else [int(c) for c in counts]
    got = engine.intensity3d(torch.from_numpy(stack).cuda(), torch.from_numpy(np.ascontiguousarray(pixels)).cuda(), channel, counts)
    assert got.dtype == torch.float64 and tuple(got.shape) == (sum(counts), 12)
    return got.cpu().numpy(), counts


def _dirty_the_scratch(engine):
    """An unrelated call that leaves other bytes in the context scratch the accumulators are carved from."""
    import torch

    vol, _ = random_labels(99, (6, 40, 44))
    engine.sizeshape3d(torch.from_numpy(vol[None]).cuda(), [int(vol.max())])


# ------------------------------------------------------------------------------------------------ 1. irregular touching labels
@pytest.mark.parametrize("seed,shape", ref.IRREGULAR_SHAPES)
def test_irregular_touching_labels(engine, seed, shape):
    """X = 1, 15, 16, 17, 31 and 130 (below, at and above the 16-voxel segment, with and without a tail), Z = 1 among them; pixels
    over the whole uint16 range; three channels, the last one read."""
    vol, n = random_labels(seed, shape)
    px = ref.full_range_pixels(seed, vol)
    got, counts = _run(engine, [vol], px[None], channel=2)
    assert counts == [n]
    want, sums = ref.intensity3d(vol, px[2], n)
    ref.check(got, want, sums, f"irregular {shape}")
    other, _ = _run(engine, [vol], px[None], channel=0)
    assert not np.array_equal(other[:, C["Intensity_IntegratedIntensity"]], got[:, C["Intensity_IntegratedIntensity"]])  # the channel is read


# ------------------------------------------------------------------------------------------------ 2. large sums
@pytest.mark.parametrize("kind,std", [("one_zero", None), ("alternating", 0.5), ("constant", 0.0), ("half_dark", 32767.5), ("nearly_constant", None)])
def test_large_sums_of_a_bright_box(engine, kind, std):
    """263 168 voxels at or near 65535: both products of the variance numerator are above 2^64 ("half_dark": the numerator too),
    and "nearly_constant" is where a float64 moment form would keep six digits."""
    vol, px = ref.bright_box(kind)
    got, _ = _run(engine, [vol], px[None])
    want, sums = ref.intensity3d(vol, px[0], 1)
    assert sums[0]["n"] * sums[0]["s2"] >= 1 << 64
    ref.check(got, want, sums, f"bright box {kind}")
    n = sums[0]["n"]
    if kind == "one_zero":
        assert abs(got[0, ref.STD] - 65535.0 * np.sqrt(n - 1.0) / n) <= ref.RTOL * got[0, ref.STD]  # the closed form
    if std is not None:
        assert _bits(got[0, ref.STD]) == _bits(np.float64(std)), (kind, got[0, ref.STD])


def test_the_widest_stack_with_sum_xv_above_2_53(engine):
    vol, px = ref.widest_stack()
    got, _ = _run(engine, [vol], px[None])
    want, sums = ref.intensity3d(vol, px[0], 2)
    assert sums[0]["xv"] >= ref.TWO53
    ref.check(got, want, sums, "X = 65536", above_2_53=(XV,))  # every other quotient, and the whole of row 2, bit for bit
    assert got[1, C["Location_Center_X"]] == 65532.5


# ------------------------------------------------------------------------------------------------ 3. run structure
def test_worst_case_runs_one_voxel_and_all_zero_pixels(engine):
    vol, n, px = ref.run_structure()
    got, _ = _run(engine, [vol], px[None], counts=[n])
    want, sums = ref.intensity3d(vol, px[0], n)
    ref.check(got, want, sums, "run structure")
    assert got[3, C["Volume"]] == 1 and got[3, ref.STD] == 0.0
    assert np.isnan(got[4, 6:9]).all() and np.isfinite(got[4, 9:]).all() and got[4, C["Intensity_IntegratedIntensity"]] == 0.0


# ------------------------------------------------------------------------------------------------ 4. batches
def _split_batch():
    """The batch of the sibling suites (tests/coloc3d_ref.split_batch): a label in two pieces, an empty stack, two absent labels."""
    from tests import coloc3d_ref

    return coloc3d_ref.split_batch()


def test_a_batch_with_a_split_label_an_empty_stack_and_absent_labels(engine):
    from scipy import ndimage as ndi

    vols, counts, px = _split_batch()
    assert ndi.label(vols[0] == 1, structure=np.ones((3, 3, 3)))[1] >= 2 and not vols[1].any() and counts[2] == int(vols[2].max()) + 2
    got, _ = _run(engine, vols, px, channel=1, counts=counts)
    want, sums = ref.intensity3d_batch(vols, px, 1, counts)
    ref.check(got, want, sums, "batch of three")
    assert (got[-2:, 0] == 0.0).all() and np.isnan(got[-2:, 1:]).all()  # announced, absent: Volume 0, NaN elsewhere
    got0, _ = _run(engine, [vols[1]], px[1:2], counts=[0])  # F = 1 with zero objects: an empty block
    assert got0.shape == (0, 12)


def test_labels_above_the_count_change_no_row_of_either_stack(engine):
    shape = (5, 33, 47)
    a, na = random_labels(51, shape, n_seeds=10)
    b, nb = random_labels(52, shape, n_seeds=6)
    assert na >= 6 and nb >= 3
    keep = na - 3  # stack 0 announces fewer labels than it holds: its last three would land on stack 1's first rows
    px = np.stack([ref.full_range_pixels(51, a, 1), ref.full_range_pixels(52, b, 1)])
    got, _ = _run(engine, [a, b], px, counts=[keep, nb])
    want, sums = ref.intensity3d_batch([a, b], px, 0, [keep, nb])
    assert int((a > keep).sum()) > 0 and all(s["n"] > 0 for s in sums[keep:keep + 3])
    ref.check(got, want, sums, "labels above the count")
    erased = np.where(a > keep, 0, a).astype(np.uint16)
    clean, _ = _run(engine, [erased, b], px, counts=[keep, nb])
    assert np.array_equal(_bits(got), _bits(clean))
    # and the last stack's surplus labels fall off the end of the table without a trace
    tail, _ = _run(engine, [b, a], px[::-1], counts=[nb, keep])
    assert np.array_equal(_bits(tail), _bits(np.concatenate([got[keep:], got[:keep]])))


# ------------------------------------------------------------------------------------------------ 5. bitwise independence
def test_rows_are_bitwise_independent_of_run_batch_and_neighbours(engine):
    shape = (6, 37, 53)
    a, na = random_labels(61, shape)
    b, nb = random_labels(62, shape, n_seeds=20)
    pa, pb = ref.full_range_pixels(61, a, 2), ref.full_range_pixels(62, b, 2)
    alone, _ = _run(engine, [a], pa[None], channel=1)
    want, sums = ref.intensity3d(a, pa[1], na)
    ref.check(alone, want, sums, "independence")
    both, _ = _run(engine, [b, a, b], np.stack([pb, pa, pb]), channel=1)  # at another index, between other stacks
    assert np.array_equal(_bits(both[nb:nb + na]), _bits(alone))
    one_b, _ = _run(engine, [b], pb[None], channel=1)
    assert np.array_equal(_bits(both[:nb]), _bits(one_b)) and np.array_equal(_bits(both[nb + na:]), _bits(one_b))
    # its neighbours erased, or relabelled above the count: the first rows keep their bits
    keep = na // 2
    erased = np.where(a > keep, 0, a).astype(np.uint16)
    lifted = np.where(a > keep, a + 1000, a).astype(np.uint16)
    for name, v in (("erased", erased), ("relabelled", lifted)):
        part, _ = _run(engine, [v], pa[None], channel=1, counts=[keep])
        assert np.array_equal(_bits(part), _bits(alone[:keep])), name
    _dirty_the_scratch(engine)
    again, _ = _run(engine, [a], pa[None], channel=1)
    assert np.array_equal(_bits(again), _bits(alone))


# ------------------------------------------------------------------------------------------------ 6. placement and refusals
def test_rows_at_a_column_offset_leave_the_rest_of_the_table_alone(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    vol, n = random_labels(71, (4, 21, 35), n_seeds=6)
    px = ref.full_range_pixels(71, vol, 2)
    want, sums = ref.intensity3d(vol, px[1], n + 1)
    lab, pix = torch.from_numpy(vol[None]).cuda(), torch.from_numpy(px[None]).cuda()
    ld, col0, fill = 29, 7, -123.25
    out = torch.full((n + 3, ld), fill, dtype=torch.float64, device="cuda")  # two rows more than are written
    off = np.asarray([0, n + 1], np.int32)
    _lib.check(engine.lib.aliby_features_intensity3d(engine.ctx.handle, _ptr(lab), _ptr(pix), 1, 2, *vol.shape, 1, _ptr(off), _ptr(out), ld, col0,
                                                     _stream_ptr()))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    ref.check(np.ascontiguousarray(host[:n + 1, col0:col0 + 12]), want, sums, "col0 = 7 of 29")
    host[:n + 1, col0:col0 + 12] = fill
    assert (host == fill).all()


def test_the_c_entry_refuses_before_anything_is_written(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    lab = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    lab[0, :, 2:5, 2:5] = 1
    px = torch.full((1, 2, 2, 8, 8), 9, dtype=torch.uint16, device="cuda")
    out = torch.zeros((1, 16), dtype=torch.float64, device="cuda")
    good_off = np.asarray([0, 1], np.int32)
    fn, h = engine.lib.aliby_features_intensity3d, engine.ctx.handle

    def call(labels=lab, pixels=px, shape=(1, 2, 2, 8, 8), channel=0, off=good_off, o=out, ld=16, col0=0):
        F, Cn, Z, Y, X = shape
        return fn(h, _ptr(labels) if labels is not None else 0, _ptr(pixels) if pixels is not None else 0, F, Cn, Z, Y, X, channel,
                  _ptr(off) if off is not None else 0, _ptr(o) if o is not None else 0, ld, col0, _stream_ptr())

    # (X = 65537 is refused on its shape alone: the entry reads no voxel before it returns; offsets that do not grow:
    # tests/test_gpu_volume.py::test_intensity3d_refuses_offsets_it_cannot_hold)
    for bad in (dict(ld=11), dict(ld=16, col0=5), dict(col0=-1), dict(channel=2), dict(channel=-1), dict(shape=(1, 2, 1, 1, 65537)),
                dict(shape=(1, 2, 0, 8, 8)), dict(labels=None), dict(pixels=None), dict(o=None), dict(off=None)):
        with pytest.raises(Exception):
            _lib.check(call(**bad))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # refused before anything was written
    _lib.check(call(col0=4))
    row = out.cpu().numpy()[0]
    assert (row[:4] == 0.0).all() and row[4] == 18 and row[5] == 18 * 9 and row[6] == 9.0 and row[7] == 0.0 and row[4 + 9] == 3.0


def test_python_refuses_bad_arguments_before_any_launch(engine):
    import torch

    vol = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    vol[0, :, 2:5, 2:5] = 1
    px = torch.ones((1, 2, 2, 8, 8), dtype=torch.uint16, device="cuda")
    ok = engine.intensity3d(vol, px, 1, [1])
    assert tuple(ok.shape) == (1, 12) and float(ok[0, 0]) == 18.0
    for channel in (2, -1):
        with pytest.raises(ValueError):
            engine.intensity3d(vol, px, channel, [1])
    for channel in (0.0, True, None):
        with pytest.raises(TypeError):
            engine.intensity3d(vol, px, channel, [1])
    with pytest.raises(ValueError):
        engine.intensity3d(vol, px, 0, [1, 1])
    with pytest.raises(ValueError):
        engine.intensity3d(vol, px[:, :, :1], 0, [1])  # another Z
    with pytest.raises(ValueError):
        engine.intensity3d(vol[0], px, 0, [1])  # labels of rank 3
    with pytest.raises(ValueError):
        engine.intensity3d(vol, px[:, 0], 0, [1])  # pixels of rank 4
    with pytest.raises(ValueError):
        engine.intensity3d(vol.cpu(), px, 0, [1])  # labels on the host
    with pytest.raises(ValueError):
        engine.intensity3d(vol, px.cpu(), 0, [1])
    with pytest.raises(TypeError):
        engine.intensity3d(vol.to(torch.int32), px, 0, [1])
    for dtype in (torch.float32, torch.float64, torch.int16, torch.int32):  # uint16 only: the family has no float form
        with pytest.raises(TypeError):
            engine.intensity3d(vol, px.to(dtype), 0, [1])
    with pytest.raises(TypeError):
        engine.intensity3d(vol.cpu().numpy(), px, 0, [1])
    with pytest.raises(TypeError):
        engine.intensity3d(vol, px.cpu().numpy(), 0, [1])


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_labels_of_the_segmenter_go_straight_into_intensity3d(engine):
    import torch

    from aliby_amd.segment.dispatch import dispatch_segmenter
    from tests import coloc3d_ref

    f, gt, dP, prob = coloc3d_ref.segmenter_case()

    def override(x):
        assert tuple(x.shape[1:]) == gt.shape
        return torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()

    segment = dispatch_segmenter(kind="cellpose", channel_to_segment=0, volume_mode="flows3d", setup_params=dict(flows_override=override))
    segment(f["pixels"][None], do_3D=True)
    volume, counts = segment.last_volume
    assert volume.dtype == torch.uint16 and volume.is_cuda and int(counts[0]) > 0
    labels = volume[0].cpu().numpy()
    assert int(labels.max()) == int(counts[0])
    px = torch.from_numpy(f["pixels"][None]).cuda()
    for c in range(f["pixels"].shape[0]):
        got = engine.intensity3d(volume, px, c, counts)
        want, sums = ref.intensity3d(labels, f["pixels"][c], int(counts[0]))
        ref.check(got, want, sums, f"segmenter, channel {c}")
