"""
`FeatureEngine.granularity3d` on the GPU (aliby_amd/csrc/feat_granularity3d.hip) against tests/granularity3d_ref.py, the NumPy / SciPy
restatement that tests/test_cpu_granularity3d_ref.py pins to the 2-D oracle on one plane and to hand values.  Parity with
CellProfiler is unpinned (it cannot be run here).

Pass bar: the 2-D family's rule, RTOL = ATOL = 1e-9 with NaN exactly where the restatement has NaN; granularity3d_ref.tolerance_bound
(at most 8.2e-11 over the cases) is the figure under which that rule is justified.  Every comparison prints its worst excess over
the rule first (negative: inside it).  Rows are bitwise equal run to run, alone and in a batch, and for uint16 pixels and the same
integers as float32.
"""
import numpy as np
import pytest

from tests import granularity3d_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = ref.RTOL, ref.ATOL


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run(engine, vol, px, channel, counts, **kw):
    """-> float64 [sum counts, L] as NumPy, and the sweeps of every step"""
    import torch

    got = engine.granularity3d(torch.from_numpy(np.array(vol, order="C")).cuda(), torch.from_numpy(np.array(px, order="C")).cuda(), channel, list(counts), **kw)
    torch.cuda.synchronize()
    L = kw.get("granular_spectrum_length", 16)
    assert got.dtype == torch.float64 and tuple(got.shape) == (int(sum(counts)), L)
    return got.cpu().numpy(), list(engine.granularity3d_sweeps)


def compare(got, want, tag):
    assert got.shape == want.shape, tag
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, np.argwhere(np.isnan(got) != np.isnan(want))[:4])
    with np.errstate(invalid="ignore"):
        excess = np.abs(got - want) - (ATOL + RTOL * np.abs(want))
    finite = excess[np.isfinite(excess)]
    worst_abs = float(np.nanmax(np.abs(got - want))) if finite.size else 0.0
    print(f"granularity3d {tag}: {want.shape[0]} rows x {want.shape[1]}, {finite.size} finite, worst |difference| {worst_abs:.3e}, "
          f"worst excess over atol + rtol |want| {float(finite.max()) if finite.size else 0.0:.3e}")
    bad = np.argwhere(np.nan_to_num(excess, nan=-1.0) > 0)
    assert len(bad) == 0, (tag, [(int(r), int(c), got[r, c], want[r, c]) for r, c in bad[:6]])


def check_sweeps(sweeps, ref_sweeps, shape, kw, tag):
    """The kernels sweep in chunks of 16 and stop after a chunk that changed nothing, and the stacks of a batch run to the slowest:
    n changing sweeps of the restatement are (ceil(n / 16) + 1) * 16 of theirs.  (One chunk of slack: a tie that rounding breaks
    differently on the two sides may move a count across a chunk's end; the values are compared elsewhere.)"""
    need = [max(s[k] for s in ref_sweeps if s) for k in range(kw["granular_spectrum_length"])]
    print(f"granularity3d {tag}: sweeps {sweeps}, the restatement's changing sweeps {need}")
    assert all(s % 16 == 0 and abs(s - ((n + 15) // 16 + 1) * 16) <= 16 for s, n in zip(sweeps, need)), (tag, sweeps, need)
    assert max(sweeps) < ref.sweep_cap(shape, kw)


# ------------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name", sorted(ref.SMALL))
def test_parity(engine, name):
    vol, px, counts, kw = ref.case(name)
    for channel in range(px.shape[1]):
        got, sweeps = run(engine, vol, px, channel, counts, **kw)
        want, ref_sweeps, _ = ref.reference(name, channel)
        compare(got, want, f"{name} channel {channel}")
        check_sweeps(sweeps, ref_sweeps, vol.shape[1:], kw, name)


def test_corridor_is_carried_to_its_end(engine):
    vol, px, counts, kw = ref.case("corridor")
    got, sweeps = run(engine, vol, px, 0, counts, **kw)
    assert sweeps[0] >= 13 * 16  # more than 200 sweeps, a dozen reads of the flag
    far = got[ref.CORRIDOR_FAR_END - 1]
    assert 0 < far[0] < 10 and far[1] > 90


def test_hand_values(engine):
    kw = dict(subsample_size=1.0, image_sample_size=1.0, element_size=1, granular_spectrum_length=5)
    lab = np.zeros((1, 4, 6, 7), np.uint16)
    lab[0, 1:3, 1:4, 2:6] = 1
    lab[0, 3, 4:6, 0:3] = 3  # label 2 is absent
    const, _ = run(engine, lab, np.full((1, 1, 4, 6, 7), 1234, np.uint16), 0, [3], **kw)
    assert const[0].tolist() == [100.0, 0, 0, 0, 0] and const[2].tolist() == [100.0, 0, 0, 0, 0] and np.isnan(const[1]).all()
    px = np.full((1, 1, 4, 6, 7), 500, np.uint16)
    px[0, 0][lab[0] == 1] = 0
    dark, _ = run(engine, lab, px, 0, [3], **kw)
    assert dark[0].tolist() == [0.0] * 5 and dark[2].tolist() == [100.0, 0, 0, 0, 0] and np.isnan(dark[1]).all()
    assert run(engine, lab, px, 0, [2], **kw)[0].shape == (2, 5)  # label 3 lies above the count
    none, sweeps = run(engine, lab, px, 0, [0], **kw)              # no object: the empty block and no launch
    assert none.shape == (0, 5) and sweeps == [0] * 5


@pytest.mark.parametrize("shape, kw", [
    ((48, 64), dict(subsample_size=0.5, image_sample_size=0.5, element_size=3, granular_spectrum_length=6)),
    ((61, 45), dict(subsample_size=0.7, image_sample_size=0.5, element_size=2, granular_spectrum_length=4)),
    ((24, 20), dict(subsample_size=1.0, image_sample_size=1.0, element_size=2, granular_spectrum_length=3)),  # the un-resized background
])
def test_one_plane_is_the_2d_family(engine, shape, kw):
    """A stack of one plane against `engine.granularity` on that plane: the two instantiate the same kernels (csrc/granularity_pass.h),
    so bit for bit; and against the restatement under the rule."""
    import torch

    from aliby_amd.extraction.engine import to_device_planes, to_device_u16
    from tests import granularity_cases as cases2d

    lab, px = cases2d.ordinary_frame(shape, 1)
    n = int(lab.max())
    dl = to_device_u16(lab[None])
    dp, dt = to_device_planes(px[None, None])
    tab = engine.object_table(dl)
    out = engine.new_output(tab.n_obj, kw["granular_spectrum_length"])
    engine.granularity(dl, dp, dt, 0, tab, out, 0, **kw)
    torch.cuda.synchronize()
    got, _ = run(engine, lab[None, None], px[None, None, None], 0, [n], **kw)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(out.cpu().numpy()).view(np.uint64)), shape
    compare(got, ref.granularity3d(lab[None], px[None], n, **kw), f"one plane {shape} against the restatement")


# ------------------------------------------------------------------------------------------------------------ reproducibility
def test_rows_are_bitwise_reproducible(engine):
    vol, px, counts, kw = ref.case("batch")
    first, _ = run(engine, vol, px, 1, counts, **kw)
    again, _ = run(engine, vol, px, 1, counts, **kw)
    assert np.array_equal(bits(first), bits(again))
    lo = 0
    for f, n in enumerate(counts):  # a stack alone gives the rows it has in the batch (the middle one: none)
        alone, _ = run(engine, vol[f:f + 1], px[f:f + 1], 1, [n], **kw)
        assert np.array_equal(bits(alone), bits(first[lo:lo + n])), f
        lo += n
    other, _ = run(engine, vol[::-1], px[::-1], 1, counts[::-1], **kw)  # ... whatever its place in the batch
    assert np.array_equal(bits(other[:counts[2]]), bits(first[counts[0]:]))


@pytest.mark.parametrize("name", ["nondyadic-z", "faces"])
def test_uint16_and_the_same_integers_as_float32(engine, name):
    vol, px, counts, kw = ref.case(name)
    assert px.dtype == np.uint16
    a, _ = run(engine, vol, px, 0, counts, **kw)
    b, _ = run(engine, vol, px.astype(np.float32), 0, counts, **kw)
    assert np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------------------- grid-stride loops
@pytest.mark.parametrize("name", ["stride_voxels", "stride_voxels_coarse"])
def test_more_voxels_than_one_pass_of_the_image_grids(engine, name):
    """17 x 512 x 512 = 4 456 448 elements where the capped grids of the image kernels cover 16384 x 256 = 4 194 304 in one pass:
    k_g3_sample_stack, k_g3_morph, k_g3_subtract and k_g3_recon_sweep stride.  At sizes 1 / 1 with ball(1) every row is [100, 0]
    (granularity3d_ref.stride_voxels_coarse says why), so the same stack is measured with a coarser background as well."""
    vol, px, counts, kw = ref.case(name)
    got, sweeps = run(engine, vol, px, 0, counts, **kw)
    want, ref_sweeps, _ = ref.reference(name)
    compare(got, want, name)
    check_sweeps(sweeps, ref_sweeps, vol.shape[1:], kw, name)


def test_more_objects_than_the_object_grid_has_blocks(engine):
    """2 x 33489 one-voxel objects: 66 978 rows where k_g3_means has 65 535 blocks."""
    vol, px, counts, kw = ref.case("stride_objects")
    got, _ = run(engine, vol, px, 0, counts, **kw)
    compare(got, ref.reference("stride_objects")[0], "stride_objects")
    alone, _ = run(engine, vol[1:], px[1:], 0, counts[1:], **kw)
    assert np.array_equal(bits(alone), bits(got[counts[0]:]))


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_in_front_of_a_real_engine(engine):
    import torch

    vol, px, counts, kw = ref.case("faces")
    dv, dp = torch.from_numpy(np.array(vol)).cuda(), torch.from_numpy(np.array(px)).cuda()
    good, _ = run(engine, vol, px, 0, counts, **kw)

    def refused(exc, match, **over):
        args = dict(volume=dv, pixels=dp, channel=0, counts=list(counts), **kw)
        args.update(over)
        with pytest.raises(exc, match=match):
            engine.granularity3d(**args)

    refused(TypeError, "pixels must be uint16", pixels=dp.to(torch.float64))
    refused(TypeError, "must be uint16", volume=dv.to(torch.int32))
    refused(ValueError, r"pixels \[F,C,Z,Y,X\]", pixels=dp[..., :-1])
    refused(ValueError, "on the device", volume=dv.cpu())
    refused(ValueError, "counts must hold one label count", counts=[1, 2])
    refused(TypeError, "channel must be an integer", channel=0.0)
    refused(ValueError, "out of range for 1 channels", channel=1)
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        refused(ValueError, "subsample_size must be a finite number", subsample_size=bad)
        refused(ValueError, "image_sample_size must be a finite number", image_sample_size=bad)
    refused(TypeError, "element_size must be an integer", element_size=2.0)
    refused(TypeError, "granular_spectrum_length must be an integer", granular_spectrum_length=True)
    for bad in (0, 17):
        refused(ValueError, r"element_size must lie in 1\.\.16", element_size=bad)
    for bad in (0, 65):
        refused(ValueError, r"granular_spectrum_length must lie in 1\.\.64", granular_spectrum_length=bad)
    refused(ValueError, "sampled lengths must be above 1", subsample_size=0.05)
    refused(ValueError, "sampled lengths must be above 1", image_sample_size=0.05)
    refused(ValueError, "sampled lengths must be above 1", volume=dv[:, :, :1].contiguous(), pixels=dp[:, :, :, :1].contiguous())
    refused(TypeError, "unexpected keyword", image_mask="objects")
    # one plane is a volume, and the next call works
    assert engine.granularity3d(dv[:, :1].contiguous(), dp[:, :, :1].contiguous(), 0, list(counts), **kw).shape == (65535, 2)
    assert np.array_equal(bits(run(engine, vol, px, 0, counts, **kw)[0]), bits(good))
