"""
tests/granularity3d_ref.py without a GPU: the restatement against the 2-D oracle on one plane (bitwise), against hand values and
against scipy.ndimage for its own dilation; every case builder is the edge it claims to be; `tolerance_bound` stays below the rule
the GPU file asserts; and the host checks of `FeatureEngine.granularity3d`, on an engine that was never initialised (a refusal
that came after any device work would fail on the missing attribute instead, tests/test_cpu_volume_args.py).
"""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from aliby_amd.extraction import features as feat
from aliby_amd.extraction.engine import FeatureEngine
from oracle import granularity_restated as oracle2d
from tests import granularity3d_ref as ref
from tests import granularity_cases as cases2d


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_the_shifted_maxima_are_ndimage_dilation():
    rng = np.random.default_rng(0)
    for shape in ((4, 5, 6), (1, 7, 3), (3, 1, 1)):
        a = rng.random(shape)
        assert np.array_equal(ref.dilate_ball1(a), ndi.grey_dilation(a, footprint=ref.ball(1), mode="constant", cval=-np.inf))
    assert ref.ball(1).sum() == 7 and ref.ball(2).sum() == 33 and ref.ball(16).sum() == 17077


@pytest.mark.parametrize("shape, kw", [
    ((48, 64), dict(subsample_size=0.5, image_sample_size=0.5, element_size=3, granular_spectrum_length=6)),
    ((61, 45), dict(subsample_size=0.7, image_sample_size=0.5, element_size=2, granular_spectrum_length=4)),
    ((40, 52), dict(subsample_size=0.25, image_sample_size=0.25, element_size=10, granular_spectrum_length=3)),
])
def test_one_plane_is_the_2d_oracle(shape, kw):
    """With the length-1 rule a stack of one plane is the 2-D family: bit for bit with the 2-D means (label by label), and within
    the bound with the bincount means the GPU file compares against."""
    lab, px = cases2d.ordinary_frame(shape, 1)
    n = int(lab.max())
    want = oracle2d.get_granularity(lab, px, image_mask="frame", **kw)
    want = np.stack([want[k] for k in oracle2d.names(kw["granular_spectrum_length"])], 1)
    got = ref.granularity3d(lab[None], px[None], n, means="mask", **kw)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.abs(want).max() > 1 and len(np.unique(want)) > n  # (not a degenerate spectrum)
    fast = ref.granularity3d(lab[None], px[None], n, **kw)
    assert np.abs(fast - want).max() <= ref.tolerance_bound(lab[None, None], px[None, None, None], [n]) < ref.ATOL


def test_hand_values():
    kw = dict(subsample_size=1.0, image_sample_size=1.0, element_size=1, granular_spectrum_length=5)
    lab = np.zeros((4, 6, 7), np.uint16)
    lab[1:3, 1:4, 2:6] = 1
    lab[3, 4:6, 0:3] = 3  # label 2 is absent
    const = ref.granularity3d(lab, np.full(lab.shape, 1234, np.uint16), 3, **kw)
    assert const[0].tolist() == [100.0, 0, 0, 0, 0] and const[2].tolist() == [100.0, 0, 0, 0, 0] and np.isnan(const[1]).all()
    px = np.full(lab.shape, 500, np.uint16)
    px[lab == 1] = 0
    dark = ref.granularity3d(lab, px, 3, **kw)
    assert dark[0].tolist() == [0.0] * 5 and dark[2].tolist() == [100.0, 0, 0, 0, 0] and np.isnan(dark[1]).all()
    assert ref.granularity3d(lab, px, 0, **kw).shape == (0, 5)
    assert ref.granularity3d(lab, px, 2, **kw).shape == (2, 5)  # label 3 lies above the count: not measured
    assert ref.names(3) == ["Granularity_1", "Granularity_2", "Granularity_3"]


def test_the_length_one_rule():
    """the resize coordinate of a destination axis of length 1 is 0, whatever the source length"""
    g = ref._resize_coords((1, 3, 3), (1, 10, 12))
    assert (g[0] == 0).all() and g[1].max() == 9 * (2 / 9) and g[2].max() == 11 * (2 / 11)
    assert (ref._resize_coords((3, 5, 5), (1, 9, 9))[0] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ the cases
def _critical(n, size):
    """the far edge of an axis of length n: the last sampled position by division and by the reciprocal fall on different sides of n - 1"""
    i = ref.sampled_shape((n,), size)[0] - 1
    return (i / size <= n - 1) != (i * (1 / size) <= n - 1)


@pytest.mark.parametrize("name", sorted(ref.NONDYADIC))
def test_nondyadic_cases_are_critical_on_their_axis_only(name):
    shape, axis = ref.NONDYADIC[name]
    size = ref.NONDYADIC_KW["subsample_size"]
    assert size == 0.7 and [_critical(n, size) for n in shape] == [a == axis for a in range(3)]
    assert all(8 <= n <= 16 for a, n in enumerate(shape) if a != axis)
    vol, px, counts, kw = ref.case(f"nondyadic-{name}")
    # the last sampled plane is the stack's far plane by one quotient and 0 by the other (which is which depends on the length),
    # the restatement follows the division, and an object lies on the far plane
    n, i = shape[axis], ref.sampled_shape((shape[axis],), size)[0] - 1
    read = i / size <= n - 1
    assert read != (i * (1 / size) <= n - 1)
    assert np.take(vol[0], n - 1, axis=axis).any() and px.min() > 0
    sub = ndi.map_coordinates(px[0, 0].astype(float), ref._sample_coords(ref.geometry(shape, kw)[1], size), order=1)
    last = np.take(sub, i, axis=axis)
    assert last.max() > 0 if read else (last == 0).all()


def test_flat_background_case():
    vol, px, counts, kw = ref.case("flat_background")
    assert kw == dict(subsample_size=0.25, image_sample_size=0.25, element_size=10, granular_spectrum_length=16)
    assert ref.geometry(vol.shape[1:], kw) == ((12, 40, 48), (3, 10, 12), (1, 3, 3))
    assert kw["element_size"] > max(ref.geometry(vol.shape[1:], kw)[2])
    want, sweeps, _ = ref.reference("flat_background")
    assert np.isfinite(want).all() and (np.abs(want) > 1e-6).sum() > want.shape[0] * 4
    assert max(sweeps[0]) < ref.sweep_cap(vol.shape[1:], kw) - 16


def test_corridor_case():
    vol, px, counts, kw = ref.case("corridor")
    assert vol.shape == (1, 6, 16, 16)
    want, sweeps, _ = ref.reference("corridor")
    cap = ref.sweep_cap(vol.shape[1:], kw)
    assert cap == 6 * 16 * 16 // 2 + 64
    assert 200 <= sweeps[0][0] < cap - 16 and sweeps[0][0] > 3 * 16  # several chunks of 16, and below the cap
    # the far end keeps its 1000 in step 1 only if the value was carried all the way: it loses just its bump there
    far = want[ref.CORRIDOR_FAR_END - 1]
    assert 0 < far[0] < 10 and far[1] > 90
    # the corridor is one voxel wide: step 1's erosion leaves the blob's core and nothing else
    ero = ndi.grey_erosion(px[0, 0].astype(float), footprint=ref.ball(1))
    core = np.zeros(ero.shape, bool)
    core[0, 2:7, 2:7] = True
    assert (ero[0, 3:6, 3:6] == 3000).all() and not ero[~core].any() and not ero[vol[0] == ref.CORRIDOR_FAR_END].any()


def test_batch_case():
    vol, px, counts, kw = ref.case("batch")
    assert px.dtype == np.float32 and px.shape[:2] == (3, 2) and 0 < px.min() and px.max() <= 1
    assert counts == (7, 0, 5) and not vol[1].any() and all(n % 4 for n in vol.shape[1:])
    for f in (0, 2):
        assert set(np.unique(vol[f])) == set(range(counts[f] + 1))
    for c in range(2):
        want = ref.reference("batch", c)[0]
        assert want.shape == (12, 4) and np.isfinite(want).all()
    assert not np.array_equal(ref.reference("batch", 0)[0], ref.reference("batch", 1)[0])


def test_faces_case():
    vol, px, counts, kw = ref.case("faces")
    assert counts == (65535,) and set(np.unique(vol)) == {0, 2, 65535}
    Z, Y, X = vol.shape[1:]
    for lab, planes in ((2, (vol[0, 0], vol[0, :, 0], vol[0, :, :, 0])), (65535, (vol[0, Z - 1], vol[0, :, Y - 1], vol[0, :, :, X - 1]))):
        assert all((p == lab).any() for p in planes)
    want = ref.reference("faces")[0]
    present = ~np.isnan(want).any(1)
    assert want.shape == (65535, 2) and np.flatnonzero(present).tolist() == [1, 65534] and np.isnan(want[~present]).all()


def test_stride_cases():
    vol, px, counts, kw = ref.case("stride_voxels")
    assert kw == dict(subsample_size=1.0, image_sample_size=1.0, element_size=1, granular_spectrum_length=2)
    assert vol[0].size > 16384 * 256 and ref.geometry(vol.shape[1:], kw)[2] == vol.shape[1:]  # every image grid strides
    assert len(np.unique(vol[0, :, :16, :16])) == 5 and counts == (5120,)
    want, sweeps, seconds = ref.reference("stride_voxels")
    print(f"granularity3d reference, stride_voxels {vol.shape[1:]}: {seconds:.1f} s, sweeps {sweeps}")
    assert seconds < 20
    assert (want == [100.0, 0.0]).all()  # (what sizes 1 / 1 with ball(1) always give: stride_voxels_coarse's docstring)
    kw2 = ref.case("stride_voxels_coarse")[3]
    want2, sweeps2, seconds2 = ref.reference("stride_voxels_coarse")
    print(f"granularity3d reference, stride_voxels_coarse: {seconds2:.1f} s, sweeps {sweeps2}")
    assert seconds2 < 20 and 16 < sweeps2[0][0] < 200 and len(np.unique(want2[:, 0])) > 1000 and np.isfinite(want2).all()
    assert ref.geometry(vol.shape[1:], kw2)[1] == vol.shape[1:]
    vol, px, counts, kw = ref.case("stride_objects")
    assert sum(counts) > 65535 and all(n <= 65535 for n in counts)
    assert all((np.bincount(vol[f].ravel())[1:] == 1).all() for f in range(2))  # one voxel each
    want = ref.reference("stride_objects")[0]
    assert want.shape == (sum(counts), 2) and np.isfinite(want).all() and len(np.unique(want[:, 0])) > 1000


@pytest.mark.parametrize("name", sorted(ref.BUILDERS))
def test_the_bound_stays_below_the_rule(name):
    vol, px, counts, kw = ref.case(name)
    bound = ref.tolerance_bound(vol, px, counts)
    print(f"{name}: tolerance bound {bound:.2e}")
    assert 0 < bound < ref.ATOL == ref.RTOL == 1e-9
    for f, n in enumerate(counts):  # no all-zero object: the bound covers every present row
        lab = np.where(vol[f] <= n, vol[f], 0).ravel()
        area = np.bincount(lab)[1:]
        for c in range(px.shape[1]):
            assert (np.bincount(lab, weights=px[f, c].ravel().astype(float))[1:][area > 0] > 0).all()


# ------------------------------------------------------------------------------------------------------------- the host checks
class _Resident(torch.Tensor):
    is_cuda = True


def _resident(t):
    return t.as_subclass(_Resident)


F, C, Z, Y, X = 2, 2, 3, 40, 48
VOL = _resident(torch.zeros((F, Z, Y, X), dtype=torch.uint16))
PIX = _resident(torch.zeros((F, C, Z, Y, X), dtype=torch.uint16))
ENGINE = object.__new__(FeatureEngine)  # no __init__: no device


def call(**kw):
    args = dict(volume=VOL, pixels=PIX, channel=0, counts=[1, 2])
    args.update(kw)
    return ENGINE.granularity3d(**args)


def test_good_arguments_reach_the_device():
    for kw in (dict(), dict(pixels=_resident(torch.zeros((F, C, Z, Y, X), dtype=torch.float32))), dict(subsample_size=1, image_sample_size=1.0),
               dict(element_size=16, granular_spectrum_length=64), dict(element_size=np.int64(1), granular_spectrum_length=np.uint8(1)),
               dict(volume=_resident(torch.zeros((F, 1, Y, X), dtype=torch.uint16)), pixels=_resident(torch.zeros((F, C, 1, Y, X), dtype=torch.uint16)))):
        with pytest.raises(AttributeError):  # the uninitialised engine has no device to allocate the result on
            call(**kw)


def test_refusals_in_their_order():
    bad_size, bad_element, small = dict(subsample_size=0.0), dict(element_size=17), dict(subsample_size=0.1, image_sample_size=0.1)
    # 1. types and shapes
    with pytest.raises(TypeError, match="pixels must be uint16"):
        call(pixels=_resident(torch.zeros((F, C, Z, Y, X), dtype=torch.float64)), channel=C, **bad_size, **bad_element)
    with pytest.raises(TypeError, match="must be uint16"):
        call(volume=_resident(torch.zeros((F, Z, Y, X), dtype=torch.int32)), channel=C)
    with pytest.raises(ValueError, match=r"pixels \[F,C,Z,Y,X\]"):
        call(pixels=_resident(torch.zeros((F, C, Z, Y, X + 1), dtype=torch.uint16)), channel=C)
    with pytest.raises(ValueError, match="counts must hold one label count"):
        call(counts=[1], channel=C)
    # 2. the channel
    for bad in (True, 0.0, "0", None):
        with pytest.raises(TypeError, match="channel must be an integer"):
            call(channel=bad, **bad_size)
    for bad in (C, -1):
        with pytest.raises(ValueError, match=f"out of range for {C} channels"):
            call(channel=bad, **bad_size)
    # 3. the sample sizes
    for name in ("subsample_size", "image_sample_size"):
        for bad in (0.0, -0.25, 1.5, float("nan"), float("inf"), "0.25", None, True):
            with pytest.raises(ValueError, match=f"{name} must be a finite number in"):
                call(**{name: bad}, element_size=2.0)
    # 4. the element and the length
    for name in ("element_size", "granular_spectrum_length"):
        for bad in (True, False, 2.0, "2", None):
            with pytest.raises(TypeError, match=f"{name} must be an integer"):
                call(**{name: bad}, **small)
    for bad in (0, -1, 17, feat.GRANULARITY3D_MAX_ELEMENT + 1):
        with pytest.raises(ValueError, match=r"element_size must lie in 1\.\.16"):
            call(element_size=bad, **small)
    for bad in (0, -3, 65):
        with pytest.raises(ValueError, match=r"granular_spectrum_length must lie in 1\.\.64"):
            call(granular_spectrum_length=bad, **small)
    # 5. Y, X and their sampled lengths
    for kw in (small, dict(subsample_size=0.02, image_sample_size=1.0), dict(subsample_size=1.0, image_sample_size=0.02)):
        with pytest.raises(ValueError, match="sampled lengths must be above 1"):
            call(**kw)
    thin = dict(volume=_resident(torch.zeros((F, Z, 1, X), dtype=torch.uint16)), pixels=_resident(torch.zeros((F, C, Z, 1, X), dtype=torch.uint16)))
    with pytest.raises(ValueError, match="sampled lengths must be above 1"):
        call(subsample_size=1.0, image_sample_size=1.0, **thin)
    # there is no image mask to choose
    for kw in (dict(image_mask="objects"), dict(image_mask="frame"), dict(mask_order=1)):
        with pytest.raises(TypeError, match="unexpected keyword"):
            call(**kw)


def test_names_and_shapes():
    assert feat.granularity3d_names() == feat.granularity_names(16) == [f"Granularity_{i}" for i in range(1, 17)]
    assert feat.granularity3d_names(3) == ref.names(3) == oracle2d.names(3)
    assert len(feat.granularity3d_names(64)) == 64 and feat.granularity3d_names(np.int32(2)) == ["Granularity_1", "Granularity_2"]
    for bad in (0, 65):
        with pytest.raises(ValueError):
            feat.granularity3d_names(bad)
    for bad in (True, 2.0, "2"):
        with pytest.raises(TypeError):
            feat.granularity3d_names(bad)
    assert (feat.GRANULARITY3D_MAX_ELEMENT, feat.GRANULARITY3D_MAX_LENGTH) == (16, 64)
    for shape, sizes in (((12, 40, 48), (0.25, 0.25)), ((61, 12, 16), (0.7, 0.5)), ((1, 45, 54), (1.0, 0.5)), ((9, 14, 121), (0.7, 0.7))):
        kw = dict(subsample_size=sizes[0], image_sample_size=sizes[1])
        assert FeatureEngine._granularity3d_shapes(*shape, *sizes) == ref.geometry(shape, kw)[1:]
        assert ref.geometry(shape[1:], kw) == cases2d.geometry(shape[1:], kw)
