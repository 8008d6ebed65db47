"""
GPU parity of `FeatureEngine.sizeshape3d` (aliby_amd/csrc/feat_sizeshape3d.hip): size and shape of volume labels [F,Z,Y,X].
Compared with the float64 / Python-int restatement tests/sizeshape3d_ref.py (itself pinned to scipy.ndimage, numpy.cov + eigvalsh,
a solid ellipsoid's closed form and known topologies by tests/test_cpu_sizeshape3d_ref.py) and with `intensity3d` for the columns
both families share.  Parity with cp_measure / CellProfiler stays unpinned (not installable offline).

Rule (README "Parity"): integer-valued columns bit-exact, float columns within 1e-4 relative.  Two columns need an absolute floor
next to the relative bound, because they can be analytically zero while both sides compute rounding noise: the smallest
eigenvalue c_min of a rank-deficient covariance (a flat or straight object).  A float64 symmetric eigensolver returns eigenvalues
with an absolute error of a small multiple of eps * c_max; taking 64 eps, MinorAxisLength = sqrt(20 c_min) is off by at most
sqrt(20 * 64 eps * c_max) = sqrt(64 eps) * MajorAxisLength (1.2e-7 of the major axis), and an inertia eigenvalue by 64 eps * tr(C).
Those floors come from the number format, not from what the kernel returns.
"""
import numpy as np
import pytest

from aliby_amd import synth
from tests import sizeshape3d_ref as ref

pytestmark = pytest.mark.gpu

C = ref.COL
RTOL = 1e-4
EPS = float(np.finfo(np.float64).eps)
EXACT = [C[k] for k in ref.NAMES if k.startswith("BoundingBoxM")] + [C["EulerNumber"]]
EXACT_UNIT = EXACT + [C["Volume"], C["BoundingBoxVolume"]]  # integers at unit spacing


def _run(engine, vols, counts=None, spacing=(1.0, 1.0, 1.0)):
    """vols: list of [Z,Y,X] label arrays of one shape -> (float64 [sum counts, 19] from the GPU, counts)."""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    counts = [int(v.max()) for v in stack] if counts is None else [int(c) for c in counts]
    got = engine.sizeshape3d(torch.from_numpy(stack).cuda(), counts, spacing=spacing)
    assert got.dtype == torch.float64 and tuple(got.shape) == (sum(counts), len(ref.NAMES))
    return got.cpu().numpy(), counts


def _want(vols, counts, spacing=(1.0, 1.0, 1.0)):
    rows = [ref.sizeshape3d(v, n=c, spacing=spacing) for v, c in zip(vols, counts)]
    return np.concatenate(rows) if rows else np.zeros((0, len(ref.NAMES)))


def _check(got, want, unit_spacing=True, tag=""):
    assert got.shape == want.shape, tag
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    exact = EXACT_UNIT if unit_spacing else EXACT
    assert np.array_equal(got[:, exact], want[:, exact], equal_nan=True), (tag, "integer-valued columns")
    major = np.nan_to_num(want[:, C["MajorAxisLength"]])
    trace = np.nan_to_num(want[:, C["InertiaTensorEigenvalues_0"]:].sum(axis=1)) / 2.0
    worst = 0.0
    for k, name in enumerate(ref.NAMES):
        floor = np.zeros(len(want))
        if name == "MinorAxisLength":
            floor = np.sqrt(64.0 * EPS) * major
        elif name.startswith("InertiaTensorEigenvalues"):
            floor = 64.0 * EPS * trace
        g, w = got[:, k], want[:, k]
        ok = np.isnan(w) | (np.abs(g - w) <= RTOL * np.abs(w) + floor)
        assert ok.all(), (tag, name, g[~ok][:4], w[~ok][:4])
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(g - w) / np.abs(w)
        rel = rel[np.isfinite(rel) & (np.abs(w) > floor * 1e4)]
        worst = max(worst, float(rel.max()) if rel.size else 0.0)
    print(f"sizeshape3d {tag}: {len(want)} objects, worst relative error of a float column {worst:.2e}")
    return worst


def _touches_every_face(vol):
    return all((f > 0).any() for f in (vol[0], vol[-1], vol[:, 0], vol[:, -1], vol[:, :, 0], vol[:, :, -1]))


def _has_touching_objects(vol):
    a, b = vol[:, :, :-1], vol[:, :, 1:]
    return bool(((a != b) & (a > 0) & (b > 0)).any())


# ------------------------------------------------------------------------------------------------ 1. random irregular labels
@pytest.mark.parametrize("seed,shape", [(0, (5, 64, 64)), (1, (32, 48, 56)), (2, (7, 61, 83)), (3, (9, 17, 130)), (4, (8, 8, 64)),
                                        (5, (16, 16, 128)), (6, (9, 9, 65))])
def test_random_labels_equal_the_restatement(engine, seed, shape):
    """Objects touch each other and every face of the volume; shapes below, at, one voxel past and above the 8 x 8 x 64 tile of the kernel."""
    vol, n = ref.random_labels(seed, shape)
    assert n >= 3 and _touches_every_face(vol) and _has_touching_objects(vol)
    got, counts = _run(engine, [vol])
    assert counts == [n]
    _check(got, _want([vol], counts), tag=f"random {shape}")


def test_a_batch_with_a_split_label_an_empty_stack_and_an_absent_label(engine):
    shape = (7, 61, 83)
    a, na = ref.random_labels(11, shape)
    b, nb = ref.random_labels(12, shape, n_seeds=9)
    # one label in two pieces: give the object farthest from object 1 the label 1
    centres = np.asarray([np.argwhere(a == k).mean(axis=0) for k in range(1, na + 1)])
    far = int(np.argmax(((centres - centres[0]) ** 2).sum(axis=1))) + 1
    from scipy import ndimage as ndi

    split = a.copy()
    split[a == far] = 1
    split[a == na] = far if far != na else 1  # keep the labels sequential
    n_split = na - 1
    assert ndi.label(split == 1, structure=np.ones((3, 3, 3)))[1] >= 2
    empty = np.zeros(shape, np.uint16)
    vols = [split, empty, b]
    counts = [n_split, 0, nb + 2]  # the last stack announces two labels that have no voxels
    got, _ = _run(engine, vols, counts)
    want = _want(vols, counts)
    _check(got, want, tag="batch of three")
    absent = got[-2:]
    assert (absent[:, 0] == 0.0).all() and np.isnan(absent[:, 1:]).all()  # as intensity3d: Volume 0, NaN elsewhere
    # F = 1 with zero objects: an empty block
    got0, _ = _run(engine, [empty], [0])
    assert got0.shape == (0, len(ref.NAMES))


def test_objects_far_from_the_origin_of_a_larger_stack(engine):
    """Many tiles per stack, and coordinates around (30, 280, 280): the central moments are formed in exact integers before the
    one division, so the distance from the origin costs nothing."""
    vol, n = ref.random_labels(4, (12, 40, 44), n_seeds=8)
    big = np.zeros((40, 300, 300), np.uint16)
    big[28:, 260:, 256:] = vol
    got, counts = _run(engine, [big])
    want_small = ref.sizeshape3d(vol)
    want = ref.sizeshape3d(big, n=n)
    _check(got, want, tag="far corner")
    # and they are the small volume's values, shifted
    shift_free = [C[k] for k in ("Volume", "BoundingBoxVolume", "Extent", "EulerNumber")]  # integers and one IEEE division of integers
    assert np.array_equal(got[:, shift_free], want_small[:, shift_free])
    assert np.allclose(got[:, C["EquivalentDiameter"]], want_small[:, C["EquivalentDiameter"]], rtol=RTOL, atol=0)
    assert np.allclose(got[:, C["MajorAxisLength"]], want_small[:, C["MajorAxisLength"]], rtol=RTOL, atol=0)


# ------------------------------------------------------------------------------------------------ 2. topology
@pytest.mark.parametrize("name,mask,euler", ref.topology_cases(), ids=[c[0] for c in ref.topology_cases()])
def test_euler_number_of_known_topologies(engine, name, mask, euler):
    vol = mask.astype(np.uint16)
    # a second stack holds the same object one voxel nearer the low faces, under label 2 beside a one-voxel label 1
    moved = np.zeros(vol.shape, np.uint16)
    if mask[0].any() or mask[:, 0].any() or mask[:, :, 0].any():
        moved = vol * 2
    else:
        moved[:-1, :-1, :-1] = vol[1:, 1:, 1:] * 2
    free = np.argwhere(moved == 0)[0]
    moved[tuple(free)] = 1
    got, counts = _run(engine, [vol, moved])
    assert counts == [1, 2]
    assert got[0, C["EulerNumber"]] == euler and got[2, C["EulerNumber"]] == euler
    _check(got, _want([vol, moved], counts), tag=name)


def test_euler_number_of_shells_that_touch_each_other(engine):
    """Hollow boxes face to face under different labels: everything is per label, so a neighbour's voxels in the window change
    nothing.  (pieces + cavities, known by construction: tests/test_cpu_sizeshape3d_ref.py)"""
    vol = np.zeros((11, 14, 70), np.uint16)
    want_euler = []
    for k in range(5):
        x = 14 * k
        vol[:, :, x:x + 14] = k + 1
        for c in range(k % 3):  # 0, 1 or 2 closed cavities
            vol[2:9, 2 + 6 * c:6 + 6 * c, x + 2:x + 12] = 0
        want_euler.append(1 + k % 3)
    got, counts = _run(engine, [vol])
    assert list(got[:, C["EulerNumber"]]) == want_euler
    _check(got, _want([vol], counts), tag="shells")


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_batch_and_run_independence_bitwise(engine):
    shape = (9, 50, 70)
    a, _ = ref.random_labels(21, shape)
    b, _ = ref.random_labels(22, shape, n_seeds=20)
    both, counts = _run(engine, [a, b])
    one_a, _ = _run(engine, [a])
    one_b, _ = _run(engine, [b])
    assert np.array_equal(both.view(np.uint64), np.concatenate([one_a, one_b]).view(np.uint64))
    again, _ = _run(engine, [a, b])
    assert np.array_equal(again.view(np.uint64), both.view(np.uint64))
    swapped, _ = _run(engine, [b, a])
    assert np.array_equal(swapped.view(np.uint64), np.concatenate([one_b, one_a]).view(np.uint64))


# ------------------------------------------------------------------------------------------------ 4. spacing
def test_spacing_scales_the_physical_columns_only(engine):
    vol, n = ref.random_labels(31, (10, 44, 52))
    unit, counts = _run(engine, [vol])
    got, _ = _run(engine, [vol], spacing=(3.0, 1.0, 1.0))
    _check(got, _want([vol], counts, spacing=(3.0, 1.0, 1.0)), unit_spacing=False, tag="spacing (3,1,1)")
    assert np.array_equal(got[:, ref.INDEX_COLUMNS].view(np.uint64), unit[:, ref.INDEX_COLUMNS].view(np.uint64))
    assert np.array_equal(got[:, C["Volume"]], 3.0 * unit[:, C["Volume"]])
    got2, _ = _run(engine, [vol], spacing=(0.5, 0.2, 0.25))
    _check(got2, _want([vol], counts, spacing=(0.5, 0.2, 0.25)), unit_spacing=False, tag="spacing (0.5,0.2,0.25)")
    import torch

    for bad in [(0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (1.0, 1.0, float("inf"))]:
        with pytest.raises(ValueError):
            engine.sizeshape3d(torch.from_numpy(vol[None]).cuda(), counts, spacing=bad)


# ------------------------------------------------------------------------------------------------ 5. next to intensity3d
def test_counts_and_centres_equal_intensity3d_bit_for_bit(engine):
    import torch

    from aliby_amd.extraction.features import intensity3d_names, sizeshape3d_names

    shape = (7, 61, 83)
    a, na = ref.random_labels(41, shape)
    b, nb = ref.random_labels(42, shape, n_seeds=7)
    stack = torch.from_numpy(np.stack([a, b])).cuda()
    rng = np.random.default_rng(0)
    px = torch.from_numpy(rng.integers(0, 60000, size=(2, 1, *shape)).astype(np.uint16)).cuda()
    counts = [na, nb + 1]  # one absent label
    inten = engine.intensity3d(stack, px, 0, counts).cpu().numpy()
    shp = engine.sizeshape3d(stack, counts).cpu().numpy()
    i_names, s_names = intensity3d_names(), sizeshape3d_names()
    assert np.array_equal(shp[:, s_names.index("Volume")], inten[:, i_names.index("Volume")])
    for k in "XYZ":
        got, want = shp[:, s_names.index(f"Center_{k}")], inten[:, i_names.index(f"Location_Center_{k}")]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), k
    assert np.isnan(shp[-1, 1:]).all() and np.isnan(inten[-1, 1:]).all() and shp[-1, 0] == inten[-1, 0] == 0.0


def test_the_c_entry_refuses_what_it_cannot_hold(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    lab = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    lab[0, :, 2:5, 2:5] = 1
    off = np.asarray([0, 1], np.int32)
    sp = np.ones(3)
    out = torch.zeros((1, 19), dtype=torch.float64, device="cuda")
    fn = engine.lib.aliby_features_sizeshape3d
    with pytest.raises(Exception):  # an output row shorter than the 19 columns
        _lib.check(fn(engine.ctx.handle, _ptr(lab), 1, 2, 8, 8, _ptr(off), _ptr(sp), _ptr(out), 18, 0, _stream_ptr()))
    with pytest.raises(Exception):  # spacing must be positive
        _lib.check(fn(engine.ctx.handle, _ptr(lab), 1, 2, 8, 8, _ptr(off), _ptr(np.asarray([1.0, 0.0, 1.0])), _ptr(out), 19, 0, _stream_ptr()))
    assert float(out.abs().sum()) == 0.0  # refused before anything was written
    _lib.check(fn(engine.ctx.handle, _ptr(lab), 1, 2, 8, 8, _ptr(off), _ptr(sp), _ptr(out), 19, 0, _stream_ptr()))
    row = out.cpu().numpy()[0]
    assert row[C["Volume"]] == 18 and row[C["EulerNumber"]] == 1 and row[C["Extent"]] == 1.0
    # offsets that do not grow would put rows past the accumulators.  All-background labels: no kernel writes whatever the entry does
    bg = torch.zeros((2, 2, 8, 8), dtype=torch.uint16, device="cuda")
    out2 = torch.zeros((3, 19), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        _lib.check(fn(engine.ctx.handle, _ptr(bg), 2, 2, 8, 8, _ptr(np.asarray([0, 3, 2], np.int32)), _ptr(sp), _ptr(out2), 19, 0, _stream_ptr()))
    torch.cuda.synchronize()
    assert float(out2.abs().sum()) == 0.0
    with pytest.raises(ValueError):
        engine.sizeshape3d(bg, [2, -1])


def test_python_refuses_bad_labels_before_any_launch(engine):
    """The label checks of the other volume families (tests/test_gpu_intensity3d.py), with their exception types."""
    import torch

    vol = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    vol[0, :, 2:5, 2:5] = 1
    ok = engine.sizeshape3d(vol, [1])
    assert tuple(ok.shape) == (1, 19) and float(ok[0, C["Volume"]]) == 18.0
    for surface_area in (False, True):
        with pytest.raises(ValueError):
            engine.sizeshape3d(vol.cpu(), [1], surface_area=surface_area)  # labels on the host
        with pytest.raises(TypeError):
            engine.sizeshape3d(vol.cpu().numpy(), [1], surface_area=surface_area)
        with pytest.raises(TypeError):
            engine.sizeshape3d(vol.to(torch.int32), [1], surface_area=surface_area)
        with pytest.raises(ValueError):
            engine.sizeshape3d(vol[0], [1], surface_area=surface_area)  # labels of rank 3


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_labels_of_eval_do_3d_go_straight_into_sizeshape3d(engine):
    """Volume labels from `CellposeModel.eval(..., do_3D=True)` (flows from synth.analytic_flows_3d, as tests/test_gpu_cellpose3d.py
    builds them) stay on the device, go into sizeshape3d and intensity3d, and match the restatement on the downloaded labels."""
    import torch

    from aliby_amd.segment.cellpose_hip import CellposeModel

    f = synth.make_fov(5, 3, shape=(128, 128), n_channels=2, n_z=16, n_target=12)
    gt = synth.ellipsoid_planes(f["nuclei"], 16, seed=3)
    dP, prob = synth.analytic_flows_3d(gt)

    def override(x):
        assert tuple(x.shape[1:]) == gt.shape
        return torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()

    model = CellposeModel(flows_override=override)
    masks, _, _ = model.eval(np.zeros(gt.shape, np.uint16), do_3D=True)
    counts = [int(c) for c in model.last_counts]
    assert masks.dtype == torch.uint16 and masks.is_cuda and counts[0] > 0
    got = engine.sizeshape3d(masks[None], counts, spacing=(2.0, 0.5, 0.5)).cpu().numpy()
    labels = masks.cpu().numpy()
    assert int(labels.max()) == counts[0]
    want = ref.sizeshape3d(labels, n=counts[0], spacing=(2.0, 0.5, 0.5))
    _check(got, want, unit_spacing=False, tag="eval do_3D")
