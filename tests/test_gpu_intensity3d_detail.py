"""
GPU parity of `FeatureEngine.intensity3d_detail` (aliby_amd/csrc/feat_intensity3d_detail.hip): the edge statistics, MassDisplacement,
quartiles, median, MAD and maximum position of the objects of volume labels [F,Z,Y,X].  Compared with tests/intensity3d_detail_ref.py
(exact integer sums, float64 order statistics; pinned to the oracle and to hand values by tests/test_cpu_intensity3d_detail_ref.py)
under that file's rule (`check`): the order statistics, the edge minimum and maximum and the maximum's position bit for bit; with
uint16 pixels the edge sum and mean bit for bit, the edge std within 1e-10 relative and MassDisplacement within 1e-10 voxels; with
float32 pixels the edge sum, mean and std within 1e-9 relative and MassDisplacement within 1e-9 voxels on non-negative pixels, and the
bit-exact columns alone on signed ones.  Reproducibility is asserted bit for bit.  Parity with cp_measure stays unpinned.
"""
import functools

import numpy as np
import pytest

from tests import coloc3d_ref
from tests import intensity3d_detail_ref as ref
from tests.volume_checks import bits as _bits, quiet_numpy  # noqa: F401 (quiet_numpy: an autouse fixture)

pytestmark = pytest.mark.gpu

C13 = ref.cols(True)
MODES = ["u16", "f32", "f32_signed"]


def _run(engine, vols, pixels, channel=0, counts=None, edge=True):
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] (uint16 or float32) -> (device result, counts)."""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    counts = [int(v.max()) for v in stack] if counts is None else [int(c) for c in counts]
    got = engine.intensity3d_detail(torch.from_numpy(stack).cuda(), torch.from_numpy(np.ascontiguousarray(pixels)).cuda(), channel, counts, edge)
    assert got.dtype == torch.float64 and tuple(got.shape) == (sum(counts), 13 if edge else 8)
    return got, counts


def _one_stack(engine, vol, px, n, mode, tag):
    """One stack, one channel of uint16 pixels taken in `mode`, against the reference."""
    p = ref.as_mode(px, mode)
    got, counts = _run(engine, [vol], p[None, None], counts=[n])
    ref.check(got, ref.detail(vol, p, n), p.dtype, f"{tag} {mode}", signed=mode == "f32_signed")
    return got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ellipsoids():
    vol, n, px = coloc3d_ref.ellipsoids()
    return vol, n, px[0]


@functools.lru_cache(maxsize=None)
def _irregular():
    vol, n, px = coloc3d_ref.irregular()
    return vol, n, px[0]


# ------------------------------------------------------------------------------------------------ 1. hand cases
def _line(values):
    values = np.asarray(values)
    vol = np.zeros((3, 3, len(values) + 2), np.uint16)
    vol[1, 1, 1:1 + len(values)] = 1
    px = np.zeros(vol.shape, values.dtype)
    px[1, 1, 1:1 + len(values)] = values
    return vol, px


def test_the_quartile_rule_branch_by_branch(engine):
    want = {(7,): [7.0, 7.0, 0.0, 7.0], (30, 10): [20.0, 30.0, 20.0, 30.0], (30, 10, 20): [17.5, 25.0, 10.0, 30.0],
            (40, 10, 30, 20): [20.0, 30.0, 10.0, 40.0], (50, 10, 40, 20, 30): [22.5, 35.0, 15.0, 47.5]}
    for values, hand in want.items():
        vol, px = _line(np.asarray(values, np.uint16))
        got = _one_stack(engine, vol, px, 1, "u16", f"n = {len(values)}")
        assert list(got[0, 6:10]) == hand, (values, got[0, 6:10])
        got = _one_stack(engine, vol, px, 1, "f32", f"n = {len(values)}")  # the same branches on float32 pixels
    vol, px = _line(np.asarray([0.1, 0.7, 0.2], np.float32))  # a MAD that does not fit a float32
    got, _ = _run(engine, [vol], px[None, None])
    ref.check(got, ref.detail(vol, px, 1), np.float32, "three floats")


def test_a_cube_a_filled_stack_and_a_repeated_maximum(engine):
    vol = np.zeros((5, 5, 5), np.uint16)
    vol[1:4, 1:4, 1:4] = 1
    px = np.full(vol.shape, 5, np.uint16)
    px[2, 2, 2] = 60000  # the centre, the one voxel of the 27 that is no edge voxel
    got = _one_stack(engine, vol, px, 1, "u16", "cube")
    assert list(got[0, :5]) == [130.0, 5.0, 0.0, 5.0, 5.0] and list(got[0, 10:]) == [2.0, 2.0, 2.0]
    full = np.ones((2, 3, 4), np.uint16)
    pf = np.arange(24, dtype=np.uint16).reshape(full.shape) + 1
    for mode in ("u16", "f32"):
        got = _one_stack(engine, full, pf, 1, mode, "filled stack")
        assert list(got[0, :5]) == [0.0] * 5 and np.isfinite(got[0, 5:]).all() and list(got[0, 10:]) == [3.0, 2.0, 1.0]
    vol = np.zeros((4, 5, 6), np.uint16)
    vol[0:3, 1:4, 1:5] = 1
    px = np.full(vol.shape, 9, np.uint16)
    px[0, 2, 3] = px[2, 1, 2] = px[1, 3, 4] = 500
    for mode in MODES:
        got = _one_stack(engine, vol, px, 1, mode, "repeated maximum")
        assert list(got[0, 10:]) == [2.0, 1.0, 2.0]
    px[:] = 9
    got = _one_stack(engine, vol, px, 1, "u16", "all equal")
    assert list(got[0, 10:]) == [4.0, 3.0, 2.0] and got[0, C13["Intensity_MADIntensity"]] == 0.0 and got[0, C13["Intensity_StdIntensityEdge"]] == 0.0


# ------------------------------------------------------------------------------------------------ 2. shapes and pixel values
@pytest.mark.parametrize("mode", MODES)
def test_ellipsoids_equal_the_reference(engine, mode):
    vol, n, px = _ellipsoids()
    assert n >= 8
    _one_stack(engine, vol, px, n, mode, "ellipsoids")


@pytest.mark.parametrize("mode", MODES)
def test_irregular_touching_labels_equal_the_reference(engine, mode):
    vol, n, px = _irregular()
    a, b = vol[:, :, :-1], vol[:, :, 1:]
    assert n >= 8 and ((a != b) & (a > 0) & (b > 0)).any()  # objects touch
    _one_stack(engine, vol, px, n, mode, "irregular")


@pytest.mark.parametrize("mode", MODES)
def test_heavy_ties_constant_objects_and_the_ends_of_the_range(engine, mode):
    vol, n, _ = _irregular()
    px = ref.tied_pixels(2, vol)
    inside = px[vol > 0]
    assert (inside == 0).any() and (inside == 65535).any() and len(np.unique(px[vol == 6])) == 1 and not px[vol == 3].any()
    got = _one_stack(engine, vol, px, n, mode, "ties")
    if mode != "f32_signed":
        assert np.isnan(got[2, C13["Intensity_MassDisplacement"]])  # label 3 is dark: no centre of mass


# ------------------------------------------------------------------------------------------------ 3. sizes
@pytest.mark.parametrize("mode", ["u16", "f32"])
def test_sizes_on_each_side_of_every_sort_padding(engine, mode):
    vol, n, px = ref.power_of_two_volume()
    _one_stack(engine, vol, px, n, mode, "2^k - 1, 2^k, 2^k + 1")


@pytest.mark.parametrize("mode", ["u16", "f32"])
def test_objects_below_at_and_above_the_lds_budget(engine, mode):
    budget = engine.intensity3d_detail_lds_voxels
    vol, n, px = ref.budget_volume(budget)
    assert list(np.bincount(vol.ravel())[1:4]) == [budget - 1, budget, budget + 1]
    _one_stack(engine, vol, px, n, mode, "budget")


@pytest.mark.parametrize("mode", ["u16", "f32"])
def test_both_forms_give_the_same_bits(engine, mode):
    """One object of exactly the budget (measured from LDS) and the same object with one more voxel of its median value (measured from
    global scratch).  The inputs are built so that the order statistics and the maximum's position are the same numbers on both sides
    (tests/test_cpu_intensity3d_detail_ref.py shows the reference agrees): the kernel's must be the same bits.  Every column of both
    rows is compared with the reference as well."""
    budget = engine.intensity3d_detail_lds_voxels
    vols, px = ref.form_pair(budget)
    assert int((vols[0] == 1).sum()) == budget and int((vols[1] == 1).sum()) == budget + 1
    p = ref.as_mode(px, mode)
    got, _ = _run(engine, vols, p, counts=[1, 1])
    ref.check(got, ref.detail_batch(vols, p, 0, [1, 1]), p.dtype, f"form pair {mode}")
    g = got.cpu().numpy().view(np.uint64)
    same = [C13[k] for k in ref.BITWISE if "Edge" not in k]
    assert np.array_equal(g[0, same], g[1, same]), (g[0, same], g[1, same])
    apart, _ = _run(engine, vols[1:], p[1:], counts=[1])  # the large object without the LDS form's launch beside it
    assert np.array_equal(apart.cpu().numpy().view(np.uint64)[0], g[1])


# ------------------------------------------------------------------------------------------------ 4. the faces of the stack
@pytest.mark.parametrize("mode", MODES)
def test_objects_on_every_face_a_label_above_the_count_and_an_enclosed_hole(engine, mode):
    vol, n, px = ref.faces_volume()
    assert n == 8 and int(vol.max()) == 9 and vol[2, 3, 4] == 0
    got = _one_stack(engine, vol, px, n, mode, "faces")
    assert np.isnan(got[7]).all()  # label 8 has no voxels
    # without the voxel of label 9, (3, 3, 4) of label 7 would still be an edge voxel; inside a solid block it is 9 alone that makes edges
    solid = np.ones((5, 5, 5), np.uint16)
    solid[2, 2, 2] = 9
    got = _one_stack(engine, solid, np.full_like(solid, 20000), 1, mode, "a label above the count inside a block")
    assert round(got[0, 0] / got[0, 1]) == 6  # edge sum / edge mean: the six face neighbours of the foreign voxel


@pytest.mark.parametrize("mode", ["u16", "f32"])
def test_one_plane_equals_the_oracles_2d_values(engine, mode):
    from oracle import cp_measure_restated as cpm

    vol, n, px = coloc3d_ref.irregular(31, (1, 64, 72), n_seeds=8)
    p = ref.as_mode(px[0], mode)
    got = _one_stack(engine, vol, px[0], n, mode, "one plane")
    res = cpm.get_intensity(vol[0], p[0], edge_measurements=True)
    want = np.stack([np.asarray(res[k], float)[:n] for k in ref.names(True)], axis=1)
    for k, j in C13.items():
        if k in ref.BITWISE:
            assert np.array_equal(got[:, j], want[:, j]), (mode, k)
        else:  # the oracle adds in float64 and takes the deviation about a rounded mean
            assert np.allclose(got[:, j], want[:, j], rtol=1e-9, atol=1e-9), (mode, k)


# ------------------------------------------------------------------------------------------------ 5. batches
@pytest.mark.parametrize("mode", ["u16", "f32"])
def test_a_batch_with_a_split_label_an_empty_stack_and_absent_labels(engine, mode):
    from scipy import ndimage as ndi

    vols, counts, px = coloc3d_ref.split_batch()
    assert ndi.label(vols[0] == 1, structure=np.ones((3, 3, 3)))[1] >= 2 and not vols[1].any() and counts[2] == int(vols[2].max()) + 2
    p = ref.as_mode(px, mode)
    for edge in (True, False):
        got, _ = _run(engine, vols, p, 1, counts, edge)
        ref.check(got, ref.detail_batch(vols, p, 1, counts, edge), p.dtype, f"batch of three {mode} edge={edge}", edge=edge)
        assert np.isnan(got.cpu().numpy()[-2:]).all()  # the announced labels without voxels: a row of NaN, the edge columns too
    full, _ = _run(engine, vols, p, 1, counts, True)
    assert np.array_equal(full.cpu().numpy()[:, 5:].view(np.uint64), got.cpu().numpy().view(np.uint64))  # the flag only drops columns
    got0, _ = _run(engine, [vols[1]], p[1:2], 0, [0])  # no objects at all: an empty block
    assert tuple(got0.shape) == (0, 13)


def test_more_rows_than_workgroups(engine):
    """Two stacks of 65 535 one-voxel objects: 131 070 rows, far more than the launch has workgroups, so nearly every compared row comes
    out of the kernel's grid-stride loop.  The expected rows are the closed form of tests/intensity3d_detail_ref.one_voxel_rows, which
    tests/test_cpu_intensity3d_detail_ref.py holds to the general reference (eight seconds per stack of this size)."""
    a, pa = ref.single_voxels(seed=81)
    b, pb = ref.single_voxels(seed=91)
    pa[a == 12345] = 0
    got, counts = _run(engine, [a, b], np.stack([pa, pb])[:, None])
    assert counts == [65535, 65535]
    want = np.concatenate([ref.one_voxel_rows(a, pa), ref.one_voxel_rows(b, pb)])
    ref.check(got, want, np.uint16, "131 070 one-voxel objects")
    g = got.cpu().numpy()
    assert np.array_equal(g[:, 2], want[:, 2]) and np.array_equal(g[:, 5], want[:, 5], equal_nan=True) and np.isnan(g[12344, 5])


# ------------------------------------------------------------------------------------------------ 6. reproducibility
@pytest.mark.parametrize("mode", ["u16", "f32"])
def test_rows_are_bitwise_independent_of_run_batch_and_neighbours(engine, mode):
    import torch

    shape = (9, 50, 70)
    vol, n, px = coloc3d_ref.irregular(21, shape)
    p = ref.as_mode(px[:1], mode)
    big = np.zeros(shape, np.uint16)
    big[:, 2:48, 2:68] = 1
    assert int((big == 1).sum()) > engine.intensity3d_detail_lds_voxels > np.bincount(vol.ravel())[1:].max()
    big_p = ref.as_mode(coloc3d_ref.noise_pixels(22, shape)[:1], mode)
    alone, _ = _run(engine, [vol], p[None])
    again, _ = _run(engine, [vol], p[None])
    assert torch.equal(_bits(alone), _bits(again))
    both, _ = _run(engine, [vol, big], np.stack([p, big_p]))
    assert torch.equal(_bits(both[:n]), _bits(alone))
    swapped, _ = _run(engine, [big, vol], np.stack([big_p, p]))
    assert torch.equal(_bits(swapped[1:]), _bits(alone)) and torch.equal(_bits(swapped[:1]), _bits(both[n:]))
    for lab in (1, n // 2, n):  # the other objects erased wherever they do not touch this one
        kept = ref.keep_touching(vol, lab)
        assert (kept > 0).sum() < (vol > 0).sum() and ((kept > 0) & (kept != lab)).any()
        pruned, _ = _run(engine, [kept], p[None], counts=[n])
        assert torch.equal(_bits(pruned[lab - 1]), _bits(alone[lab - 1])), lab
    ref.check(alone, ref.detail(vol, p[0], n), p.dtype, f"reproducibility {mode}")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_python_refuses_bad_arguments_before_any_launch(engine):
    import torch

    vol = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    vol[0, :, 2:5, 2:5] = 1
    px = torch.ones((1, 2, 2, 8, 8), dtype=torch.uint16, device="cuda")
    ok = engine.intensity3d_detail(vol, px, 1, [1])
    assert tuple(ok.shape) == (1, 13) and tuple(engine.intensity3d_detail(vol, px.float(), 0, [1], False).shape) == (1, 8)
    for channel in (2, -1):
        with pytest.raises(ValueError):
            engine.intensity3d_detail(vol, px, channel, [1])
    for counts in ([1, 1], [-1], [65536]):
        with pytest.raises(ValueError):
            engine.intensity3d_detail(vol, px, 0, counts)
    with pytest.raises(ValueError):
        engine.intensity3d_detail(vol, px[:, :, :1], 0, [1])
    with pytest.raises(ValueError):
        engine.intensity3d_detail(vol[0], px, 0, [1])
    with pytest.raises(ValueError):
        engine.intensity3d_detail(vol.cpu(), px, 0, [1])
    with pytest.raises(ValueError):
        engine.intensity3d_detail(vol, px.cpu(), 0, [1])
    for channel in (0.0, True, "0"):
        with pytest.raises(TypeError):
            engine.intensity3d_detail(vol, px, channel, [1])
    for flag in (1, 0, None, "yes"):
        with pytest.raises(TypeError):
            engine.intensity3d_detail(vol, px, 0, [1], flag)
    with pytest.raises(TypeError):
        engine.intensity3d_detail(vol, px.to(torch.float64), 0, [1])
    with pytest.raises(TypeError):
        engine.intensity3d_detail(vol.to(torch.int32), px, 0, [1])
    with pytest.raises(TypeError):
        engine.intensity3d_detail(vol.cpu().numpy(), px, 0, [1])


def test_the_c_entry_refuses_before_anything_is_written(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    vol, _, pix = coloc3d_ref.c_entry_case()
    lab = torch.from_numpy(vol[None]).cuda()
    px = torch.from_numpy(pix[None]).cuda()
    off = np.asarray([0, 1], np.int32)
    out = torch.zeros((1, 15), dtype=torch.float64, device="cuda")
    fn = engine.lib.aliby_features_intensity3d_detail
    h = engine.ctx.handle

    def call(labels=lab, pixels=px, dtype=_lib.F32, shape=(1, 2, 2, 8, 8), channel=1, offsets=off, edge=1, o=out, ld=15, col0=1):
        F, C, Z, Y, X = shape
        return fn(h, _ptr(labels) if labels is not None else 0, _ptr(pixels) if pixels is not None else 0, dtype, F, C, Z, Y, X, channel,
                  _ptr(offsets), edge, _ptr(o) if o is not None else 0, ld, col0, _stream_ptr())

    for bad in (dict(o=None), dict(labels=None), dict(pixels=None), dict(shape=(1, 2, 0, 8, 8)), dict(channel=2), dict(channel=-1), dict(dtype=99),
                dict(edge=2), dict(ld=13), dict(col0=3), dict(col0=-1), dict(offsets=np.asarray([1, 2], np.int32)),
                dict(offsets=np.asarray([0, 70000], np.int32))):
        with pytest.raises(Exception):
            _lib.check(call(**bad))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # refused before anything was written
    _lib.check(call(edge=0, ld=15, col0=7))  # 8 columns fit where 13 would not
    assert float(out[:, :7].abs().sum()) == 0.0
    ref.check(out[:, 7:], ref.detail(vol, pix[1], 1, edge=False), np.float32, "through the C entry, edge = 0", edge=False)
    out.zero_()
    _lib.check(call())
    ref.check(out[:, 1:14], ref.detail(vol, pix[1], 1), np.float32, "through the C entry")
    assert float(out[0, 0]) == 0.0 and float(out[0, 14]) == 0.0  # nothing beside the 13 columns


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_labels_of_the_flows3d_segmenter_go_straight_into_intensity3d_detail(engine):
    import torch

    from aliby_amd.extraction import features
    from aliby_amd.segment.dispatch import dispatch_segmenter
    from tests import cellpose3d_ref

    f, gt, dP, prob = coloc3d_ref.segmenter_case()
    want_labels, n, _ = cellpose3d_ref.compute_masks_3d(dP, prob)

    def override(x):
        assert tuple(x.shape[1:]) == gt.shape
        return torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()

    segment = dispatch_segmenter(kind="cellpose", channel_to_segment=0, volume_mode="flows3d", setup_params=dict(flows_override=override))
    segment(f["pixels"][None], do_3D=True)
    volume, counts = segment.last_volume
    assert volume.dtype == torch.uint16 and volume.is_cuda and list(counts) == [n] and n > 0
    labels = volume[0].cpu().numpy()
    assert np.array_equal(labels, want_labels)
    for px in (f["pixels"], ref.unit_float(f["pixels"])):
        dev = torch.from_numpy(px[None]).cuda()
        got = engine.intensity3d_detail(volume, dev, 1, counts)
        ref.check(got, ref.detail(labels, px[1], n), px.dtype, f"flows3d segmenter {px.dtype}")
    # the full block of a channel: the moment columns and the detail columns side by side
    block = torch.cat([engine.intensity3d(volume, torch.from_numpy(f["pixels"][None]).cuda(), 1, counts), got], 1)
    assert tuple(block.shape) == (n, len(features.intensity3d_names()) + len(features.intensity3d_detail_names()))
