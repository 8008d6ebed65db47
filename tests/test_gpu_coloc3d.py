"""
GPU parity of `FeatureEngine.coloc3d` (aliby_amd/csrc/feat_coloc3d.hip): the colocalisation metrics of channel pairs inside the
objects of volume labels [F,Z,Y,X].  Compared with the float64 reference tests/coloc3d_ref.py (the oracle's
MeasureColocalization restatement driven with one mask per object; pinned by tests/test_cpu_coloc3d_ref.py, which also shows that
no Costes probe of any input used here is within 1e-8 of a sign change).  Parity with cp_measure stays unpinned.

Rule (README "Parity", tests/test_gpu_features.py::_compare): float columns within rtol = 1e-4, atol = 1e-9, NaN where the
reference has NaN.  Reproducibility is asserted bit for bit.
"""
from functools import partial

import numpy as np
import pytest

from tests import coloc3d_ref as ref
from tests.volume_checks import bits as _bits, check, pixel_mode as _mode, quiet_numpy  # noqa: F401 (quiet_numpy: an autouse fixture)

pytestmark = pytest.mark.gpu

ALL3 = [(0, 1), (0, 2), (1, 2)]
_check = partial(check, "coloc3d")


def _run(engine, vols, pixels, pairs, counts=None, **kw):
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] (uint16 or float32) -> (device result, counts)."""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    counts = [int(v.max()) for v in stack] if counts is None else [int(c) for c in counts]
    got = engine.coloc3d(torch.from_numpy(stack).cuda(), torch.from_numpy(np.ascontiguousarray(pixels)).cuda(), pairs, counts, **kw)
    n_metrics = len(kw.get("metrics", ref.METRICS))
    assert got.dtype == torch.float64 and tuple(got.shape) == (sum(counts), 2 * n_metrics * len(pairs))
    return got, counts


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("mode", ["u16", "f32_unit"])
def test_ellipsoids_all_pairs_equal_the_reference(engine, mode):
    vol, n, px = ref.ellipsoids()
    px = _mode(px, mode)
    assert n >= 8 and px.shape[0] == 3
    got, counts = _run(engine, [vol], px[None], ALL3)
    assert counts == [n]
    _check(got, ref.coloc3d_batch([vol], px[None], ALL3, counts), f"ellipsoids {mode}")


@pytest.mark.parametrize("mode", ["u16", "f32_unit"])
def test_irregular_touching_labels_equal_the_reference(engine, mode):
    vol, n, px = ref.irregular()
    px = _mode(px, mode)
    a, b = vol[:, :, :-1], vol[:, :, 1:]
    assert n >= 8 and ((a != b) & (a > 0) & (b > 0)).any()  # objects touch
    got, counts = _run(engine, [vol], px[None], ALL3)
    _check(got, ref.coloc3d_batch([vol], px[None], ALL3, counts), f"irregular {mode}")


# ------------------------------------------------------------------------------------------------ 2. a batch
def test_a_batch_with_a_split_label_an_empty_stack_and_absent_labels(engine):
    from scipy import ndimage as ndi

    vols, counts, px = ref.split_batch()
    assert ndi.label(vols[0] == 1, structure=np.ones((3, 3, 3)))[1] >= 2 and not vols[1].any() and counts[2] == int(vols[2].max()) + 2
    px = ref.unit_float(px)
    got, _ = _run(engine, vols, px, [(0, 1)], counts)
    want = ref.coloc3d_batch(vols, px, [(0, 1)], counts)
    _check(got, want, "batch of three")
    assert np.isnan(got.cpu().numpy()[-2:]).all()  # the announced labels without voxels: a row of NaN
    # no objects at all: an empty block
    got0, _ = _run(engine, [vols[1]], px[1:2], [(0, 1)], [0])
    assert tuple(got0.shape) == (0, 8)


# ------------------------------------------------------------------------------------------------ 3. both sides of the LDS budget
@pytest.mark.parametrize("mode", ["u16", "f32_unit"])
def test_objects_on_both_sides_of_the_lds_budget(engine, mode):
    budget = engine.coloc3d_lds_voxels
    vol, n, px, voxels = ref.budget_volume(budget)
    assert (voxels == budget).any() and (voxels == budget + 1).any() and (voxels < budget).sum() >= 2 and (voxels > 2 * budget).any()
    px = _mode(px, mode)
    got, counts = _run(engine, [vol], px[None], [(0, 1)])
    _check(got, ref.coloc3d_batch([vol], px[None], [(0, 1)], counts), f"budget {mode}")


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_rows_are_bitwise_independent_of_run_batch_and_neighbours(engine):
    """The same stack alone, beside a stack holding an object far above the LDS budget (which in the 2-D family would change the
    workgroup size of the launch), in the other order, and twice."""
    import torch

    shape = (9, 50, 70)
    vol, n, px = ref.irregular(21, shape)
    px = ref.unit_float(px)
    big = np.zeros(shape, np.uint16)
    big[:, 2:48, 2:68] = 1
    assert int((big == 1).sum()) > 3 * engine.coloc3d_lds_voxels and np.bincount(vol.ravel())[1:].max() < engine.coloc3d_lds_voxels
    big_px = ref.unit_float(ref.noise_pixels(22, shape))
    pairs = [(0, 1), (2, 1)]
    alone, _ = _run(engine, [vol], px[None], pairs)
    again, _ = _run(engine, [vol], px[None], pairs)
    assert torch.equal(_bits(alone), _bits(again))
    both, _ = _run(engine, [vol, big], np.stack([px, big_px]), pairs)
    assert torch.equal(_bits(both[:n]), _bits(alone))
    swapped, _ = _run(engine, [big, vol], np.stack([big_px, px]), pairs)
    assert torch.equal(_bits(swapped[1:]), _bits(alone))
    assert torch.equal(_bits(swapped[:1]), _bits(both[n:]))
    # a pair measured on its own equals the same pair among others
    one, _ = _run(engine, [vol], px[None], [(2, 1)])
    assert torch.equal(_bits(one), _bits(alone[:, 8:]))
    _check(alone, ref.coloc3d_batch([vol], px[None], pairs, [n]), "reproducibility")


# ------------------------------------------------------------------------------------------------ 5. edges
def test_one_voxel_a_constant_channel_and_keywords(engine):
    vol, n, px = ref.edge_volume()
    assert int((vol == 1).sum()) == 1 and len(np.unique(px[0][vol == 2])) == 1
    got, counts = _run(engine, [vol], px[None], [(0, 1)])
    want = ref.coloc3d_batch([vol], px[None], [(0, 1)], counts)
    _check(got, want, "edges u16")
    g = got.cpu().numpy()
    assert np.isnan(g[0, 0]) and np.isnan(g[1, 0]) and np.isnan(want[1, 0])  # Pearson of one voxel / of a constant channel: NaN on both sides
    # keywords other than the defaults, a subset of the metrics in another order, the pair reversed
    pf = ref.unit_float(px)
    kw = dict(metrics=("costes", "manders_fold"), thr=40.0, scale_max=100.0)
    got, _ = _run(engine, [vol], pf[None], [(1, 0)], **kw)
    want = ref.coloc3d_batch([vol], pf[None], [(1, 0)], counts, **kw)
    _check(got, want, "edges unit f32, thr 40, scale_max 100")
    default = ref.coloc3d_batch([vol], pf[None], [(1, 0)], counts, metrics=kw["metrics"])
    assert not np.allclose(want[2], default[2], rtol=1e-3, equal_nan=True)  # the keywords reach the kernel's arithmetic
    only, _ = _run(engine, [vol], pf[None], [(1, 0)], metrics=("rwc",))
    _check(only, ref.coloc3d_batch([vol], pf[None], [(1, 0)], counts, metrics=("rwc",)), "rwc alone")


def test_one_plane_equals_the_2d_family(engine):
    import torch

    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    vol, n, px = ref.irregular(31, (1, 64, 72), n_seeds=8)
    pf = ref.unit_float(px)
    got, counts = _run(engine, [vol], pf[None], [(0, 1)])
    _check(got, ref.coloc3d_batch([vol], pf[None], [(0, 1)], counts), "one plane")
    dl = to_device_u16(vol)  # [1,Y,X]
    dp, dt = to_device_planes(pf[None, :, 0])  # [1,C,Y,X]
    tab = engine.object_table(dl)
    out = engine.new_output(tab.n_obj, 8)
    engine.coloc(dl, dp, dt, 0, 1, tab, out, dict(pearson=0, manders_fold=2, rwc=4, costes=6))
    torch.cuda.synchronize()
    _check(got, out.cpu().numpy(), "one plane against the 2-D family")


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_python_refuses_bad_arguments_before_any_launch(engine):
    import torch

    vol = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    vol[0, :, 2:5, 2:5] = 1
    px = torch.ones((1, 2, 2, 8, 8), dtype=torch.uint16, device="cuda")
    ok = engine.coloc3d(vol, px, [(0, 1)], [1])
    assert tuple(ok.shape) == (1, 8)
    for pairs in ([(0, 0)], [(0, 2)], [(-1, 0)], [], [(0, 1, 1)]):
        with pytest.raises(ValueError):
            engine.coloc3d(vol, px, pairs, [1])
    with pytest.raises(ValueError):
        engine.coloc3d(vol, px, [(0, 1)], [1], metrics=("pearson", "spearman"))
    with pytest.raises(ValueError):
        engine.coloc3d(vol, px, [(0, 1)], [1, 1])
    with pytest.raises(ValueError):
        engine.coloc3d(vol, px[:, :, :1], [(0, 1)], [1])
    with pytest.raises(ValueError):
        engine.coloc3d(vol[0], px, [(0, 1)], [1])
    with pytest.raises(ValueError):
        engine.coloc3d(vol, px, [(0, 1)], [1], scale_max=0.0)
    with pytest.raises(TypeError):
        engine.coloc3d(vol, px.to(torch.float64), [(0, 1)], [1])
    with pytest.raises(TypeError):
        engine.coloc3d(vol.to(torch.int32), px, [(0, 1)], [1])
    with pytest.raises(TypeError):
        engine.coloc3d(vol.cpu().numpy(), px, [(0, 1)], [1])


def test_the_c_entry_refuses_before_anything_is_written(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    vol, _, pix = ref.c_entry_case()
    lab = torch.from_numpy(vol[None]).cuda()
    px = torch.from_numpy(pix[None]).cuda()
    off = np.asarray([0, 1], np.int32)
    pair = np.asarray([[0, 1]], np.int32)
    out = torch.zeros((1, 8), dtype=torch.float64, device="cuda")
    fn = engine.lib.aliby_features_coloc3d
    h = engine.ctx.handle

    def call(labels=lab, pixels=px, dtype=_lib.F32, shape=(1, 2, 2, 8, 8), pairs=pair, n_pairs=1, o=out, ld=8, stride=8, cols=(0, 2, 4, 6)):
        F, C, Z, Y, X = shape
        return fn(h, _ptr(labels), _ptr(pixels), dtype, F, C, Z, Y, X, _ptr(pairs), n_pairs, _ptr(off), _ptr(o) if o is not None else 0, ld, 0,
                  stride, *cols, 15.0, 255.0, _stream_ptr())

    for bad in (dict(shape=(1, 2, 0, 8, 8)), dict(pairs=np.asarray([[0, 2]], np.int32)), dict(pairs=np.asarray([[1, 1]], np.int32)), dict(o=None),
                dict(dtype=99), dict(ld=7), dict(stride=6), dict(n_pairs=0)):
        with pytest.raises(Exception):
            _lib.check(call(**bad))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # refused before anything was written
    _lib.check(call())
    _check(out, ref.coloc3d(vol, pix[0], pix[1], 1), "through the C entry")


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_labels_of_the_flows3d_segmenter_go_straight_into_coloc3d(engine):
    import torch

    from aliby_amd.segment.dispatch import dispatch_segmenter
    from tests import cellpose3d_ref

    f, gt, dP, prob = ref.segmenter_case()
    want_labels, n, _ = cellpose3d_ref.compute_masks_3d(dP, prob)

    def override(x):
        assert tuple(x.shape[1:]) == gt.shape
        return torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()

    segment = dispatch_segmenter(kind="cellpose", channel_to_segment=0, volume_mode="flows3d", setup_params=dict(flows_override=override))
    segment(f["pixels"][None], do_3D=True)
    volume, counts = segment.last_volume
    assert volume.dtype == torch.uint16 and volume.is_cuda and list(counts) == [n] and n > 0
    labels = volume[0].cpu().numpy()
    assert np.array_equal(labels, want_labels)  # the labels tests/test_cpu_coloc3d_ref.py checked the Costes probes of
    for px in (f["pixels"], ref.unit_float(f["pixels"])):
        got = engine.coloc3d(volume, torch.from_numpy(px[None]).cuda(), [(0, 1)], counts)
        _check(got, ref.coloc3d(labels, px[0], px[1], n), f"flows3d segmenter {px.dtype}")
