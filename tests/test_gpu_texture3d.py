"""
GPU parity of `FeatureEngine.texture3d` (aliby_amd/csrc/feat_texture3d.hip): the 13 Haralick statistics in 13 directions inside the
objects of volume labels [F,Z,Y,X].  Compared with the NumPy reference tests/texture3d_ref.py (crop and matrices restated, the
statistics the oracle's own; pinned by tests/test_cpu_texture3d_ref.py).  Parity with cp_measure / mahotas stays unpinned, the
order of the directions included.

Rule (README "Parity", tests/test_gpu_features.py::_compare): float columns within rtol = 1e-4, atol = 1e-9, NaN where the
reference has NaN.  Reproducibility is asserted bit for bit.  Every test prints the worst relative error it saw; on an
MI355X the largest over the file was 7.7e-11 (42 comparisons, most of them below 1e-11).
"""
from functools import partial

import numpy as np
import pytest

from tests import coloc3d_ref as c3
from tests import texture3d_ref as ref
from tests.volume_checks import bits as _bits, check, pixel_mode as _mode, quiet_numpy  # noqa: F401 (quiet_numpy: an autouse fixture)

pytestmark = pytest.mark.gpu

_check = partial(check, "texture3d")


def _run(engine, vols, pixels, channel=0, counts=None, **kw):
    """vols [F][Z,Y,X], pixels [F,C,Z,Y,X] (uint16 or float32) -> (device result, counts)."""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    counts = [int(v.max()) for v in stack] if counts is None else [int(c) for c in counts]
    got = engine.texture3d(torch.from_numpy(stack).cuda(), torch.from_numpy(np.ascontiguousarray(pixels)).cuda(), channel, counts, **kw)
    assert got.dtype == torch.float64 and tuple(got.shape) == (sum(counts), 169)
    return got, counts


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("mode", ["u16", "f32_unit"])
@pytest.mark.parametrize("scale,gl", [(3, 256), (1, 256), (3, 64), (1, 64)])
@pytest.mark.parametrize("maker", ["ellipsoids", "irregular"])
def test_default_inputs_equal_the_reference(engine, maker, scale, gl, mode):
    vol, n, px = getattr(c3, maker)()
    px = _mode(px, mode)
    assert n >= 8 and px.shape[0] == 3
    channel = 1 if maker == "irregular" else 0
    got, counts = _run(engine, [vol], px[None], channel, scale=scale, gray_levels=gl)
    want = ref.texture3d_batch([vol], px[None], channel, counts, scale, gl)
    if scale == 3:
        assert np.isfinite(want).all()  # 169 numbers per object: every direction of every object has pairs
    _check(got, want, f"{maker} {mode} scale {scale} levels {gl}")


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_seeded_random_volumes_equal_the_reference(engine, seed):
    vol, n, px, scale = ref.random_case(seed)
    assert n >= 2 and 1 <= scale <= 4
    for mode in ("u16", "f32_unit"):
        p = _mode(px, mode)
        got, counts = _run(engine, [vol], p[None], 0, scale=scale)
        _check(got, ref.texture3d_batch([vol], p[None], 0, counts, scale), f"random {seed} {mode} scale {scale}")


# ------------------------------------------------------------------------------------------------ 2. grey-level edges
@pytest.mark.parametrize("mode", ["u16", "f32_unit"])
def test_all_grey_levels_one_grey_level_none_one_voxel_and_a_plate(engine, mode):
    vol, n, px = ref.grey_edge_volume()
    p = _mode(px, mode)
    grey = ref.grey_levels(p[0])
    assert len(np.unique(grey[vol == 1])) == 255 and grey[vol == 1].min() == 1
    assert len(np.unique(grey[vol == 2])) == 1 and grey[vol == 2].max() > 0
    assert grey[vol == 3].max() == 0 and int((vol == 4).sum()) == 1
    got, counts = _run(engine, [vol], p[None])
    want = ref.texture3d_batch([vol], p[None], 0, counts)
    _check(got, want, f"grey edges {mode}")
    g = got.cpu().numpy().reshape(n, 13, 13)
    assert np.isfinite(g[0]).all()
    assert np.isfinite(g[1]).all() and (g[1][:, 2] == 1.0).all() and (g[1][:, [7, 8, 10]] == 0.0).all()  # Correlation's sx == 0 branch, entropies 0
    assert np.isnan(g[2]).all() and np.isnan(g[3]).all()
    in_plane = [k for k, d in enumerate(ref.DELTAS_3D) if d[0] == 0]
    assert np.isfinite(g[4][in_plane]).all() and np.isnan(np.delete(g[4], in_plane, axis=0)).all()  # 2 voxels thick, scale 3
    got64, _ = _run(engine, [vol], p[None], gray_levels=64)
    _check(got64, ref.texture3d_batch([vol], p[None], 0, counts, 3, 64), f"grey edges {mode}, 64 levels")


# ------------------------------------------------------------------------------------------------ 3. both sides of the LDS budget
@pytest.mark.parametrize("mode,scale", [("u16", 3), ("f32_unit", 1)])
def test_boxes_on_both_sides_of_the_lds_budget_and_at_it(engine, mode, scale):
    budget = engine.texture3d_lds_voxels
    vol, n, px, boxes = ref.budget_volume(budget)
    assert boxes[0] == budget and budget < boxes[1] < budget + budget // 16 and budget - budget // 16 < boxes[2] < budget and boxes[3] > 2 * budget
    p = _mode(px, mode)
    got, counts = _run(engine, [vol], p[None], scale=scale)
    want = ref.texture3d_batch([vol], p[None], 0, counts, scale)
    _check(got, want, f"budget {mode} scale {scale}")
    plate = got.cpu().numpy()[4].reshape(13, 13)
    if scale == 3:
        assert np.isnan(plate).all()
    else:
        assert int(np.isfinite(plate).all(axis=1).sum()) == 4 and int(np.isnan(plate).all(axis=1).sum()) == 9


def test_the_same_object_in_both_forms_gives_the_same_bits(engine):
    import torch

    budget = engine.texture3d_lds_voxels
    vols, px = ref.stretched_box(budget)
    z, y, x = np.nonzero(vols[0])
    assert (np.ptp(z) + 1) * (np.ptp(y) + 1) * (np.ptp(x) + 1) < budget < np.prod(vols[1].shape) - 3 * vols[1].shape[1] * vols[1].shape[2]
    for mode in ("u16", "f32_unit"):
        p = _mode(px, mode)
        got, counts = _run(engine, vols, p)
        assert counts == [1, 1] and torch.isfinite(got).all()
        assert torch.equal(_bits(got[0]), _bits(got[1]))
        _check(got, ref.texture3d_batch(vols, p, 0, counts), f"stretched box {mode}")


# ------------------------------------------------------------------------------------------------ 4. a batch
def test_a_batch_with_a_split_label_an_empty_stack_and_absent_labels(engine):
    from scipy import ndimage as ndi

    vols, counts, px = c3.split_batch()
    assert ndi.label(vols[0] == 1, structure=np.ones((3, 3, 3)))[1] >= 2 and not vols[1].any() and counts[2] == int(vols[2].max()) + 2
    for mode, channel in (("u16", 0), ("f32_unit", 1)):
        p = _mode(px, mode)
        got, _ = _run(engine, vols, p, channel, counts)
        _check(got, ref.texture3d_batch(vols, p, channel, counts), f"batch of three {mode}")
        assert np.isnan(got.cpu().numpy()[-2:]).all()  # the announced labels without voxels: a row of NaN
    got0, _ = _run(engine, [vols[1]], px[1:2], 0, [0])
    assert tuple(got0.shape) == (0, 169)


# ------------------------------------------------------------------------------------------------ 5. one plane
def test_one_plane_equals_the_2d_family(engine):
    import torch

    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    vol, n, px = c3.irregular(31, (1, 64, 72), n_seeds=8)
    for mode in ("u16", "f32_unit"):
        p = _mode(px, mode)
        got, counts = _run(engine, [vol], p[None], 1)
        _check(got, ref.texture3d_batch([vol], p[None], 1, counts), f"one plane {mode}")
        dl = to_device_u16(vol)  # [1,Y,X]
        dp, dt = to_device_planes(p[None, :, 0])  # [1,C,Y,X]
        tab = engine.object_table(dl)
        out = engine.new_output(tab.n_obj, 52)
        engine.texture(dl, dp, dt, 1, tab, out, 0)
        torch.cuda.synchronize()
        two = out.cpu().numpy()
        g = got.cpu().numpy()
        want = np.full_like(g, np.nan)
        for d3, d2 in ref.IN_PLANE.items():
            want[:, d3 * 13:(d3 + 1) * 13] = two[:, d2 * 13:(d2 + 1) * 13]
        assert np.isfinite(two).sum() > two.size // 2
        _check(g, want, f"one plane {mode} against the 2-D family")


# ------------------------------------------------------------------------------------------------ 6. reproducibility
def test_rows_are_bitwise_independent_of_run_batch_and_neighbours(engine):
    """The same stack alone, beside a stack holding an object whose box is far above the LDS budget, in the other order, twice."""
    import torch

    shape = (9, 50, 70)
    vol, n, px = c3.irregular(21, shape)
    px = c3.unit_float(px)
    big = np.zeros(shape, np.uint16)
    big[:, 1:49, 1:69] = 1
    assert int((big == 1).sum()) > engine.texture3d_lds_voxels
    big_px = c3.unit_float(c3.noise_pixels(22, shape))
    alone, _ = _run(engine, [vol], px[None], 2)
    again, _ = _run(engine, [vol], px[None], 2)
    assert torch.equal(_bits(alone), _bits(again))
    both, _ = _run(engine, [vol, big], np.stack([px, big_px]), 2)
    assert torch.equal(_bits(both[:n]), _bits(alone))
    swapped, _ = _run(engine, [big, vol], np.stack([big_px, px]), 2)
    assert torch.equal(_bits(swapped[1:]), _bits(alone))
    assert torch.equal(_bits(swapped[:1]), _bits(both[n:]))
    _check(alone, ref.texture3d_batch([vol], px[None], 2, [n]), "reproducibility")
    _check(both[n:], ref.texture3d_batch([big], big_px[None], 2, [1]), "reproducibility, the large box")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_python_refuses_bad_arguments_before_any_launch(engine, monkeypatch):
    import torch

    vol = torch.zeros((1, 2, 8, 8), dtype=torch.uint16, device="cuda")
    vol[0, :, 2:6, 2:6] = 1
    px = torch.full((1, 2, 2, 8, 8), 5000, dtype=torch.uint16, device="cuda")
    ok = engine.texture3d(vol, px, 0, [1], scale=1)
    assert tuple(ok.shape) == (1, 169) and bool(torch.isfinite(ok).all())
    launched = []
    monkeypatch.setattr(engine.lib, "aliby_features_texture3d", lambda *a: launched.append(a) or 0)  # the C entry, were it reached
    for kw in (dict(channel=2), dict(channel=-1), dict(scale=0), dict(gray_levels=1), dict(gray_levels=257), dict(counts=[1, 1]), dict(counts=[-1]),
               dict(pixels=px[:, :, :1]), dict(volume=vol[0]), dict(volume=vol.cpu())):
        args = dict(volume=vol, pixels=px, channel=0, counts=[1])
        args.update(kw)
        with pytest.raises(ValueError):
            engine.texture3d(**args)
    for kw in (dict(pixels=px.to(torch.float64)), dict(volume=vol.to(torch.int32)), dict(volume=vol.cpu().numpy()), dict(scale=1.5), dict(channel="0")):
        args = dict(volume=vol, pixels=px, channel=0, counts=[1])
        args.update(kw)
        with pytest.raises(TypeError):
            engine.texture3d(**args)
    assert not launched


def test_the_c_entry_refuses_before_anything_is_written(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    vol, _, pix = c3.c_entry_case()
    lab = torch.from_numpy(vol[None]).cuda()
    px = torch.from_numpy(pix[None]).cuda()
    off = np.asarray([0, 1], np.int32)
    out = torch.zeros((1, 169), dtype=torch.float64, device="cuda")
    fn = engine.lib.aliby_features_texture3d
    h = engine.ctx.handle

    def call(labels=lab, pixels=px, dtype=_lib.F32, shape=(1, 2, 2, 8, 8), channel=0, scale=1, gl=256, o=out, ld=169, col0=0):
        F, C, Z, Y, X = shape
        return fn(h, _ptr(labels), _ptr(pixels), dtype, F, C, Z, Y, X, channel, _ptr(off), scale, gl, _ptr(o) if o is not None else 0, ld, col0, _stream_ptr())

    for bad in (dict(shape=(1, 2, 0, 8, 8)), dict(channel=2), dict(o=None), dict(dtype=99), dict(ld=168), dict(col0=1), dict(scale=0), dict(gl=1), dict(gl=257)):
        with pytest.raises(Exception):
            _lib.check(call(**bad))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # refused before anything was written
    _lib.check(call())
    _check(out, ref.texture3d(vol, pix[0], 1, 1), "through the C entry")
