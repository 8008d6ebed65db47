"""
The grid-stride paths of every volume kernel.  Each launches a capped grid and walks the rest of its work items in a loop:
k_intensity3d and k_volume_table (the front end of coloc3d and texture3d) 32768 x 256 sixteen-voxel segments, k_sizeshape3d 65536
tiles, k_apply_lut (behind stitch_planes) 16384 x 256 voxels.  One thin stack, 130 x 65536 x 1 (tests/volume_scale_ref.py, built
once), exceeds all three; tests/test_cpu_volume_scale.py shows on the CPU, from each kernel's own order of work items, which of its
six small objects lie in the first pass, wholly beyond it (a kernel without the loop reports them absent) and across its boundary.
The same memory read as two stacks of 65 planes makes a strided work item decode a stack index f = 1.

Every family is compared with its own reference under its own rule (tests/test_gpu_intensity3d.py, test_gpu_sizeshape3d.py,
tests/volume_checks.py); the stitched labels must equal oracle/volume_restated.stitch3d voxel for voxel.
"""
import numpy as np
import pytest

from tests import coloc3d_ref, intensity3d_ref, sizeshape3d_ref, texture3d_ref
from tests import volume_scale_ref as vs
from tests.test_gpu_sizeshape3d import _check as check_sizeshape3d
from tests.volume_checks import check, quiet_numpy  # noqa: F401 (quiet_numpy: an autouse fixture)

pytestmark = pytest.mark.gpu

VIEWS = {"one stack": (1, *vs.SHAPE), "two stacks": vs.BATCH_SHAPE}


@pytest.fixture(scope="module")
def scale(engine):
    """The shared stack, on the host and on the device: labels [Z,Y,X], pixels uint16 [2,Z,Y,X] and as unit floats."""
    import torch

    vol, n, px = vs.stack()
    assert all(a > b for a, b in zip(vs.n_items((1, *vs.SHAPE)), (vs.SEGMENT_CAP, vs.TILE_CAP, vs.VOXEL_CAP)))
    pf = coloc3d_ref.unit_float(px)
    return dict(vol=vol, n=n, px=px, pf=pf, d_vol=torch.from_numpy(vol).cuda(), d_px=torch.from_numpy(px).cuda(), d_pf=torch.from_numpy(pf).cuda())


def _view(scale, name, pixels="px"):
    """-> (host vols [F][Z,Y,X], host pixels [F,C,Z,Y,X], device labels [F,Z,Y,X], device pixels [F,C,Z,Y,X], counts)."""
    F, Z, Y, X = VIEWS[name]
    vols = scale["vol"].reshape(F, Z, Y, X)
    # [C, F * Z, Y, X] -> [F, C, Z, Y, X]
    host = np.ascontiguousarray(scale[pixels].reshape(2, F, Z, Y, X).transpose(1, 0, 2, 3, 4))
    dev = scale["d_" + pixels].view(2, F, Z, Y, X).permute(1, 0, 2, 3, 4).contiguous()
    return list(vols), host, scale["d_vol"].view(F, Z, Y, X), dev, [scale["n"]] * F


def _absent(vols, counts):
    return np.concatenate([np.bincount(v.ravel(), minlength=c + 1)[1:c + 1] == 0 for v, c in zip(vols, counts)])


@pytest.mark.parametrize("name", list(VIEWS))
def test_intensity3d_beyond_its_first_pass(engine, scale, name):
    vols, px, d_vol, d_px, counts = _view(scale, name)
    for channel in (0, 1):
        got = engine.intensity3d(d_vol, d_px, channel, counts)
        want, sums = intensity3d_ref.intensity3d_batch(vols, px, channel, counts)
        intensity3d_ref.check(got, want, sums, f"scale, {name}, channel {channel}")
        assert np.array_equal(got.cpu().numpy()[:, 0] == 0, _absent(vols, counts))  # no object reported absent


@pytest.mark.parametrize("name", list(VIEWS))
def test_sizeshape3d_beyond_its_first_pass(engine, scale, name):
    vols, _, d_vol, _, counts = _view(scale, name)
    got = engine.sizeshape3d(d_vol, counts).cpu().numpy()
    want = np.concatenate([sizeshape3d_ref.sizeshape3d(v, n=c) for v, c in zip(vols, counts)])
    check_sizeshape3d(got, want, tag=f"scale, {name}")
    assert np.array_equal(got[:, 0] == 0, _absent(vols, counts))


@pytest.mark.parametrize("name", list(VIEWS))
def test_coloc3d_and_texture3d_read_an_object_table_filled_beyond_the_first_pass(engine, scale, name):
    """One pair and one channel: k_volume_table's stride (a row it missed would come back as a row of NaN)."""
    vols, pf, d_vol, d_pf, counts = _view(scale, name, "pf")
    got = engine.coloc3d(d_vol, d_pf, [(0, 1)], counts)
    check("coloc3d", got, coloc3d_ref.coloc3d_batch(vols, pf, [(0, 1)], counts), f"scale, {name}")
    assert np.array_equal(np.isnan(got.cpu().numpy()).all(axis=1), _absent(vols, counts))
    vols, px, d_vol, d_px, counts = _view(scale, name)
    got = engine.texture3d(d_vol, d_px, 1, counts, scale=1)
    want = texture3d_ref.texture3d_batch(vols, px, 1, counts, 1)
    check("texture3d", got, want, f"scale, {name}")
    present = ~_absent(vols, counts)
    assert np.isfinite(want[present]).any(axis=1).sum() >= present.sum() - 2  # (the one-voxel object has no pair)


@pytest.mark.parametrize("name", list(VIEWS))
def test_stitch_planes_writes_the_labels_back_beyond_the_first_pass(engine, scale, name):
    import torch

    from oracle import volume_restated as vr

    F, Z, Y, X = VIEWS[name]
    planes = vs.per_plane_labels(scale["vol"]).reshape(F, Z, Y, X)
    volume, counts = engine.stitch_planes(torch.from_numpy(planes).cuda(), threshold=0.01)
    got = volume.cpu().numpy()
    for f in range(F):
        want, k = vr.stitch3d(planes[f], 0.01)
        assert int(counts[f]) == k and k >= 2
        assert np.array_equal(got[f], want), (name, f, np.argwhere(got[f] != want)[:4])
    assert np.array_equal(got.reshape(vs.SHAPE) > 0, scale["vol"] > 0)  # the last planes were written, not left as they were allocated
