"""
FeatureEngine.secondary_volume (csrc/feat_secondary3d.hip: "Distance - N" of CellProfiler's IdentifySecondaryObjects on volume labels,
on an integer lattice) against the brute-force restatement tests/secondary3d_ref.py, bit for bit in every case of
tests/secondary3d_cases.py: shapes that break the tiling (one plane, one column along each axis, a stack smaller than every halo,
narrower than a wave, a batch whose Z crosses a z segment, whose Y crosses a row group and whose X crosses a 256-block), contents that
exercise the tie rule along and between the axes, the sentinel, the 16-bit distance field and the stack edges; then one plane against
`secondary_labels`, batches, a side stream, the arguments, the C entry's refusals and the host form.  No kernel caps its grid, so no
case has to reach past a first pass.
"""
import numpy as np
import pytest

from tests import secondary3d_cases as cases
from tests.secondary3d_cases import CASES, PAIRS, UNIT, want

pytestmark = pytest.mark.gpu


def run(engine, volumes, n, spacing):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    dev = to_device_u16(volumes)
    got = engine.secondary_volume(dev, n, spacing)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint16 and got.shape == dev.shape and got.data_ptr() != dev.data_ptr()
    assert np.array_equal(dev.cpu().numpy(), volumes)  # the input is left alone
    return got.cpu().numpy()


@pytest.mark.parametrize("name, n, spacing", PAIRS)
def test_exact(engine, name, n, spacing):
    volumes = CASES[name][0]
    got, exp = run(engine, volumes, n, spacing), want(name, n, spacing)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (f"{name} N={n} spacing={spacing}: {len(bad)} voxels differ, first at {bad[0]}: got {got[tuple(bad[0])]}, "
                           f"want {exp[tuple(bad[0])]}")
    assert np.array_equal(got[volumes != 0], volumes[volumes != 0])


@pytest.mark.parametrize("n", [1, 5, 64])
def test_one_plane_is_secondary_labels(engine, n):
    """Z == 1 with unit spacing: the bits of the 2-D kernels, on one tile and on a batch."""
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    tiles = cases.sprinkle((3, 1, 64, 96), 24, 5)
    for vol in (CASES["one_plane"][0], tiles):
        dev = to_device_u16(vol)
        stack = engine.secondary_volume(dev, n)
        flat = engine.secondary_labels(dev[:, 0], n)
        torch.cuda.synchronize()
        assert torch.equal(stack[:, 0].view(torch.int16), flat.view(torch.int16))
    # and the planes of a stack do see one another: the same planes as a [1,3,Y,X] stack differ from the three tiles
    moved = engine.secondary_volume(to_device_u16(tiles[:, 0][None]), 5)
    assert not torch.equal(moved[0].view(torch.int16), engine.secondary_labels(to_device_u16(tiles[:, 0]), 5).view(torch.int16))


@pytest.mark.parametrize("n, spacing", [(1, UNIT), (5, UNIT), (50, (13, 5, 5))])
def test_alone_in_a_batch_and_on_a_side_stream(engine, n, spacing):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    name = "2x34x10x260_batch"
    other, stack = CASES[name][0]
    alone = engine.secondary_volume(to_device_u16(stack[None]), n, spacing)
    batch = engine.secondary_volume(to_device_u16(np.stack([other, stack, np.zeros_like(stack), stack])), n, spacing)
    torch.cuda.synchronize()
    assert torch.equal(alone[0].view(torch.int16), batch[1].view(torch.int16))
    assert torch.equal(alone[0].view(torch.int16), batch[3].view(torch.int16)) and not batch[2].cpu().numpy().any()
    side = torch.cuda.Stream()
    dev = to_device_u16(stack[None])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        streamed = engine.secondary_volume(dev, n, spacing)
    side.synchronize()
    assert torch.equal(alone.view(torch.int16), streamed.view(torch.int16))
    assert np.array_equal(alone[0].cpu().numpy(), want(name, n, spacing)[1])


def test_arguments(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    name = "6x5x7_narrower_than_a_wave"
    vol = CASES[name][0]
    dev = to_device_u16(vol)
    for bad in (0, 256, -3, True, 2.5, None, "5"):
        with pytest.raises(ValueError, match="1..255"):
            engine.secondary_volume(dev, bad)
    for bad in ((1, 1), (1.0, 1.0, 1.0), (0.6, 0.23, 0.23), (0, 1, 1), (1, 256, 1), None, "111", (True, 1, 1)):
        with pytest.raises(ValueError, match="spacing"):
            engine.secondary_volume(dev, 3, bad)
    for n, spacing in ((65, UNIT), (200, (13, 5, 3))):
        with pytest.raises(ValueError, match="64 voxels"):
            engine.secondary_volume(dev, n, spacing)
    for bad in (dev[0], dev[None], dev.cpu(), dev.to(torch.int32), vol):
        with pytest.raises(ValueError, match="uint16"):
            engine.secondary_volume(bad, 3)
    assert np.array_equal(engine.secondary_volume(dev, 3.0).cpu().numpy(), want(name, 3))  # a float that holds an integer
    assert np.array_equal(engine.secondary_volume(dev, np.int64(6), np.array([3, 1, 1])).cpu().numpy(), want(name, 6, (3, 1, 1)))
    view = to_device_u16(np.pad(vol, ((0, 0), (0, 0), (0, 3), (0, 11))))[:, :, :5, :7]  # not contiguous
    assert not view.is_contiguous() and np.array_equal(engine.secondary_volume(view, 3).cpu().numpy(), want(name, 3))
    for shape in ((0, 2, 4, 4), (2, 0, 4, 4), (2, 3, 0, 4), (2, 3, 4, 0)):
        empty = engine.secondary_volume(torch.zeros(shape, dtype=torch.uint16, device=dev.device), 3)
        assert tuple(empty.shape) == shape and empty.dtype == torch.uint16


def test_c_entry(engine):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr, to_device_u16

    lib, h = engine.lib, engine.ctx.handle
    name = "tie_at_the_last_step"
    vol = CASES[name][0]
    dev = to_device_u16(vol)
    F, Z, Y, X = vol.shape
    need = int(lib.aliby_secondary_volume_workspace_bytes(F, Z, Y, X))
    assert need == 8 * F * Z * Y * X  # the plain form: two 4-byte words per voxel
    for shape in ((0, Z, Y, X), (F, 0, Y, X), (F, Z, 0, X), (F, Z, Y, 0), (-1, Z, Y, X)):
        assert int(lib.aliby_secondary_volume_workspace_bytes(*shape)) == 0
    work = torch.empty(need // 4, dtype=torch.int32, device=dev.device)
    out = torch.full_like(dev, 77)

    def call(primary=dev, shape=(F, Z, Y, X), n=5, spacing=UNIT, workspace=None, nbytes=need, result=out):
        workspace = _ptr(work) if workspace is None else workspace
        _lib.check(lib.aliby_secondary_volume(h, _ptr(primary) if primary is not None else 0, *shape, n, *spacing, workspace, nbytes,
                                              _ptr(result) if result is not None else 0, _stream_ptr()))

    call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want(name, 5))
    # the workspace need only be 4-byte aligned
    spare = torch.empty(need // 4 + 1, dtype=torch.int32, device=dev.device)
    assert spare.data_ptr() % 8 == 0
    call(n=10, spacing=(2, 2, 2), workspace=spare.data_ptr() + 4)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want(name, 10, (2, 2, 2)))
    out.fill_(77)
    work.fill_(0x5A5A5A5A)
    with pytest.raises(ValueError, match="alias"):  # out == primary
        call(result=dev)
    with pytest.raises(ValueError, match="workspace"):  # a workspace one word short
        call(nbytes=need - 4)
    with pytest.raises(ValueError, match="workspace"):
        call(workspace=0)
    for off in (1, 2, 3):  # misaligned by less than 4
        with pytest.raises(ValueError, match="aligned"):
            call(workspace=spare.data_ptr() + off)
    with pytest.raises(ValueError, match="NULL"):
        call(primary=None)
    with pytest.raises(ValueError, match="NULL"):
        call(result=None)
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="distance"):
            call(n=bad)
    for bad in ((0, 1, 1), (1, 256, 1), (1, 1, -2)):
        with pytest.raises(ValueError, match="spacing"):
            call(spacing=bad)
    for n, spacing in ((65, UNIT), (200, (13, 5, 3)), (255, (4, 4, 3))):
        with pytest.raises(ValueError, match="64 voxels"):
            call(n=n, spacing=spacing)
    with pytest.raises(ValueError):
        call(shape=(-1, Z, Y, X))
    # zero voxels: a successful no-op that touches nothing, with no buffers at all
    for shape in ((0, Z, Y, X), (F, 0, Y, X), (F, Z, 0, X), (F, Z, Y, 0)):
        _lib.check(lib.aliby_secondary_volume(h, 0, *shape, 5, 1, 1, 1, 0, 0, 0, _stream_ptr()))
    torch.cuda.synchronize()
    assert (out == 77).all() and (work == 0x5A5A5A5A).all() and np.array_equal(dev.cpu().numpy(), vol)  # no refused call wrote anything


def test_host_form(engine):
    from aliby_amd.extraction import functions

    name = "2x34x10x260_batch"
    stacks = CASES[name][0]
    one = functions.secondary_objects_3d(stacks[1], 50, (13, 5, 5))
    assert isinstance(one, np.ndarray) and one.dtype == np.uint16 and np.array_equal(one, want(name, 50, (13, 5, 5))[1])
    assert np.array_equal(functions.secondary_objects_3d(stacks[0], 5), want(name, 5)[0])
    with pytest.raises(ValueError):
        functions.secondary_objects_3d(stacks, 5)  # one stack
    with pytest.raises(ValueError):
        functions.secondary_objects_3d(stacks[0, 0], 5)
    with pytest.raises(ValueError):
        functions.secondary_objects_3d(stacks[0], 0)
    with pytest.raises(ValueError):
        functions.secondary_objects_3d(stacks[0], 5, (0.6, 0.23, 0.23))
