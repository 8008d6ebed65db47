"""
The preconditions of tests/test_gpu_volume_scale.py, checked without a GPU: the shared thin stack (tests/volume_scale_ref.py) has
more work items than each volume kernel's grid cap covers in one pass, and its objects lie where the GPU tests say they lie in each
kernel's own order of work items: in the first pass, wholly beyond it, across its boundary.
"""
import numpy as np
import pytest

from tests import volume_scale_ref as vs
from tests.volume_checks import quiet_numpy  # noqa: F401 (an autouse fixture: the oracle's one-voxel variance warns)

SHAPES = {"one stack": (1, *vs.SHAPE), "two stacks": vs.BATCH_SHAPE}


def _coords(vol4, lab):
    f, z, y, x = np.nonzero(vol4 == lab)
    return f, z, y, x


def _passes(vol4, lab):
    """-> per kernel, the set of passes of its grid-stride loop that touch label `lab` (0 = the first pass)."""
    f, z, y, x = _coords(vol4, lab)
    return {"segments": set(np.unique(vs.segment_items(f, z, y, x, vol4.shape) // vs.SEGMENT_CAP)),
            "tiles": set(np.unique(vs.tile_items(f, z, y, x, vol4.shape) // vs.TILE_CAP)),
            "voxels": set(np.unique(vs.voxel_items(f, z, y, x, vol4.shape) // vs.VOXEL_CAP))}


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_stack_exceeds_every_grid_cap(name):
    segments, tiles, voxels = vs.n_items(SHAPES[name])
    assert segments > vs.SEGMENT_CAP and tiles > vs.TILE_CAP and voxels > vs.VOXEL_CAP
    assert segments < 2 * vs.SEGMENT_CAP and voxels < 3 * vs.VOXEL_CAP  # (what the tables below assume)
    assert int(np.prod(SHAPES[name])) * 2 <= 18 << 20  # 17 MB of labels


def test_the_item_formulas_number_every_item_once():
    """On a small batch: the three index formulas are bijections onto 0 .. n_items - 1 (segments, voxels), and a tile index stays
    below the number of tiles."""
    shape4 = (2, 9, 17, 70)
    f, z, y, x = np.indices(shape4).reshape(4, -1)
    segments, tiles, voxels = vs.n_items(shape4)
    assert np.array_equal(np.unique(vs.segment_items(f, z, y, x, shape4)), np.arange(segments))
    assert np.array_equal(np.sort(vs.voxel_items(f, z, y, x, shape4)), np.arange(voxels))
    t = vs.tile_items(f, z, y, x, shape4)
    assert t.min() == 0 and t.max() == tiles - 1


def test_where_the_objects_of_one_stack_lie_in_each_kernel_s_passes():
    vol, n, px = vs.stack()
    assert vol.shape == vs.SHAPE and n == vs.N_OBJECTS and px.shape == (2, *vs.SHAPE) and int(vol.max()) == n
    counts = np.bincount(vol.ravel(), minlength=n + 1)[1:]
    assert (counts > 0).all() and counts.max() < 400 and counts.sum() < 1500  # few and small: the references stay quick
    v4 = vol[None]
    p = {lab: _passes(v4, lab) for lab in range(1, n + 1)}
    assert p[1] == {"segments": {0}, "tiles": {0}, "voxels": {0}}                      # the first pass of every kernel
    assert p[2]["tiles"] == {0, 1} and p[2]["voxels"] == {0, 1} and p[2]["segments"] == {0}  # across two boundaries
    assert p[3] == {"segments": {0}, "tiles": {1}, "voxels": {1}}
    assert p[4]["segments"] == {0, 1} and 0 not in p[4]["tiles"] and p[4]["voxels"] == {1, 2}   # across the segment boundary
    for lab in (5, 6):                                                                     # wholly beyond, for every kernel
        assert 0 not in p[lab]["segments"] and 0 not in p[lab]["tiles"] and 0 not in p[lab]["voxels"], lab
    f, z, y, x = _coords(v4, 6)
    assert (int(z[0]), int(y[0]), int(x[0])) == (vs.SHAPE[0] - 1, vs.SHAPE[1] - 1, 0) and len(z) == 1  # the last voxel of the stack
    assert (vol[:, 0] > 0).any() and (vol[:, -1] > 0).any() and (vol[-1] > 0).any()  # faces of the stack are touched


def test_where_the_objects_of_the_batch_of_two_lie():
    """The same memory as [2, 65, 65536, 1]: object 2 is cut in two by the stack boundary, stack 0 has no voxel of labels 4 to 6,
    stack 1 none of label 1; a strided work item has f = 1."""
    vol, n, _ = vs.stack()
    v4 = vol.reshape(vs.BATCH_SHAPE)
    present = [[lab for lab in range(1, n + 1) if (v4[f] == lab).any()] for f in range(2)]
    assert present == [[1, 2], [2, 3, 4, 5, 6]]
    for lab in (5, 6):
        f, z, y, x = _coords(v4, lab)
        assert (f == 1).all()
        assert (vs.segment_items(f, z, y, x, v4.shape) >= vs.SEGMENT_CAP).all() and (vs.tile_items(f, z, y, x, v4.shape) >= vs.TILE_CAP).all()


def test_no_costes_probe_of_the_stack_sits_at_a_sign_change():
    """As tests/test_cpu_coloc3d_ref.py shows for the inputs of the coloc3d suite: the Costes columns come out of a search on the
    sign of a correlation, so an input must keep every probe away from 0."""
    from tests import coloc3d_ref as c3

    vol, n, px = vs.stack()
    pf = c3.unit_float(px)
    probes = c3.costes_probes(vol, pf[0], pf[1], n)
    assert len(probes) == n
    for lab, log in enumerate(probes, 1):
        vals = np.asarray([v for v in log if not np.isnan(v)])
        assert vals.size == 0 or np.abs(vals).min() > c3.PROBE_MARGIN, (lab, np.abs(vals).min())
    assert sum(len(log) for log in probes) > 20


def test_per_plane_labels_are_sequential_and_cover_the_objects():
    vol, _, _ = vs.stack()
    planes = vs.per_plane_labels(vol)
    assert np.array_equal(planes > 0, vol > 0)
    for z in (3, 64, 129):
        present = np.unique(planes[z][planes[z] > 0])
        assert np.array_equal(present, np.arange(1, len(present) + 1)) and len(present) >= 1
