"""
tests/relate3d_ref.py, the restatement the GPU tests of `relate3d` compare with, pinned without a device: to the hand-worked example of
the header, to np.bincount / scipy.ndimage (overlaps, label sums, centres), to what each scene was built to show, and — on stacks of one
plane — to tests/relate_ref.py, the 2-D family's restatement, bit for bit.  The tertiary volume is pinned to relate_ref.tertiary plane
by plane.
"""
import numpy as np
import pytest
from scipy import ndimage

from tests import relate3d_ref as ref
from tests import relate_ref as ref2


def test_names():
    assert ref.names("cell") == ref2.names("cell") and len(ref.names("x")) == 5


def test_worked_example_by_hand():
    a, b = ref.worked()
    ra, rb = ref.relate3d(a, b)
    assert np.array_equal(ra[:, :3], ref.WORKED_NUCLEI[:, :3]) and np.array_equal(rb[:, :3], ref.WORKED_CELLS[:, :3])
    assert np.allclose(ra[:, 3:], ref.WORKED_NUCLEI[:, 3:], rtol=1e-15, atol=0)
    assert np.allclose(rb[:, 3:], ref.WORKED_CELLS[:, 3:], rtol=1e-15, atol=0)
    for shrink, volumes in ref.WORKED_TERTIARY_VOLUMES.items():
        t = ref.tertiary(b, a, shrink)
        assert (int((t == 1).sum()), int((t == 2).sum())) == volumes


def test_outline_is_taken_plane_by_plane():
    v = np.zeros((3, 7, 7), np.uint16)
    v[:, 1:6, 1:6] = 1
    edge = ref.outline(v)
    assert not edge[:, 2:5, 2:5].any()  # the interior of the first and last plane too: they are no borders
    assert edge[:, 1:6, 1:6].sum() == 3 * 16
    v[1, 3, 3] = 0  # a hole in the middle plane: its in-plane neighbours become outline voxels, those above and below do not
    edge = ref.outline(v)
    assert edge[1, 2:5, 2:5].sum() == 8 and not edge[0, 2:5, 2:5].any() and not edge[2, 2:5, 2:5].any()
    full = np.ones((2, 3, 4), np.uint16)  # an object filling its planes: only the rows and columns on the frame
    assert np.array_equal(ref.outline(full)[0], np.array([[1, 1, 1, 1], [1, 0, 0, 1], [1, 1, 1, 1]], bool))


@pytest.mark.parametrize("name", list(ref.scenes()))
def test_scenes_against_bincount_and_ndimage(name):
    a, b, na, nb = ref.scenes()[name]
    (ra, rb) = ref.relate3d(a, b, na, nb)
    assert ra.shape == (na, 5) and rb.shape == (nb, 5)
    for x, y, nx, ny, rows in ((a, b, na, nb, ra), (b, a, nb, na, rb)):
        xi, yi = x.astype(np.int64), y.astype(np.int64)
        hist = np.bincount((np.where(xi <= nx, xi, 0) * (ny + 1) + np.where(yi <= ny, yi, 0)).ravel(), minlength=(nx + 1) * (ny + 1))
        hist = hist.reshape(nx + 1, ny + 1)[1:, 1:]
        if ny:
            assert np.array_equal(rows[:, 1], hist.max(axis=1))
            assert np.array_equal(rows[:, 0], np.where(hist.max(axis=1) > 0, hist.argmax(axis=1) + 1, 0))  # argmax: the first maximum
        else:
            assert not rows[:, :3].any()
        assert np.array_equal(np.isnan(rows[:, 3]), rows[:, 0] == 0) and np.array_equal(np.isnan(rows[:, 4]), rows[:, 0] == 0)
    assert ra[:, 2].sum() == (rb[:, 0] > 0).sum() and rb[:, 2].sum() == (ra[:, 0] > 0).sum()
    for vol, n in ((a, na), (b, nb)):
        c = ref.centres(vol, n)
        present = np.bincount(vol.ravel(), minlength=n + 1)[1:n + 1] > 0
        assert np.array_equal(np.isnan(c[:, 0]), ~present)
        want = np.asarray(ndimage.center_of_mass(np.ones(vol.shape), vol, np.flatnonzero(present) + 1)).reshape(-1, 3)
        assert np.allclose(c[present], want, rtol=1e-13, atol=0)
    # column 3 against the centres, column 4 against a brute-force minimum over the outline
    cb, edge = ref.centres(b, nb), ref.outline(b)
    for row in range(na):
        p = int(ra[row, 0])
        if p:
            c = ref.centres(a, na)[row]
            assert np.isclose(ra[row, 3], np.linalg.norm(cb[p - 1] - c), rtol=1e-14)
            q = np.argwhere(edge & (b == p)).astype(np.float64)
            assert np.isclose(ra[row, 4], np.sqrt(((q - c) ** 2).sum(axis=1).min()), rtol=1e-14)


def test_what_the_scenes_were_built_for():
    sc = ref.scenes()
    ra, rb = ref.relate3d(*sc["tie"])
    assert ra[0, :2].tolist() == [1, 6] and rb[:, 2].tolist() == [1, 0]  # six voxels in either cell: the smaller label
    ra, rb = ref.relate3d(*sc["orphan"])
    assert ra[:, 0].tolist() == [1, 0, 0] and np.isnan(ra[1:, 3:]).all()  # no cell; a value above the count only
    ra, rb = ref.relate3d(*sc["absent"])
    assert ra[[1, 3, 4], :3].tolist() == [[0, 0, 0]] * 3 and np.isnan(ra[[1, 3, 4], 3:]).all()
    assert rb[[0, 2, 4, 5], :3].tolist() == [[0, 0, 0]] * 4
    ra, rb = ref.relate3d(*sc["three_children"])
    assert rb[0, 2] == 3 and ra[:, 0].tolist() == [1, 1, 1] and ra[2, 1] == 1
    ra, rb = ref.relate3d(*sc["faces"])
    assert (ra[:, 0] > 0).all() and ra[0, 4] == 0.0  # the child on row 0 sits on its parent's outline
    ra, rb = ref.relate3d(*sc["thin_parents"])
    assert ra[:, :2].tolist() == [[1, 1], [2, 9]]
    assert ra[0, 3] == 0.0 and ra[0, 4] == 0.0  # the one-voxel parent is its own outline, at the child's centre
    # the second parent is a 5 x 6 rectangle on the plane above the child's centre (1, 8, 10): its centre is (2, 8, 10.5), and its
    # 3 x 4 interior is no outline, so the nearest outline voxel is two rows or columns away
    assert ra[1, 3] == np.sqrt(1.25) and ra[1, 4] == np.sqrt(5.0)


def test_spacing_scales_each_axis():
    a, b, na, nb = ref.scenes()["three_children"]
    unit, _ = ref.relate3d(a, b, na, nb)
    twice, _ = ref.relate3d(a, b, na, nb, spacing=(2.0, 2.0, 2.0))
    assert np.array_equal(twice[:, :3], unit[:, :3]) and np.allclose(twice[:, 3:], 2 * unit[:, 3:], rtol=1e-15)
    aniso, _ = ref.relate3d(a, b, na, nb, spacing=(2.5, 1.0, 1.0))
    ca, cb = ref.centres(a, na), ref.centres(b, nb)
    d = (cb[0] - ca) * np.array([2.5, 1.0, 1.0])
    assert np.allclose(aniso[:, 3], np.sqrt((d * d).sum(axis=1)), rtol=1e-14)
    assert (aniso[:, 4] >= unit[:, 4]).all()


@pytest.mark.parametrize("name", list(ref2.scenes()))
def test_one_plane_is_the_2d_restatement_bit_for_bit(name):
    a, b, na, nb = ref2.scenes()[name]
    ra, rb = ref.relate3d(a[None], b[None], na, nb)
    wa, wb = ref2.relate(a, b, na, nb)
    assert np.array_equal(ra.view(np.int64), wa.view(np.int64)) and np.array_equal(rb.view(np.int64), wb.view(np.int64))
    assert np.array_equal(ra, wa, equal_nan=True) and np.array_equal(rb, wb, equal_nan=True)


def test_one_plane_strip_and_batch_are_the_2d_restatement():
    a, b = ref2.strip()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ref.relate3d(a[None], b[None]), ref2.relate(a, b)))
    tiles_a, tiles_b, ca, cb = ref2.batch3()
    got = ref.relate3d_batch([t[None] for t in tiles_a], [t[None] for t in tiles_b], ca, cb)
    want = [np.concatenate([ref2.relate(x, y, n, m)[k] for x, y, n, m in zip(tiles_a, tiles_b, ca, cb)]) for k in (0, 1)]
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True)


@pytest.mark.parametrize("shrink", [True, False])
def test_tertiary_volume_is_the_2d_tertiary_of_every_plane(shrink):
    for name, (outer, inner) in ref.tertiary_scenes().items():
        t = ref.tertiary(outer, inner, shrink)
        assert t.dtype == np.uint16 and t.shape == outer.shape
        for z in range(outer.shape[0]):
            assert np.array_equal(t[z], ref2.tertiary(outer[z], inner[z], shrink)), (name, z)
        assert np.array_equal(t[inner == 0], outer[inner == 0]) and set(np.unique(t)) <= set(np.unique(outer)) | {0}
    for name, (outer, inner) in ref2.tertiary_scenes().items():
        assert np.array_equal(ref.tertiary(outer[None], inner[None], shrink)[0], ref2.tertiary(outer, inner, shrink)), name


def test_caps_lose_their_interior():
    """A 5 x 5 nucleus on three planes inside a cell: the plane-wise rule removes the 3 x 3 interior of every plane, the first and the
    last one included, although cytoplasm lies above and below them."""
    outer, inner = np.zeros((5, 9, 9), np.uint16), np.zeros((5, 9, 9), np.uint16)
    outer[:] = 1
    inner[1:4, 2:7, 2:7] = 1
    t = ref.tertiary(outer, inner, True)
    assert int((t == 0).sum()) == 3 * 9 and not t[1:4, 3:6, 3:6].any() and t[0].all() and t[4].all()
    assert int((ref.tertiary(outer, inner, False) == 0).sum()) == 3 * 25
    covered = ref.tertiary(*ref.tertiary_scenes()["covered"], True)
    assert not (covered == 2).any()  # a label that loses every voxel is absent
