"""
GPU parity of the `SurfaceArea` column of `FeatureEngine.sizeshape3d(..., surface_area=True)` (aliby_amd/csrc/feat_surface3d.hip).

The kernel counts, per object, the 2 x 2 x 2 cells of the volume grid by configuration in exact integers and sums
float64(count) * area in increasing configuration, without contraction.  tests/surface3d_ref.py restates that in NumPy, so fed the
library's own table (FeatureEngine.surface3d_table) the two must agree BIT FOR BIT: there is no tolerance in this file, except
where the comparison is with scikit-image's recorded numbers (1e-4 relative, README "Parity"; tests/test_cpu_surface3d_ref.py
measures what the difference really is).
"""
import numpy as np
import pytest

from tests import surface3d_ref as ref

pytestmark = pytest.mark.gpu

UNIT = (1.0, 1.0, 1.0)
ANISO = (3.0, 0.7, 1.3)
GRID_CAP = 8192  # A3_GRID_CAP of feat_surface3d.hip: workgroups per launch, one 8 x 8 x 64 tile of cells each per pass


def _run(engine, vols, counts=None, spacing=UNIT):
    """vols: [Z,Y,X] label arrays of one shape -> (SurfaceArea float64 [sum counts] from the GPU, counts)."""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    counts = [int(v.max()) for v in stack] if counts is None else [int(c) for c in counts]
    got = engine.sizeshape3d(torch.from_numpy(stack).cuda(), counts, spacing=spacing, surface_area=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (sum(counts), 20)
    return got.cpu().numpy()[:, 19].copy(), counts


def _want(engine, vols, counts, spacing=UNIT):
    table = engine.surface3d_table(spacing)
    rows = [ref.surface_area(v, c, spacing, table) for v, c in zip(vols, counts)]
    return np.concatenate(rows) if rows else np.zeros(0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _touches_every_face(vol):
    return all((f > 0).any() for f in (vol[0], vol[-1], vol[:, 0], vol[:, -1], vol[:, :, 0], vol[:, :, -1]))


# ------------------------------------------------------------------------------------------------ 1. random irregular labels
@pytest.mark.parametrize("spacing", [UNIT, ANISO], ids=["unit", "aniso"])
@pytest.mark.parametrize("seed,shape", [(0, (2, 2, 2)), (1, (2, 3, 70)), (2, (5, 64, 64)), (3, (7, 61, 83)), (4, (9, 17, 130)), (5, (8, 8, 64)),
                                        (6, (9, 9, 65)), (7, (10, 10, 66))])
def test_random_labels_equal_the_restatement_bit_for_bit(engine, seed, shape, spacing):
    """One cell, Z at its minimum, sizes that are no tile multiple, exactly one tile of voxels, one tile of cells (9 x 9 x 65), one cell
    past it on every axis (10 x 10 x 66)."""
    vol, n = ref.random_labels(seed, shape)
    assert n >= 1
    if min(shape) > 2:
        a, b = vol[:, :, :-1], vol[:, :, 1:]
        assert n >= 3 and _touches_every_face(vol) and ((a != b) & (a > 0) & (b > 0)).any()
    got, counts = _run(engine, [vol], spacing=spacing)
    want = _want(engine, [vol], counts, spacing)
    assert np.isfinite(want).all() and (want > 0).all()
    assert _same_bits(got, want), (shape, got, want)


def test_a_dense_binary_volume_holds_every_configuration(engine):
    vol = (np.random.default_rng(0).random((6, 20, 40)) < 0.5).astype(np.uint16)
    hist = ref.label_histogram(vol, 1)
    assert (hist[1:255] > 0).all()  # all 254 mixed configurations
    for spacing in (UNIT, ANISO):
        got, counts = _run(engine, [vol], spacing=spacing)
        assert _same_bits(got, _want(engine, [vol], counts, spacing))


def test_eight_labels_in_every_window(engine):
    z, y, x = np.mgrid[:5, :11, :70]
    vol = (1 + 4 * ((z + 1) % 2) + 2 * ((y + 1) % 2) + ((x + 1) % 2)).astype(np.uint16)
    assert len(np.unique(vol[1:3, 3:5, 63:65])) == 8
    for spacing in (UNIT, ANISO):
        got, counts = _run(engine, [vol], spacing=spacing)
        assert counts == [8]
        assert _same_bits(got, _want(engine, [vol], counts, spacing))


# ------------------------------------------------------------------------------------------------ 2. borders and counts
def test_faces_absent_labels_labels_above_the_count_and_an_empty_count(engine):
    shape = (7, 30, 75)
    a, na = ref.random_labels(11, shape)
    b, nb = ref.random_labels(12, shape, n_seeds=7)
    c, nc = ref.random_labels(13, shape, n_seeds=6)
    assert _touches_every_face(a) and nb >= 2 and nc >= 4
    vols, counts = [a, b, c], [na + 1, 0, nc - 2]  # an announced label without voxels; nothing announced; two labels not announced
    got, _ = _run(engine, vols, counts)
    want = _want(engine, vols, counts)
    assert np.isnan(want[na]) and np.isfinite(np.delete(want, na)).all() and len(want) == na + 1 + nc - 2
    assert _same_bits(got, want)
    # no object at all: an empty block of 20 columns
    import torch

    out = engine.sizeshape3d(torch.from_numpy(b[None]).cuda(), [0], surface_area=True)
    assert tuple(out.shape) == (0, 20)


def test_closed_forms_on_the_device(engine):
    one = np.zeros((3, 3, 3), np.uint16)
    one[1, 1, 1] = 1
    got, _ = _run(engine, [one])
    assert abs(got[0] - 4 * np.sqrt(3)) <= 1e-12
    slab = np.zeros((5, 7, 9), np.uint16)
    slab[2] = 1
    got, _ = _run(engine, [slab])
    assert got[0] == 2.0 * 6 * 8  # open at the sides
    full = np.ones((2, 3, 4), np.uint16)
    got, _ = _run(engine, [full, np.zeros_like(full)], [2, 1])
    assert got[0] == 0.0 and np.isnan(got[1]) and np.isnan(got[2])  # fills the volume: 0 (scikit-image raises); absent: NaN


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_batch_run_and_neighbour_independence_bitwise(engine):
    shape = (9, 50, 70)
    a, na = ref.random_labels(21, shape)
    b, _ = ref.random_labels(22, shape, n_seeds=14)
    c, _ = ref.random_labels(23, shape, n_seeds=5)
    alone, _ = _run(engine, [a], spacing=ANISO)
    first, cf = _run(engine, [a, b, c], spacing=ANISO)
    last, cl = _run(engine, [b, c, a], spacing=ANISO)
    again, _ = _run(engine, [b, c, a], spacing=ANISO)
    assert _same_bits(first[:na], alone) and _same_bits(last[-na:], alone) and _same_bits(again, last)
    for lab in (1, na):  # every other label erased: an object's value is its own
        only = np.where(a == lab, a, 0).astype(np.uint16)
        got, _ = _run(engine, [only], [na], spacing=ANISO)
        assert _same_bits(got[lab - 1], alone[lab - 1]) and np.isnan(np.delete(got, lab - 1)).all()


# ------------------------------------------------------------------------------------------------ 4. beyond the first pass
def test_tiles_beyond_the_grid_cap(engine):
    """2 x 32770 x 66 voxels: 1 x 4097 x 2 = 8194 tiles of cells, two more than the launch has workgroups.  The last two tiles
    hold the single cell row y = 32768.  Label 1 lies in the first pass, label 2 across the boundary, label 3 wholly beyond it (a
    kernel without the loop reports it absent), in both x tiles."""
    Z, Y, X = 2, 32770, 66
    tiles = ((Z + 6) // 8) * ((Y + 6) // 8) * ((X + 62) // 64)
    assert tiles == GRID_CAP + 2
    vol = np.zeros((Z, Y, X), np.uint16)
    vol[:, 100:140, 3:60] = 1
    vol[0, 120, 10:20] = 0
    vol[:, 32750:32769, 60:66] = 2
    vol[1, 32769, 2:66] = 3
    got, counts = _run(engine, [vol], spacing=ANISO)
    want = _want(engine, [vol], counts, ANISO)
    assert np.isfinite(want).all() and (want > 0).all()
    assert _same_bits(got, want), (got, want)


# ------------------------------------------------------------------------------------------------ 5. scikit-image
def test_fixture_volumes_equal_scikit_image(engine):
    worst = 0.0
    for name, lab, n, recorded in ref.fixture_volumes():
        for spacing, want in recorded.items():
            got, _ = _run(engine, [lab], [n], spacing=spacing)
            assert np.all(np.abs(got - want) <= 1e-4 * np.abs(want)), (name, spacing, got, want)
            worst = max(worst, float((np.abs(got - want) / want).max()))
            assert _same_bits(got, _want(engine, [lab], [n], spacing))
    print(f"surface3d on the device against scikit-image's per-label mesh areas: worst relative difference {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 6. the rest of sizeshape3d
def test_the_other_nineteen_columns_are_untouched(engine):
    import torch

    from aliby_amd.extraction.features import sizeshape3d_names

    a, na = ref.random_labels(31, (7, 61, 83))
    b, nb = ref.random_labels(32, (7, 61, 83), n_seeds=6)
    stack, counts = torch.from_numpy(np.stack([a, b])).cuda(), [na, nb + 1]
    plain = engine.sizeshape3d(stack, counts, spacing=ANISO)
    more = engine.sizeshape3d(stack, counts, spacing=ANISO, surface_area=True)
    assert tuple(plain.shape) == (na + nb + 1, 19) and tuple(more.shape) == (na + nb + 1, 20)
    assert len(sizeshape3d_names()) == 19 and sizeshape3d_names(True)[19] == "SurfaceArea"
    assert _same_bits(more.cpu().numpy()[:, :19], plain.cpu().numpy())
    assert np.isnan(more.cpu().numpy()[-1, 19])
    assert tuple(engine.sizeshape3d(stack, counts, surface_area=False).shape) == (na + nb + 1, 19)


def test_a_volume_thinner_than_a_cell_is_refused_before_any_launch(engine):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    flat = torch.ones((1, 1, 8, 8), dtype=torch.uint16, device="cuda")
    with pytest.raises(ValueError):
        engine.sizeshape3d(flat, [1], surface_area=True)
    assert tuple(engine.sizeshape3d(flat, [1]).shape) == (1, 19)  # the default call takes it as before
    for bad in [(0.0, 1.0, 1.0), (1.0, 1.0, float("nan"))]:
        with pytest.raises(ValueError):
            engine.sizeshape3d(torch.ones((1, 2, 8, 8), dtype=torch.uint16, device="cuda"), [1], spacing=bad, surface_area=True)
    # the raw C entry: an error status, nothing written
    fn = engine.lib.aliby_features_surface3d
    off, sp = np.asarray([0, 1], np.int32), np.ones(3)
    out = torch.full((1, 20), 7.0, dtype=torch.float64, device="cuda")
    for Z, Y, X in ((1, 8, 8), (8, 1, 8), (8, 8, 1)):
        rc = fn(engine.ctx.handle, _ptr(flat), 1, Z, Y, X, _ptr(off), _ptr(sp), _ptr(out), 20, 19, _stream_ptr())
        assert rc == _lib.ERR_INVALID
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert fn(engine.ctx.handle, _ptr(flat), 1, 2, 4, 8, _ptr(off), _ptr(sp), _ptr(out), 19, 19, _stream_ptr()) == _lib.ERR_INVALID  # no room for the column
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert fn(engine.ctx.handle, _ptr(flat), 1, 2, 4, 8, _ptr(off), _ptr(sp), _ptr(out), 20, 19, _stream_ptr()) == _lib.OK
    torch.cuda.synchronize()
    row = out.cpu().numpy()[0]
    assert (row[:19] == 7.0).all() and row[19] == 0.0  # (the object fills its 2 x 4 x 8 volume)
