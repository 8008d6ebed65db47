"""
The `relate3d` family and the tertiary volume on the GPU (aliby_amd/csrc/feat_relate3d.hip) against tests/relate3d_ref.py, the NumPy
restatement that tests/test_cpu_relate3d_ref.py pins to hand values, to np.bincount / scipy.ndimage and to the 2-D restatement: the
engine calls, the C entry with a NULL output, and the host-array conveniences.  Parity with CellProfiler is unpinned.

Pass bar: Parent, ParentOverlap and the children count (columns 0-2) and the NaN pattern equal to the restatement exactly; the two
distances (columns 3-4) under rtol = atol = 1e-12, the 2-D family's bar: each is one sqrt of about a dozen float64 operations in one
fixed order, each rounded to at most 1 ulp, about 12 x 2^-52 = 3e-15.  Every comparison prints its largest difference first.  On a
stack of one plane all five columns carry the bits of `FeatureEngine.relate`.  Tertiary volumes are exact.  Measured on an MI355X:
see `compare`.
"""
import numpy as np
import pytest

from tests import relate3d_ref as ref
from tests import relate_ref as ref2

pytestmark = pytest.mark.gpu

MAX_GRID = 4096  # RELATE3D_MAX_GRID of feat_relate3d.hip: the LDS-form overlap launch and the finish launch stride above it
_REF = {}


def want(key, a, b, na=None, nb=None, spacing=(1.0, 1.0, 1.0)):
    """The restatement of a scene, computed once."""
    if key not in _REF:
        _REF[key] = ref.relate3d(a, b, na, nb, spacing)
    return _REF[key]


def compare(got, wanted, what):
    """Measured on an MI355X, largest absolute difference of a distance column against the restatement over every comparison of this
    file: 0 (every value carried the restatement's bits)."""
    got, wanted = np.asarray(got, float), np.asarray(wanted, float)
    assert got.shape == wanted.shape, (what, got.shape, wanted.shape)
    fin = ~np.isnan(wanted[:, ref.FLOAT])
    diff = np.abs(got[:, ref.FLOAT] - wanted[:, ref.FLOAT])[fin]
    print(f"{what}: rows {len(wanted)}, largest distance difference {diff.max() if diff.size else 0.0:.3e}")
    assert np.array_equal(np.isnan(got), np.isnan(wanted)), what
    assert np.array_equal(got[:, ref.EXACT], wanted[:, ref.EXACT]), what
    assert np.allclose(got[:, ref.FLOAT], wanted[:, ref.FLOAT], rtol=ref.RTOL, atol=ref.ATOL, equal_nan=True), what


def dev(stacks):
    from aliby_amd.extraction.engine import to_device_u16

    return to_device_u16(np.stack(stacks))


def run(engine, vols_a, vols_b, counts_a, counts_b, **kw):
    """-> (rows of A, rows of B) through windows of wider matrices: only columns col0 .. col0 + 4 may be written."""
    import torch

    na, nb = int(np.sum(counts_a)), int(np.sum(counts_b))
    out_a, out_b = engine.new_output(na, 8), engine.new_output(nb, 7)
    got_a, got_b = engine.relate3d(dev(vols_a), counts_a, dev(vols_b), counts_b, out_a=out_a, col0_a=2, out_b=out_b, col0_b=1, **kw)
    torch.cuda.synchronize()
    assert tuple(got_a.shape) == (na, 5) and tuple(got_b.shape) == (nb, 5)
    full_a, full_b = out_a.cpu().numpy(), out_b.cpu().numpy()
    assert np.isnan(full_a[:, :2]).all() and np.isnan(full_a[:, 7:]).all() and np.isnan(full_b[:, :1]).all() and np.isnan(full_b[:, 6:]).all()
    return full_a[:, 2:7].copy(), full_b[:, 1:6].copy()


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name", list(ref.scenes()))
def test_scenes(engine, name):
    """The worked example, an exact tie, a child under no parent, absent labels with counts above the largest label, a parent of three,
    objects on the faces of the volume, a one-voxel parent and a parent on one plane only; both directions."""
    a, b, na, nb = ref.scenes()[name]
    got_a, got_b = run(engine, [a], [b], [na], [nb])
    wa, wb = want(name, a, b, na, nb)
    compare(got_a, wa, f"{name} A"), compare(got_b, wb, f"{name} B")
    if name == "worked":
        assert np.array_equal(got_a[:, :3], ref.WORKED_NUCLEI[:, :3]) and np.array_equal(got_b[:, :3], ref.WORKED_CELLS[:, :3])
        assert np.allclose(got_a[:, 3:], ref.WORKED_NUCLEI[:, 3:], rtol=ref.RTOL, atol=ref.ATOL)
        assert np.allclose(got_b[:, 3:], ref.WORKED_CELLS[:, 3:], rtol=ref.RTOL, atol=ref.ATOL)
    if name == "tie":
        assert got_a[0, :2].tolist() == [1, 6]
    if name == "orphan":
        assert got_a[1:, :3].tolist() == [[0, 0, 0]] * 2 and np.isnan(got_a[1:, 3:]).all()


def test_the_scenes_of_one_shape_as_one_batch(engine):
    sc = {k: v for k, v in ref.scenes().items() if v[0].shape == ref.SHAPE}
    assert len(sc) >= 6
    got_a, got_b = run(engine, [v[0] for v in sc.values()], [v[1] for v in sc.values()], [v[2] for v in sc.values()], [v[3] for v in sc.values()])
    wa = np.concatenate([want(k, *v)[0] for k, v in sc.items()])
    wb = np.concatenate([want(k, *v)[1] for k, v in sc.items()])
    compare(got_a, wa, "batch A"), compare(got_b, wb, "batch B")


# ------------------------------------------------------------------------------------------------ one plane = the 2-D family
def test_one_plane_carries_the_bits_of_relate(engine):
    """Every scene of the 2-D restatement as [1,1,Y,X]: all five columns, viewed as int64, equal `FeatureEngine.relate`'s."""
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    for name, (a, b, na, nb) in ref2.scenes().items():
        la, lb = to_device_u16(a[None]), to_device_u16(b[None])
        flat = engine.relate(la, engine.object_table(la, max_labels=[na]), lb, engine.object_table(lb, max_labels=[nb]))
        vol = engine.relate3d(la[:, None], [na], lb[:, None], [nb])
        torch.cuda.synchronize()
        for k in (0, 1):
            assert torch.equal(bits(vol[k]), bits(flat[k])), (name, k, vol[k], flat[k])
        compare(vol[0].cpu().numpy(), ref2.relate(a, b, na, nb)[0], f"one plane, {name}")


def test_one_plane_batch_carries_the_bits_of_relate(engine):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    tiles_a, tiles_b, ca, cb = ref2.batch3()
    la, lb = to_device_u16(np.stack(tiles_a)), to_device_u16(np.stack(tiles_b))
    flat = engine.relate(la, engine.object_table(la, max_labels=ca), lb, engine.object_table(lb, max_labels=cb))
    vol = engine.relate3d(la[:, None], ca, lb[:, None], cb)
    torch.cuda.synchronize()
    assert torch.equal(bits(vol[0]), bits(flat[0])) and torch.equal(bits(vol[1]), bits(flat[1]))


# ------------------------------------------------------------------------------------------------ spacing
@pytest.mark.parametrize("spacing", [(2.5, 1.0, 1.0), (0.6, 0.23, 0.23)])
def test_spacing(engine, spacing):
    for name in ("worked", "faces", "thin_parents"):
        a, b, na, nb = ref.scenes()[name]
        got_a, got_b = run(engine, [a], [b], [na], [nb], spacing=spacing)
        wa, wb = want((name, spacing), a, b, na, nb, spacing)
        compare(got_a, wa, f"{name} A at {spacing}"), compare(got_b, wb, f"{name} B at {spacing}")


def test_unit_spacing_is_the_default_bit_for_bit(engine):
    import torch

    a, b, na, nb = ref.scenes()["faces"]
    one = engine.relate3d(dev([a]), [na], dev([b]), [nb], spacing=(1, 1, 1))
    default = engine.relate3d(dev([a]), [na], dev([b]), [nb])
    torch.cuda.synchronize()
    assert torch.equal(bits(one[0]), bits(default[0])) and torch.equal(bits(one[1]), bits(default[1]))


# ------------------------------------------------------------------------------------------------ the scratch form
def single_voxel_parents(n):
    """One stack [4,48,48]: B = its first n voxels in raster order, one object each (9216 = all of them); A = five blocks."""
    b = np.zeros(4 * 48 * 48, np.int64)
    b[:n] = np.arange(1, n + 1)
    b = b.reshape(4, 48, 48).astype(np.uint16)
    a = np.zeros((4, 48, 48), np.uint16)
    a[0:2, 2:6, 3:10], a[1:4, 20:23, 5:8], a[3, 30, 3:45], a[0, 0:2, 40:48], a[2:4, 46:48, 44:48] = 1, 2, 3, 4, 5
    return a, b


def test_9216_single_voxel_parents_take_the_scratch_form(engine):
    """One counter per label of the other set: 9217 ints are past the 32 KiB of the LDS form, so A's workgroups count in the
    context's scratch (and B's 9216 rows, more than MAX_GRID, are walked by striding workgroups in the LDS form)."""
    a, b = single_voxel_parents(9216)
    got_a, got_b = run(engine, [a], [b], [5], [9216])
    wa, wb = want("many", a, b, 5, 9216)
    compare(got_a, wa, "single-voxel parents A"), compare(got_b, wb, "single-voxel parents B")
    assert got_a[:, 1].tolist() == [1] * 5 and got_a[:, 2].tolist() == [56, 27, 42, 16, 16]
    assert (got_b[:, 0] > 0).sum() == 56 + 27 + 42 + 16 + 16


def test_the_8191_8192_boundary_between_lds_and_scratch(engine):
    """The same scene cut to 8191 labels (32 KiB of counters: LDS) and to 8192 (16 bytes more: scratch).  The two cuts differ in one
    voxel, which lies under no block of A, so all of A's rows must carry the same bits, and both equal the restatement."""
    a, b1 = single_voxel_parents(8191)
    _, b2 = single_voxel_parents(8192)
    got1, _ = run(engine, [a], [b1], [5], [8191])
    got2, rows2 = run(engine, [a], [b2], [5], [8192])
    compare(got1, want("8191", a, b1, 5, 8191)[0], "8191 labels A"), compare(got2, want("8192", a, b2, 5, 8192)[0], "8192 labels A")
    compare(rows2, want("8192", a, b2, 5, 8192)[1], "8192 labels B")
    shared = (a > 0) & (b1 != b2)
    assert not shared.any()  # voxel 8192 (z 3, y 26, x 31) lies under no block of A: all five rows are the shared region
    assert np.array_equal(got1.view(np.int64), got2.view(np.int64))


def test_more_rows_than_the_largest_grid(engine):
    """A stack of 5120 voxels, every voxel an object of A and of B (B's labels reversed): 5120 rows a side, more than MAX_GRID, so
    the overlap launches (LDS form) and the finish launches produce rows 4096.. in their second pass."""
    n = 4 * 32 * 40
    assert n > MAX_GRID
    a = np.arange(1, n + 1).reshape(4, 32, 40).astype(np.uint16)
    b = (n + 1 - a.astype(np.int64)).astype(np.uint16)
    got_a, got_b = run(engine, [a], [b], [n], [n])
    wa, wb = want("grid", a, b, n, n)
    compare(got_a, wa, "5120 rows A"), compare(got_b, wb, "5120 rows B")
    assert np.array_equal(got_a[:, 0], np.arange(n, 0, -1)) and (got_a[:, 1:3] == 1).all() and (got_a[:, 3:] == 0).all()


# ------------------------------------------------------------------------------------------------ determinism
def random_stack(shape, n_cells, n_nuclei, seed):
    rng = np.random.default_rng(seed)
    Z, Y, X = shape

    def boxes(n, lo, hi, dlo, dhi):
        vol = np.zeros(shape, np.uint16)
        for L in range(1, n + 1):
            d, h, w = rng.integers(dlo, dhi), *rng.integers(lo, hi, 2)
            z, y, x = rng.integers(0, Z - 1), rng.integers(0, Y - 2), rng.integers(0, X - 2)
            vol[z:z + d, y:y + h, x:x + w] = L  # (later boxes overwrite earlier ones: ragged shapes, some labels may vanish)
        return vol

    return boxes(n_nuclei, 2, 8, 1, 4), boxes(n_cells, 6, 20, 2, 6)


def test_one_stack_alone_and_in_a_batch_beside_a_large_object(engine):
    import torch

    a0, b0 = random_stack((6, 60, 70), 14, 20, 5)
    a1, b1 = np.zeros_like(a0), np.zeros_like(b0)
    a1[:, 2:58, 3:67] = 1  # one large object: 6 x 56 x 64 voxels
    b1[:, :, :35], b1[:, :, 35:] = 1, 2
    zero = np.zeros_like(a0)
    alone = engine.relate3d(dev([a0]), [20], dev([b0]), [14])
    batch = engine.relate3d(dev([a1, a0, zero]), [1, 20, 0], dev([b1, b0, zero]), [2, 14, 0])
    torch.cuda.synchronize()
    assert torch.equal(bits(alone[0]), bits(batch[0][1:21])) and torch.equal(bits(alone[1]), bits(batch[1][2:16]))
    wa, wb = want("random", a0, b0, 20, 14)
    compare(alone[0].cpu().numpy(), wa, "random A"), compare(alone[1].cpu().numpy(), wb, "random B")
    w1 = want("large", a1, b1, 1, 2)
    compare(batch[0][:1].cpu().numpy(), w1[0], "large A"), compare(batch[1][:2].cpu().numpy(), w1[1], "large B")
    again = engine.relate3d(dev([a1, a0, zero]), [1, 20, 0], dev([b1, b0, zero]), [2, 14, 0])  # run to run
    torch.cuda.synchronize()
    assert torch.equal(bits(again[0]), bits(batch[0])) and torch.equal(bits(again[1]), bits(batch[1]))


# ------------------------------------------------------------------------------------------------ empty sets, the C entry, refusals
def test_an_empty_set_on_either_side(engine):
    a, _, na, _ = ref.scenes()["worked"]
    zeros = np.zeros_like(a)
    got_a, got_b = run(engine, [a], [zeros], [na], [0])
    assert got_b.shape == (0, 5) and got_a[:, :3].tolist() == [[0, 0, 0]] * 3 and np.isnan(got_a[:, 3:]).all()
    got_a, got_b = run(engine, [zeros], [a], [0], [na])
    assert got_a.shape == (0, 5) and got_b[:, :3].tolist() == [[0, 0, 0]] * 3 and np.isnan(got_b[:, 3:]).all()
    got_a, got_b = run(engine, [zeros], [zeros], [0], [0])
    assert got_a.shape == (0, 5) and got_b.shape == (0, 5)
    got_a, got_b = run(engine, [a], [a], [0], [0])  # labels without a count are not measured
    assert got_a.shape == (0, 5) and got_b.shape == (0, 5)
    got_a, got_b = run(engine, [zeros, a], [zeros, zeros], [0, na], [2, 0])  # counts for labels that are all absent
    assert got_b[:, :3].tolist() == [[0, 0, 0]] * 2 and np.isnan(got_b[:, 3:]).all() and got_a[:, :3].tolist() == [[0, 0, 0]] * 3


def test_c_entry_with_one_output_null(engine):
    """aliby_features_relate3d with out_b NULL fills the rows of A alone, children count included (it needs B's parents all the same);
    bad arguments are refused with a message."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    a, b, na, nb = ref.scenes()["worked"]
    va, vb = dev([a]), dev([b])
    lib = engine.lib
    out = engine.new_output(na, 5)
    off_a, off_b, sp = np.asarray([0, na], np.int32), np.asarray([0, nb], np.int32), np.ones(3)
    head = [engine.ctx.handle, _ptr(va), _ptr(vb), 1, 3, 6, 8]
    _lib.check(lib.aliby_features_relate3d(*head, _ptr(off_a), _ptr(off_b), _ptr(sp), _ptr(out), 5, 0, 0, 0, 0, _stream_ptr()))
    torch.cuda.synchronize()
    compare(out.cpu().numpy(), want("worked", a, b, na, nb)[0], "C entry, out_b NULL")
    out_b = engine.new_output(nb, 5)
    _lib.check(lib.aliby_features_relate3d(*head, _ptr(off_a), _ptr(off_b), _ptr(sp), 0, 0, 0, _ptr(out_b), 5, 0, _stream_ptr()))
    torch.cuda.synchronize()
    compare(out_b.cpu().numpy(), want("worked", a, b, na, nb)[1], "C entry, out_a NULL")
    with pytest.raises(ValueError):  # columns past the row stride
        _lib.check(lib.aliby_features_relate3d(*head, _ptr(off_a), _ptr(off_b), _ptr(sp), _ptr(out), 5, 1, 0, 0, 0, _stream_ptr()))
    with pytest.raises(ValueError):  # offsets that are not monotone
        _lib.check(lib.aliby_features_relate3d(*head, _ptr(np.asarray([0, -1], np.int32)), _ptr(off_b), _ptr(sp), _ptr(out), 5, 0, 0, 0, 0,
                                               _stream_ptr()))
    with pytest.raises(ValueError):  # F <= 0
        _lib.check(lib.aliby_features_relate3d(engine.ctx.handle, _ptr(va), _ptr(vb), 0, 3, 6, 8, _ptr(off_a), _ptr(off_b), _ptr(sp), _ptr(out),
                                               5, 0, 0, 0, 0, _stream_ptr()))
    with pytest.raises(ValueError):  # a spacing of zero
        _lib.check(lib.aliby_features_relate3d(*head, _ptr(off_a), _ptr(off_b), _ptr(np.asarray([1.0, 0.0, 1.0])), _ptr(out), 5, 0, 0, 0, 0,
                                               _stream_ptr()))


def test_refusals_of_the_engine_method(engine):
    import torch

    a, b, na, nb = ref.scenes()["worked"]
    va, vb = dev([a]), dev([b])
    with pytest.raises(ValueError, match="shape"):
        engine.relate3d(va, [na], dev([np.pad(b, ((0, 0), (0, 1), (0, 0)))]), [nb])
    with pytest.raises(ValueError, match="uint16"):
        engine.relate3d(va.to(torch.int32), [na], vb, [nb])
    with pytest.raises(ValueError, match="uint16"):
        engine.relate3d(va, [na], vb[0], [nb])  # [Z,Y,X]
    with pytest.raises(ValueError, match="uint16"):
        engine.relate3d(a[None], [na], vb, [nb])  # a host array
    with pytest.raises(ValueError, match="counts"):
        engine.relate3d(va, [na, 1], vb, [nb])
    with pytest.raises(ValueError, match="counts"):
        engine.relate3d(va, [na], vb, [])
    with pytest.raises(ValueError, match="counts"):
        engine.relate3d(va, [-1], vb, [nb])
    for spacing in ((1, 1), (1, 0, 1), (1, -2, 1), (1, np.nan, 1), (np.inf, 1, 1)):
        with pytest.raises(ValueError):
            engine.relate3d(va, [na], vb, [nb], spacing=spacing)
    with pytest.raises(ValueError, match="rows"):
        engine.relate3d(va, [na], vb, [nb], out_a=engine.new_output(na + 1, 5))
    with pytest.raises(ValueError, match="shape"):
        engine.tertiary_volume(va, dev([np.pad(b, ((0, 1), (0, 0), (0, 0)))]))
    with pytest.raises(ValueError, match="uint16"):
        engine.tertiary_volume(va[0], vb[0])


# ------------------------------------------------------------------------------------------------ the tertiary volume
def tertiary_cases():
    cases = dict(ref.tertiary_scenes())
    a, b = ref.worked()
    cases["worked"] = (b, a)
    return cases


@pytest.mark.parametrize("shrink", [True, False])
@pytest.mark.parametrize("name", list(tertiary_cases()))
def test_tertiary_volume_is_exact(engine, name, shrink):
    import torch

    outer, inner = tertiary_cases()[name]
    zeros = np.zeros_like(outer)
    vo, vi = dev([outer, zeros, outer, inner]), dev([inner, inner, zeros, outer])
    got = engine.tertiary_volume(vo, vi, shrink_inner=shrink)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint16 and got.shape == vo.shape
    planes = engine.tertiary_labels(vo.view(-1, *vo.shape[2:]), vi.view(-1, *vi.shape[2:]), shrink_inner=shrink)  # per plane
    assert torch.equal(got.view(torch.int16), planes.view(got.shape).view(torch.int16))
    got = got.cpu().numpy()
    assert np.array_equal(got[0], ref.tertiary(outer, inner, shrink))
    assert not got[1].any() and np.array_equal(got[2], outer)
    assert np.array_equal(got[3], ref.tertiary(inner, outer, shrink))
    if name == "worked":
        assert (int((got[0] == 1).sum()), int((got[0] == 2).sum())) == ref.WORKED_TERTIARY_VOLUMES[shrink]
    if name == "covered":
        assert not (got[0] == 2).any()


@pytest.mark.parametrize("shrink", [True, False])
def test_tertiary_volume_odd_width_batch(engine, shrink):
    """[2,5,33,47]: a width that is no multiple of eight takes the scalar form of the 2-D kernel."""
    import torch

    pairs = [random_stack((5, 33, 47), 9, 14, seed) for seed in (21, 22)]
    vo, vi = dev([p[1] for p in pairs]), dev([p[0] for p in pairs])
    got = engine.tertiary_volume(vo, vi, shrink_inner=shrink)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    for f, (nuclei, cells) in enumerate(pairs):
        assert np.array_equal(got[f], ref.tertiary(cells, nuclei, shrink)), f
        for z in range(5):
            assert np.array_equal(got[f, z], ref2.tertiary(cells[z], nuclei[z], shrink)), (f, z)


def test_host_array_conveniences(engine):
    from aliby_amd.extraction import features, functions

    assert features.relate3d_names("cell") == features.relate_names("cell") == ref.names("cell")
    a, b, na, nb = ref.scenes()["worked"]
    rows_a, rows_b = functions.relate_objects_3d(a, b)
    wa, wb = want("worked", a, b, na, nb)
    compare(rows_a, wa, "relate_objects_3d A"), compare(rows_b, wb, "relate_objects_3d B")
    rows_a, _ = functions.relate_objects_3d(a, b, spacing=(2.5, 1.0, 1.0))
    compare(rows_a, want(("worked", (2.5, 1.0, 1.0)), a, b, na, nb, (2.5, 1.0, 1.0))[0], "relate_objects_3d A, spacing")
    cyto = functions.tertiary_objects_3d(b, a)
    assert cyto.dtype == np.uint16 and np.array_equal(cyto, ref.tertiary(b, a, True))
    assert np.array_equal(functions.tertiary_objects_3d(b, a, shrink_inner=False), ref.tertiary(b, a, False))
    with pytest.raises(ValueError):
        functions.relate_objects_3d(a, b[:-1])
    with pytest.raises(ValueError):
        functions.tertiary_objects_3d(a[0], b[0])
