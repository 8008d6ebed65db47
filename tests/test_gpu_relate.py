"""
The `relate` family and the tertiary image on the GPU (aliby_amd/csrc/feat_relate.hip) against tests/relate_ref.py, the NumPy
restatement that tests/test_cpu_relate_ref.py pins to hand values and to np.bincount / scipy.ndimage: the engine calls, the C entry
with a NULL output, and the host-array conveniences.  Parity with CellProfiler is unpinned (it cannot be run here).

Pass bar: Parent, ParentOverlap and the children count (columns 0-2) and the NaN pattern equal to the restatement exactly; the two
distances (columns 3-4) under rtol = atol = 1e-12.  Each is fewer than ten float64 operations rounded to at most 1 ulp each, about
10 x 2^-52 = 2e-15, so the rule leaves three orders of margin, and it is never looser than the project's 1e-4 / 1e-9.  Every
comparison prints its largest difference first.  Tertiary images are exact.  Measured on an MI355X: see `compare`.
"""
import numpy as np
import pytest

from tests import relate_ref as ref

pytestmark = pytest.mark.gpu

_REF = {}


def want(key, a, b, na=None, nb=None):
    """The restatement of a scene, computed once."""
    if key not in _REF:
        _REF[key] = ref.relate(a, b, na, nb)
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


def tables(engine, tiles_a, tiles_b, counts_a=None, counts_b=None):
    from aliby_amd.extraction.engine import to_device_u16

    la, lb = to_device_u16(np.stack(tiles_a)), to_device_u16(np.stack(tiles_b))
    return la, engine.object_table(la, max_labels=counts_a), lb, engine.object_table(lb, max_labels=counts_b)


def run(engine, tiles_a, tiles_b, counts_a=None, counts_b=None):
    """-> (rows of A, rows of B) through windows of wider matrices: only columns col0 .. col0 + 4 may be written."""
    import torch

    la, ta, lb, tb = tables(engine, tiles_a, tiles_b, counts_a, counts_b)
    out_a, out_b = engine.new_output(ta.n_obj, 8), engine.new_output(tb.n_obj, 7)
    got_a, got_b = engine.relate(la, ta, lb, tb, out_a=out_a, col0_a=2, out_b=out_b, col0_b=1)
    torch.cuda.synchronize()
    assert tuple(got_a.shape) == (ta.n_obj, 5) and tuple(got_b.shape) == (tb.n_obj, 5)
    full_a, full_b = out_a.cpu().numpy(), out_b.cpu().numpy()
    assert np.isnan(full_a[:, :2]).all() and np.isnan(full_a[:, 7:]).all() and np.isnan(full_b[:, :1]).all() and np.isnan(full_b[:, 6:]).all()
    return full_a[:, 2:7].copy(), full_b[:, 1:6].copy()


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("name", list(ref.scenes()))
def test_scenes(engine, name):
    """The worked example, a child without a parent, a child whose box contains other children, absent labels in both sets (the last
    label included), objects on all four frame borders."""
    a, b, na, nb = ref.scenes()[name]
    got_a, got_b = run(engine, [a], [b], [na], [nb])
    wa, wb = want(name, a, b, na, nb)
    compare(got_a, wa, f"{name} A"), compare(got_b, wb, f"{name} B")
    if name == "worked":
        assert np.array_equal(got_a[:, :3], ref.WORKED_NUCLEI[:, :3]) and np.array_equal(got_b[:, :3], ref.WORKED_CELLS)
        assert np.allclose(got_a[:, 3:], ref.WORKED_NUCLEI[:, 3:], rtol=ref.RTOL, atol=ref.ATOL)
    if name == "orphan":
        assert got_a[1, :3].tolist() == [0, 0, 0] and np.isnan(got_a[1, 3:]).all()


def test_strip_across_257_parents(engine):
    a, b = ref.strip()
    got_a, got_b = run(engine, [a], [b])
    wa, wb = want("strip", a, b)
    compare(got_a, wa, "strip A"), compare(got_b, wb, "strip B")
    assert got_a[:, :2].tolist() == [[258, 21], [1, 1]] and got_a[:, 2].tolist() == [259, 0]


def test_batch_of_three_with_an_empty_tile_and_an_empty_set(engine):
    tiles_a, tiles_b, ca, cb = ref.batch3()
    got_a, got_b = run(engine, tiles_a, tiles_b, ca, cb)
    wa = np.concatenate([want(("batch3", f), tiles_a[f], tiles_b[f], ca[f], cb[f])[0] for f in range(3)])
    wb = np.concatenate([want(("batch3", f), tiles_a[f], tiles_b[f], ca[f], cb[f])[1] for f in range(3)])
    assert len(wa) == 5 and len(wb) == 2
    compare(got_a, wa, "batch3 A"), compare(got_b, wb, "batch3 B")
    assert got_a[3:, :3].tolist() == [[0, 0, 0]] * 2 and np.isnan(got_a[3:, 3:]).all()  # present children, no object in B


def test_a_set_with_zero_objects(engine):
    a, _ = ref.worked()
    zeros = np.zeros_like(a)
    got_a, got_b = run(engine, [a], [zeros])
    assert got_b.shape == (0, 5) and got_a[:, :3].tolist() == [[0, 0, 0]] * 3 and np.isnan(got_a[:, 3:]).all()
    got_a, got_b = run(engine, [zeros], [a])
    assert got_a.shape == (0, 5) and got_b[:, :3].tolist() == [[0, 0, 0]] * 3 and np.isnan(got_b[:, 3:]).all()
    got_a, got_b = run(engine, [zeros], [zeros])
    assert got_a.shape == (0, 5) and got_b.shape == (0, 5)


def test_65534_single_pixel_parents_take_the_scratch_form(engine):
    """One counter per label of the other set: 65 535 ints are 256 KiB, past the 32 KiB of the LDS form, so the children's workgroups
    count in the context's scratch.  The same children over only the parents they touch (a few hundred: LDS) must give the same
    bits, the parent's label aside."""
    a, many, few, old = ref.single_pixel_parents()
    got_many, rows_many = run(engine, [a], [many])
    got_few, _ = run(engine, [a], [few])
    assert got_many[3, 1] == 1 and got_many[:, 2].tolist() == [28, 9, 65, 10]  # (child 4: two of its twelve pixels have no parent)
    assert np.array_equal(got_many[:, 0], old[got_few[:, 0].astype(np.int64) - 1])
    assert np.array_equal(got_many[:, 1:].view(np.int64), got_few[:, 1:].view(np.int64))
    wa, wb = want("many", a, many)
    compare(got_many, wa, "single-pixel parents A"), compare(rows_many, wb, "single-pixel parents B")


def random_scene(shape, n_cells, n_nuclei, seed):
    rng = np.random.default_rng(seed)
    Y, X = shape

    def boxes(n, lo, hi):
        lab = np.zeros(shape, np.uint16)
        for L in range(1, n + 1):
            h, w = rng.integers(lo, hi, 2)
            y, x = rng.integers(0, Y - 2), rng.integers(0, X - 2)
            lab[y:y + h, x:x + w] = L  # (later boxes overwrite earlier ones: ragged shapes, some labels may vanish)
        return lab

    return boxes(n_nuclei, 2, 9), boxes(n_cells, 6, 25)


def test_one_tile_alone_and_in_a_batch_beside_a_large_object(engine):
    import torch

    a0, b0 = random_scene((210, 213), 30, 40, 5)
    a1, b1 = np.zeros_like(a0), np.zeros_like(b0)
    a1[3:203, 5:205] = 1  # 200 x 200: the launch picks the largest workgroup
    b1[:, :100], b1[:, 100:] = 1, 2
    la, ta, lb, tb = tables(engine, [a0], [b0], [40], [30])
    alone = engine.relate(la, ta, lb, tb)
    la2, ta2, lb2, tb2 = tables(engine, [a1, a0, a1], [b1, b0, b1], [1, 40, 1], [2, 30, 2])
    batch = engine.relate(la2, ta2, lb2, tb2)
    torch.cuda.synchronize()
    assert torch.equal(bits(alone[0]), bits(batch[0][1:41])) and torch.equal(bits(alone[1]), bits(batch[1][2:32]))
    wa, wb = want("random", a0, b0, 40, 30)
    compare(alone[0].cpu().numpy(), wa, "random A"), compare(alone[1].cpu().numpy(), wb, "random B")
    w1 = want("large", a1, b1)
    compare(batch[0][:1].cpu().numpy(), w1[0], "large A"), compare(batch[1][32:].cpu().numpy(), w1[1], "large B (second copy)")
    again = engine.relate(la2, ta2, lb2, tb2)  # run to run
    torch.cuda.synchronize()
    assert torch.equal(bits(again[0]), bits(batch[0])) and torch.equal(bits(again[1]), bits(batch[1]))


def test_differing_shapes_are_refused(engine):
    from aliby_amd.extraction.engine import to_device_u16

    a, b = ref.worked()
    la, lb = to_device_u16(a[None]), to_device_u16(np.pad(b, ((0, 1), (0, 0)))[None])
    with pytest.raises(ValueError):
        engine.relate(la, engine.object_table(la), lb, engine.object_table(lb))
    with pytest.raises(ValueError):
        engine.tertiary_labels(lb, la)


def test_c_entry_with_one_output_null(engine):
    """aliby_features_relate with out_b NULL fills the rows of A alone, children count included (it needs B's parents all the same)."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    a, b = ref.worked()
    la, ta, lb, tb = tables(engine, [a], [b])
    lib, dev = engine.lib, la.device
    work = torch.empty(int(lib.aliby_relate_workspace_bytes(ta.n_obj, tb.n_obj)) // 8, dtype=torch.float64, device=dev)
    assert int(lib.aliby_relate_workspace_bytes(3, 2)) == 88 + 56  # (28 bytes a row, each side rounded up to 8)
    out = engine.new_output(ta.n_obj, 5)
    offs = [torch.from_numpy(t.offsets.astype(np.int32)).to(dev) for t in (ta, tb)]
    args = [engine.ctx.handle, _ptr(la), _ptr(lb), 1, 6, 8, _ptr(ta.dev), ta.n_obj, ta.max_h, ta.max_w, _ptr(tb.dev), tb.n_obj, tb.max_h,
            tb.max_w, _ptr(offs[0]), 3, _ptr(offs[1]), 2, _ptr(work)]
    _lib.check(lib.aliby_features_relate(*args, _ptr(out), 5, 0, 0, 0, 0, _stream_ptr()))
    torch.cuda.synchronize()
    compare(out.cpu().numpy(), want("worked", a, b, 3, 2)[0], "C entry, out_b NULL")
    with pytest.raises(ValueError):  # columns past the row stride
        _lib.check(lib.aliby_features_relate(*args, _ptr(out), 5, 1, 0, 0, 0, _stream_ptr()))


# ------------------------------------------------------------------------------------------------ the tertiary image
def tertiary_cases():
    cases = dict(ref.tertiary_scenes())
    nuclei, cells = random_scene((67, 261), 25, 40, 11)  # one pixel per thread, several workgroups
    cases["random_w261"] = (cells, nuclei)
    nuclei, cells = random_scene((70, 264), 25, 40, 12)  # eight pixels per thread
    cases["random_w264"] = (cells, nuclei)
    return cases


@pytest.mark.parametrize("shrink", [True, False])
@pytest.mark.parametrize("name", list(tertiary_cases()))
def test_tertiary_is_exact(engine, name, shrink):
    import torch
    from aliby_amd.extraction.engine import to_device_u16

    outer, inner = tertiary_cases()[name]
    zeros = np.zeros_like(outer)
    lo, li = to_device_u16(np.stack([outer, zeros, outer, inner])), to_device_u16(np.stack([inner, inner, zeros, outer]))
    got = engine.tertiary_labels(lo, li, shrink_inner=shrink)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint16 and got.shape == lo.shape
    got = got.cpu().numpy()
    assert np.array_equal(got[0], ref.tertiary(outer, inner, shrink))
    assert not got[1].any() and np.array_equal(got[2], outer)
    assert np.array_equal(got[3], ref.tertiary(inner, outer, shrink))
    if name == "worked":
        assert (int((got[0] == 1).sum()), int((got[0] == 2).sum())) == ref.WORKED_TERTIARY_AREAS[shrink]
    if name == "three_by_three_w16":
        assert not (got[0] == 2).any()  # the cell under the large nucleus is left empty
        assert int((got[0] == 1).sum()) == (48 if shrink else 40)


def test_host_array_conveniences(engine):
    from aliby_amd.extraction import functions

    a, b = ref.worked()
    rows_a, rows_b = functions.relate_objects(a, b)
    wa, wb = want("worked", a, b, 3, 2)
    compare(rows_a, wa, "relate_objects A"), compare(rows_b, wb, "relate_objects B")
    cyto = functions.tertiary_objects(b, a)
    assert cyto.dtype == np.uint16 and np.array_equal(cyto, ref.tertiary(b, a, True))
    assert np.array_equal(functions.tertiary_objects(b, a, shrink_inner=False), ref.tertiary(b, a, False))
    with pytest.raises(ValueError):
        functions.relate_objects(a, b[:-1])
