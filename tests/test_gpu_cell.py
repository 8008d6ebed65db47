"""
GPU parity of the reference's in-repo metrics: `FeatureEngine.cell_metrics` (aliby_amd/csrc/feat_cell.hip, k_cell), `cell_ratio` and
`trap_background` (aliby_amd/csrc/feat_extra.hip), column by column in every launch form, against the exact reference
tests/cell_ref.py (pinned to oracle/cell_metrics.py and to closed forms by tests/test_cpu_cell_ref.py, which also checks the stated
precondition of every input used here: the areas on the boundaries of the six sort forms, the launch form of every case, and the
margin that keeps both axis roundings away from a tie).

Rule (tests/cell_ref.check): area, both centroids, min_ax, maj_ax and median bit for bit; with uint16 pixels also total,
total_squared, mean, max2p5pc and max5px_median; conical_volume, std and moment_of_inertia (and, with float32 pixels, the five
columns above) within 4 N 2^-53 relative, floor 1e-13; volume, eccentricity and spherical_volume within 1e-14.  Rows of absent
labels are compared with the reference like any other row.  Every comparison prints the worst relative error of each column.
"""
import numpy as np
import pytest

from tests import cell_ref as ref

pytestmark = pytest.mark.gpu

C = ref.COL
DTYPES = ("u16", "f32")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    """Equal bit for bit, NaN in the same places (whatever the NaN's payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _device(labels, planes):
    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    dl = to_device_u16(np.ascontiguousarray(labels))
    dp, dt = to_device_planes(np.ascontiguousarray(planes))
    return dl, dp, dt


def _run(engine, case, pixels=True):
    """-> (float64 [n, 17] from the GPU, the object table); the table's limits are those the launch form was worked out from."""
    dl, dp, dt = _device(case["labels"], case["planes"])
    tab = engine.object_table(dl)
    assert tab.n_obj == sum(case["counts"])
    assert (tab.max_h, tab.max_w, tab.max_area) == ref.table_limits(case["labels"], case["counts"])[:3]
    out = engine.cell_metrics(dl, dp if pixels else None, dt, case["channel"], tab)
    assert tuple(out.shape) == (tab.n_obj, 17)
    return out.cpu().numpy(), tab


def _form(tab):
    return ref.launch_form(tab.max_h, tab.max_w, tab.max_area)


def _dirty_the_scratch(engine):
    """An unrelated call that leaves other bytes in the context scratch the global form carves its work space from."""
    import torch

    from tests.sizeshape3d_ref import random_labels

    vol, _ = random_labels(99, (6, 40, 44))
    engine.sizeshape3d(torch.from_numpy(vol[None]).cuda(), [int(vol.max())])


# ------------------------------------------------------------------------------------------------ 1. the six sort forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_area_ladder_in_the_three_lds_launches(engine, dtype):
    """Areas 1 .. 2048 on the boundaries of the sort forms, in a 64-thread launch (padded, 128 / 256 / 512 in registers, two halves
    and a merge, the generic loop in one wave) and, beside a 90 x 90 or 100 x 100 band, in the 128- and 256-thread launches (the
    generic loop in several waves).  The ladder's rows do not depend on the launch."""
    rows = {}
    for block in (64, 128, 256):
        case = ref.case(f"ladder{block}", dtype)
        got, tab = _run(engine, case)
        assert _form(tab) == ("lds", block)
        ref.check(got, case["want"], case["meta"], f"ladder, {block} threads", dtype)
        rows[block] = got[:16]
    exact = ref.EXACT_BOTH + (ref.EXACT_U16 if dtype == "u16" else ())
    for block in (128, 256):
        for name in exact:
            assert _same_bits(rows[block][:, C[name]], rows[64][:, C[name]]), (block, name)
        # the rest: each launch is within the rule of the one reference, so they are within twice the rule of each other
        assert np.allclose(rows[block], rows[64], rtol=2e-12, atol=0.0, equal_nan=True), block


# ------------------------------------------------------------------------------------------------ 2. the global form
@pytest.mark.parametrize("dtype", DTYPES)
def test_global_scratch_with_limits_from_three_objects(engine, dtype):
    case = ref.case("global_scratch", dtype)
    _dirty_the_scratch(engine)
    got, tab = _run(engine, case)
    assert _form(tab) == ("global", 256)
    ref.check(got, case["want"], case["meta"], "global scratch", dtype)
    mask_only, _ = _run(engine, case, pixels=False)
    ref.check(mask_only, case["want"], case["meta"], "global scratch, mask only", dtype, pixels=False)
    assert np.isnan(mask_only[:, ref.N_MASK:]).all()  # nothing of the pixel columns is written


def test_global_scratch_with_more_objects_than_workgroups(engine):
    case = ref.case("global_stride")
    _dirty_the_scratch(engine)
    got, tab = _run(engine, case)
    assert _form(tab) == ("global", 256) and tab.n_obj == 621
    ref.check(got, case["want"], case["meta"], "global stride")
    again, _ = _run(engine, case)
    assert _same_bits(again, got)


# ------------------------------------------------------------------------------------------------ 3. sparse ids and batches
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("sparse_ids", "two_tiles"))
def test_sparse_ids_and_batches(engine, name, dtype):
    """Labels 1, 4 and 9 of 1..9 (one touching all four borders, one pixel, 2 x 2); two tiles with the second empty and channel 2
    of three read.  The rows of absent labels hold what the reference module returns for an all-False mask: 0 for the sums, both
    axes and the volume, NaN for the quotients."""
    case = ref.case(name, dtype)
    got, tab = _run(engine, case)
    assert _form(tab) == ("lds", 64)
    ref.check(got, case["want"], case["meta"], name, dtype)
    mask_only, _ = _run(engine, case, pixels=False)
    ref.check(mask_only, case["want"], case["meta"], f"{name}, mask only", dtype, pixels=False)
    present = np.asarray([m["n"] > 0 for m in case["meta"]])
    assert np.isnan(mask_only[present][:, ref.N_MASK:]).all()
    if name == "sparse_ids":
        absent = got[~present]
        assert len(absent) == 6
        for col in ("area", "volume", "min_ax", "maj_ax", "conical_volume", "spherical_volume", "total", "total_squared"):
            assert (absent[:, C[col]] == 0.0).all(), col
        assert np.isnan(absent[:, C["eccentricity"]]).all()
    else:
        other = dict(case, channel=0)
        got0, _ = _run(engine, other)
        assert not np.array_equal(got0[:, C["total"]], got[:, C["total"]])  # the channel is read


# ------------------------------------------------------------------------------------------------ 4. placement
@pytest.mark.parametrize("dtype", DTYPES)
def test_only_the_17_columns_are_written(engine, dtype):
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    case = ref.case("sparse_ids", dtype)
    dl, dp, dt = _device(case["labels"], case["planes"])
    tab = engine.object_table(dl)
    n, ld, col0, fill = tab.n_obj, 26, 5, -123.25
    F, Y, X = case["labels"].shape
    present = np.asarray([m["n"] > 0 for m in case["meta"]])
    for planes in (dp, None):
        out = torch.full((n + 2, ld), fill, dtype=torch.float64, device="cuda")  # two rows more than are written
        _lib.check(engine.lib.aliby_features_cell(engine.ctx.handle, _ptr(dl), _ptr(planes), dt, F, dp.shape[1], Y, X, case["channel"], _ptr(tab.dev),
                                                  n, tab.max_h, tab.max_w, tab.max_area, _ptr(out), ld, col0, _stream_ptr()))
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        block = np.ascontiguousarray(host[:n, col0:col0 + 17])
        if planes is None:
            # a mask-only call leaves columns 9..16 of present objects untouched (an absent label's row is written whole)
            assert (block[present][:, ref.N_MASK:] == fill).all()
            block[present, ref.N_MASK:] = case["want"][present, ref.N_MASK:]
        ref.check(block, case["want"], case["meta"], f"col0 = {col0} of {ld}, {'pixels' if planes is not None else 'mask only'}", dtype)
        host[:n, col0:col0 + 17] = fill
        assert (host == fill).all()


# ------------------------------------------------------------------------------------------------ 5. cell.ratio
@pytest.mark.parametrize("dtype", ("u16", "f32", "f32_signed"))
def test_cell_ratio_bit_for_bit(engine, dtype):
    """Areas 1, 2, 35, 36 and 45; one zero (a -0.0 in the signed variant) in the denominator of one object makes that object NaN and
    no other; channel pairs (0, 2) and (2, 0) of three."""
    lab, px = ref.ratio_case(dtype)
    dl, dp, dt = _device(lab, px)
    tab = engine.object_table(dl)
    n = tab.n_obj
    assert n == len(ref.RATIO_OBJECTS)
    for c0, c1 in ((0, 2), (2, 0)):
        got = engine.cell_ratio(dl, dp, dt, c0, c1, tab).cpu().numpy()
        want = ref.ratio(lab[0], px[0, c0], px[0, c1], n)
        assert np.isnan(want).sum() in (1, 2) and np.isnan(want[4 if c1 == 2 else 5])
        assert _same_bits(got, want), (dtype, c0, c1, got, want)


def test_cell_ratio_at_its_area_limit(engine):
    """16384 pixels are the most the kernel sorts in LDS: computed; a table that announces 16385 is refused, with its message."""
    from aliby_amd import _lib

    lab, px = ref.ratio_limit_case()
    dl, dp, dt = _device(lab, px)
    tab = engine.object_table(dl)
    assert tab.max_area == 16384 and tab.n_obj == 2
    got = engine.cell_ratio(dl, dp, dt, 0, 1, tab).cpu().numpy()
    assert _same_bits(got, ref.ratio(lab[0], px[0, 0], px[0, 1], 2)), got
    big = type(tab).__new__(type(tab))
    big.__dict__.update(tab.__dict__)
    big.max_area = 16385
    with pytest.raises(_lib.AlibyHipError, match=r"cell\.ratio: an object of 16385 pixels does not fit"):
        engine.cell_ratio(dl, dp, dt, 0, 1, big)


# ------------------------------------------------------------------------------------------------ 6. the trap metrics
@pytest.mark.parametrize("dtype", ("u16", "f32", "f32_signed"))
def test_trap_background_in_one_batch(engine, dtype):
    """Tiles with 0, 1, 4, 5, 6, 40 and 77 pixels under no label in one launch, channel 1 of two read; duplicates at the median and
    among the five largest, and (signed variant) negatives and both zeros.  The median bit for bit; the mean of the five largest
    bit for bit for uint16 (an exact sum, one division) and within 5 x 2^-53 for float32 (five additions and the division)."""
    labels, planes, ch = ref.trap_case(dtype)
    dl, dp, dt = _device(labels, planes)
    got = engine.trap_background(dl, dp, dt, ch).cpu().numpy()
    assert got.shape == (len(labels), 2)
    want = np.asarray([ref.trap_background(labels[f], planes[f, ch]) for f in range(len(labels))])
    assert np.isnan(want[0]).all() and np.isfinite(want[1:]).all()
    assert _same_bits(got[:, 0], want[:, 0]), (dtype, got[:, 0], want[:, 0])
    if dtype == "u16":
        assert _same_bits(got[:, 1], want[:, 1]), (got[:, 1], want[:, 1])
    else:
        assert np.isnan(got[0, 1])
        rel = np.abs(got[1:, 1] - want[1:, 1]) / np.abs(want[1:, 1])
        print(f"[trap {dtype}] worst relative error of max5: {rel.max():.2e}")
        assert (rel <= 5 * 2.0 ** -53).all(), (got[:, 1], want[:, 1])
    other = engine.trap_background(dl, dp, dt, 0).cpu().numpy()
    assert not np.array_equal(other[1:], got[1:])  # the channel is read
