"""
CPU: pins tests/cell_ref.py — the exact reference tests/test_gpu_cell.py compares the per-cell metric kernels with — to
oracle/cell_metrics.py (itself pinned to the reference module by tests/golden) and to closed forms, and checks the stated
precondition of every input built there: the ladder's areas and boxes, the launch and sort form every case lands in, the object
counts, the uint16 wrap of total_squared, and the margin that keeps both axis roundings away from a tie.

The oracle takes one full-frame mask per object.  It is called on the frame cut behind the object's last row and column (the
origin stays): what is cut holds no pixel of the object, and the ring the oracle pads with stands where the nearest such pixel
stood, so no value changes — test_the_oracle_on_a_cut_frame_is_the_oracle_on_the_whole_frame checks that, thin objects included.
"""
import math
import warnings

import numpy as np
import pytest

from oracle import cell_metrics as cm
from tests import cell_ref as ref

C = ref.COL
INTEGER_VALUED = ("area", "min_ax", "maj_ax", "median", "total", "total_squared")
DTYPES = ("u16", "f32")


def _oracle_row(lab, plane, L, cut=True, mask_columns=True):
    """The oracle's 17 columns for label L (NaN where it has no pixels to work on)."""
    mask = lab == L
    if cut and mask.any():
        ys, xs = np.nonzero(mask)
        mask = mask[: ys.max() + 1, : xs.max() + 1]
        plane = None if plane is None else plane[: ys.max() + 1, : xs.max() + 1]
    row = np.full(len(ref.COLUMNS), np.nan)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if mask_columns:
            for name in ("area", "centroid_x", "centroid_y", "conical_volume", "eccentricity", "spherical_volume", "volume"):
                row[C[name]] = cm.ONE_ARG[name](mask)
            row[C["min_ax"]], row[C["maj_ax"]] = cm.min_maj_approximation(mask)
        if plane is not None:
            for name in ref.COLUMNS[ref.N_MASK:]:
                row[C[name]] = cm.TWO_ARG[name](mask, plane)
    return row


def _compare_with_oracle(case, dtype, what):
    labels, planes, ch, want = case["labels"], case["planes"], case["channel"], case["want"]
    rows = []
    u16 = dtype == "u16"  # the float inputs have the same labels: their mask columns are those of the uint16 run, bit for bit
    for f, n in enumerate(case["counts"]):
        rows += [_oracle_row(labels[f], planes[f, ch], L, mask_columns=u16) for L in range(1, n + 1)]
    got = np.asarray(rows).reshape(len(want), len(ref.COLUMNS))
    if not u16:
        assert np.array_equal(want[:, :ref.N_MASK], ref.case(what, "u16")["want"][:, :ref.N_MASK], equal_nan=True)
    for name in ref.COLUMNS[0 if u16 else ref.N_MASK:]:
        g, w = got[:, C[name]], want[:, C[name]]
        loose = dtype != "u16" and C[name] >= ref.N_MASK
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, name, np.flatnonzero(np.isnan(g) != np.isnan(w))[:5])
        if name in INTEGER_VALUED and not loose:
            assert np.array_equal(g, w, equal_nan=True), (what, name)
        else:
            # float32 pixels: NumPy accumulates them in float32, the only reason for the project's 1e-4 here
            assert np.allclose(g, w, rtol=1e-4 if loose else 1e-12, atol=0.0, equal_nan=True), (what, name, np.nanmax(np.abs(g - w) / np.abs(w)))


# ------------------------------------------------------------------------------------------------ 1. the reference and the oracle
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ref.CASES)
def test_reference_matches_the_oracle_on_every_input(name, dtype):
    case = ref.case(name, dtype)
    assert len(case["want"]) == sum(case["counts"]) == len(case["meta"])
    _compare_with_oracle(case, dtype, name)


def test_the_oracle_on_a_cut_frame_is_the_oracle_on_the_whole_frame():
    for name in ("sparse_ids", "two_tiles"):
        case = ref.case(name)
        lab, plane = case["labels"][0], case["planes"][0, case["channel"]]
        for L in range(1, case["counts"][0] + 1):
            cut, whole = _oracle_row(lab, plane, L, cut=True), _oracle_row(lab, plane, L, cut=False)
            assert np.array_equal(cut[:ref.N_MASK], whole[:ref.N_MASK], equal_nan=True), (name, L)
            # (NumPy's pairwise sums split another array shape at other places)
            assert np.allclose(cut[ref.N_MASK:], whole[ref.N_MASK:], rtol=1e-12, atol=0.0, equal_nan=True), (name, L)
    meta = ref.case("sparse_ids")["meta"]
    assert meta[3]["all_top"] and meta[8]["all_top"] and not meta[0]["all_top"]  # the thin objects took scipy's no-background answer


def test_absent_labels_have_zero_axes_and_volume_in_the_oracle():
    case = ref.case("sparse_ids")
    present = [m["n"] > 0 for m in case["meta"]]
    assert present == [True, False, False, True, False, False, False, False, True]
    row = _oracle_row(case["labels"][0], case["planes"][0, 0], 2)
    for name in ("area", "volume", "min_ax", "maj_ax", "conical_volume", "spherical_volume", "total", "total_squared"):
        assert row[C[name]] == 0.0 and case["want"][1, C[name]] == 0.0, name
    for name in ("eccentricity", "centroid_x", "centroid_y", "mean", "median", "std", "max2p5pc", "max5px_median", "moment_of_inertia"):
        assert np.isnan(case["want"][1, C[name]]), name


@pytest.mark.parametrize("dtype", ("u16", "f32", "f32_signed"))
def test_ratio_and_trap_references_match_the_oracle(dtype):
    rtol = 1e-12 if dtype == "u16" else 1e-4
    lab, px = ref.ratio_case(dtype)
    n = int(lab.max())
    assert n == len(ref.RATIO_OBJECTS)
    areas = np.bincount(lab.ravel())[1:]
    assert areas.tolist() == [1, 2, 35, 36, 20, 21, 45]
    for c0, c1 in ((0, 2), (2, 0)):
        want = ref.ratio(lab[0], px[0, c0], px[0, c1], n)
        with np.errstate(all="ignore"):
            got = [cm.ratio(lab[0] == L, np.stack([px[0, c0], px[0, c1]], -1)) for L in range(1, n + 1)]
        assert np.allclose(got, want, rtol=rtol, atol=0.0, equal_nan=True), (dtype, c0, c1)
        nan = np.flatnonzero(np.isnan(want)) + 1
        # one zero denominator makes its own object NaN and no other; a -0.0 is a zero; a numerator's zero becomes one in (2, 0)
        assert nan.tolist() == ([5] if c1 == 2 else ([6, 7] if dtype == "f32_signed" else [6])), (dtype, c0, c1, nan)
        assert (want[~np.isnan(want)] != 0).all()  # no median lies on a signed zero, whose bits no sort defines
        assert int((px[0, c1][lab[0] == nan[0]] == 0).sum()) == 1
    if dtype == "f32_signed":
        num = px[0, 0][lab[0] == 7]
        assert (num < 0).any() and np.signbit(num[num == 0]).tolist() == [False, True] and np.signbit(px[0, 2][lab[0] == 5]).any()
        assert len(np.unique(px[0, 0][lab[0] == 4])) < 36  # exact duplicates
    labels, planes, ch = ref.trap_case(dtype)
    assert tuple(int((t == 0).sum()) for t in labels) == ref.TRAP_BACKGROUND_COUNTS == (0, 1, 4, 5, 6, 40, 77) and ch == 1
    for f in range(len(labels)):
        med, top = ref.trap_background(labels[f], planes[f, ch])
        masks = (labels[f] > 0)[..., None]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            o_med, o_top = cm.imBackground(masks, planes[f, ch]), cm.background_max5(masks, planes[f, ch])
        assert np.allclose([med, top], [o_med, o_top], rtol=rtol, atol=0.0, equal_nan=True), (dtype, f)
        bg = np.sort(planes[f, ch][labels[f] == 0])
        if len(bg) >= 40:
            k = len(bg)
            assert bg[k // 2 - 1] == bg[k // 2] == bg[k // 2 + 1] and bg[-1] == bg[-2] and bg[-6] == bg[-5] and med != 0
            if dtype == "f32_signed":
                zeros = planes[f, ch][labels[f] == 0]  # (unsorted: a vectorised sort may hand back either zero for both)
                zeros = zeros[zeros == 0]
                assert (bg < 0).sum() == 10 and np.signbit(zeros).any() and not np.signbit(zeros).all() and med > 0
    assert math.isnan(ref.trap_background(labels[0], planes[0, ch])[0])


# ------------------------------------------------------------------------------------------------ 2. closed forms
@pytest.mark.parametrize("r,c", [(1, 1), (1, 7), (2, 9), (5, 5), (6, 11), (9, 4), (12, 12)])
def test_rectangle_closed_forms(r, c):
    lab = np.zeros((r + 5, c + 7), np.uint16)
    lab[3:3 + r, 4:4 + c] = 1
    want, meta = ref.cell_metrics(lab, None, 1)
    # the distance of pixel (i, j) to the outside of an r x c rectangle is min(i + 1, r - i, j + 1, c - j)
    depth = [min(i + 1, r - i, j + 1, c - j) for i in range(r) for j in range(c)]
    assert want[0, C["min_ax"]] == float(round(max(depth))) == (min(r, c) + 1) // 2
    assert want[0, C["conical_volume"]] == 4.0 * sum(depth)
    assert want[0, C["area"]] == r * c and want[0, C["centroid_x"]] == 4 + (c + 1) / 2 and want[0, C["centroid_y"]] == 3 + (r + 1) / 2
    assert meta[0]["all_top"] == (min(r, c) <= 2)
    assert np.isnan(want[0, ref.N_MASK:]).all()  # no plane: nothing from the pixels


@pytest.mark.parametrize("n,n_top", [(40, 1), (41, 2), (80, 2)])
def test_constant_plane_and_the_size_of_the_top_list(n, n_top):
    lab = np.zeros((6, 50), np.uint16)
    flat = np.zeros(2 * 40, np.uint16)
    flat[:n] = 1
    lab[1:3, 2:42] = flat.reshape(2, 40)
    assert int((lab == 1).sum()) == n and n_top == math.ceil(0.025 * n)
    for const in (np.uint16(40000), np.float32(0.3)):
        plane = np.full(lab.shape, const)
        want, meta = ref.cell_metrics(lab, plane, 1)
        assert want[0, C["std"]] == 0.0 and want[0, C["max2p5pc"]] == float(const) == want[0, C["mean"]] == want[0, C["median"]]
        assert want[0, C["max5px_median"]] == 1.0 and meta[0]["n_top"] == n_top
    ramp = np.zeros(lab.shape, np.uint16)
    ramp[lab == 1] = np.arange(1, n + 1)
    want, _ = ref.cell_metrics(lab, ramp, 1)
    assert want[0, C["max2p5pc"]] == sum(range(n - n_top + 1, n + 1)) / n_top
    assert want[0, C["total_squared"]] == sum(k * k for k in range(1, n + 1))  # below 256: nothing wraps


# ------------------------------------------------------------------------------------------------ 3. preconditions of the inputs
def _forms(name):
    case = ref.case(name)
    max_h, max_w, max_area, who = ref.table_limits(case["labels"], case["counts"])
    return case, (max_h, max_w, max_area), who, ref.launch_form(max_h, max_w, max_area)


@pytest.mark.parametrize("block", (64, 128, 256))
def test_the_ladder_lands_on_every_sort_form(block):
    case, (max_h, max_w, max_area), _, form = _forms(f"ladder{block}")
    meta = case["meta"]
    assert tuple(m["n"] for m in meta[:16]) == ref.LADDER_AREAS == (1, 2, 5, 6, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)
    assert all(m["box"][0] * m["box"][1] <= 2048 and m["box"][0] <= 32 and m["box"][1] <= 64 for m in meta[:16])
    assert form == ("lds", block) and max_area == 2048
    if block == 64:
        assert len(meta) == 16 and max_h * max_w <= 2048
        forms = [ref.sort_form(64, m["n"]) for m in meta]
        assert forms == (["one wave, padded in registers"] * 6 + ["one wave, 128 in registers"] * 2 + ["one wave, 256 in registers"] * 2
                         + ["one wave, 512 in registers"] * 2 + ["one wave, two register halves and an LDS merge"] * 2
                         + ["one wave, generic loop"] * 2)
    else:
        side = ref.SPARSE_BOX[block]
        assert len(meta) == 17 and meta[16]["box"] == (side, side) and meta[16]["n"] <= 2048 and (max_h, max_w) == (side, side)
        assert (2048 < side * side <= 8192) if block == 128 else side * side > 8192
        assert {ref.sort_form(block, m["n"]) for m in meta} == {"several waves, generic loop"}
        assert np.array_equal(case["labels"][0] * (case["labels"][0] <= 16), ref.case("ladder64")["labels"][0])  # the ladder stays
        for dtype in DTYPES:
            assert np.array_equal(ref.case(f"ladder{block}", dtype)["want"][:16], ref.case("ladder64", dtype)["want"], equal_nan=True)


def test_the_ladder_pixels():
    case = ref.case("ladder64")
    lab, px, want, meta = case["labels"][0], case["planes"][0, 0], case["want"], case["meta"]
    assert px.min() == 0 and px.max() == 65535 and px.dtype == np.uint16
    zero_median = [m["n"] for m, w in zip(meta, want) if w[C["median"]] == 0]
    assert zero_median == [ref.ZERO_MEDIAN_AREA] and np.isnan(want[10, C["max5px_median"]]) and want[10, C["total"]] > 0
    for k, m in enumerate(meta):
        v = np.sort(px[lab == k + 1])
        if m["n"] >= 63:
            n = m["n"]
            assert v[n // 2 - 1] == v[n // 2] == v[n // 2 + 1] and v[-1] == v[-2] and v[-6] == v[-5], n
        if m["n"] > 2:
            assert m["true_sq"] != want[k, C["total_squared"]]  # the uint16 square wrapped
    assert want[:, C["total"]].max() < 2 ** 53
    f32 = ref.case("ladder64", "f32")["planes"]
    assert f32.dtype == np.float32 and f32.min() == 0.0 and f32.max() == 1.0


def test_the_global_cases_take_the_global_form():
    case, (max_h, max_w, max_area), who, form = _forms("global_scratch")
    assert form == ("global", 256) and len({w for w in who}) == 3 and (0, 1) not in who  # three different objects, none the band
    assert case["meta"][0]["box"] == (128, 128) and 1800 <= case["meta"][0]["n"] <= 2200
    assert ref.launch_form(128, 128, 64) == ("global", 256) and ref.launch_form(125, 125, 64)[0] == "lds"  # the band's box alone
    assert case["channel"] == 1 and case["planes"].shape[1] == 2
    case, _, _, form = _forms("global_stride")
    assert form == ("global", 256) and len(case["meta"]) == 621 > 512 and all(m["n"] > 0 for m in case["meta"])
    boxes = {m["box"] for m in case["meta"][1:]}
    assert boxes == {(h, w) for h in (3, 4, 5) for w in (3, 4, 5)}
    assert case["labels"].shape == (1, 160, 640)


def test_the_small_cases():
    case, _, _, form = _forms("sparse_ids")
    lab = case["labels"][0]
    assert form == ("lds", 64) and sorted(set(np.unique(lab)) - {0}) == [1, 4, 9] and case["counts"] == [9]
    cross = lab == 1
    assert cross[0].any() and cross[-1].any() and cross[:, 0].any() and cross[:, -1].any()
    assert case["meta"][3]["n"] == 1 and case["meta"][8]["n"] == 4 and case["meta"][8]["box"] == (2, 2)
    case, _, _, form = _forms("two_tiles")
    assert form == ("lds", 64) and case["labels"].shape[0] == 2 and case["planes"].shape[1] == 3 and case["channel"] == 2
    assert case["counts"] == [4, 0] and not case["labels"][1].any()
    lab, px = ref.ratio_limit_case()
    assert int((lab == 1).sum()) == 16384 and int((lab == 2).sum()) == 9


# ------------------------------------------------------------------------------------------------ 4. no rounding near a tie
@pytest.mark.parametrize("name", ref.CASES)
def test_both_axes_round_far_from_a_tie(name):
    """Every present object of every input: max dn + sum cone_top / 2 and sqrt(max d2) stay 1e-6 away from a half-integer, so a
    different summation order on the GPU can never flip min_ax, maj_ax, volume or eccentricity.  No object is exempt."""
    meta = ref.case(name)["meta"]
    worst = min((m["tie"], m["sqrt_tie"]) for m in meta if m["n"])
    print(f"[{name}] nearest to a half-integer: major {min(m['tie'] for m in meta if m['n']):.3e}, sqrt {min(m['sqrt_tie'] for m in meta if m['n']):.3e}")
    for k, m in enumerate(meta):
        if m["n"]:
            assert m["tie"] >= ref.TIE_MARGIN and m["sqrt_tie"] >= ref.TIE_MARGIN, (name, k + 1, m["major"], worst)
