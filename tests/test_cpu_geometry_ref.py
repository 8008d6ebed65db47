"""
The references of tests/geometry_ref.py against closed forms and against the float64 oracles (oracle/zernike_restated.py,
oracle/radial_restated.py), and the preconditions of tests/test_gpu_geometry.py: conditions on the inputs that hold for the
references alone, so that what the GPU tests compare never hangs on a rounding.  No GPU, no aliby_amd kernel.

Every label 1 .. max of every tile of every case is visited (`rows` counts them): present objects are compared, the absent labels
(8 and 15 of `small`) are compared as absent, nothing is skipped.
"""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from tests import geometry_ref as g
from tests import shape_ref

ALL_CASES = tuple(shape_ref.CASES) + tuple(g.WINDING)
RADIAL_MODES = ((4, None), (5, None), (4, 10))
N_ROWS = {"small": 2 * shape_ref.N_SMALL}


def rows(name):
    """(row, tile, label, present) of every label of every tile; asserts the count so that no object is left out"""
    lab = g.labels_of(name)
    out = [(row, t, L, bool((lab[t] == L).any())) for row, (t, L) in enumerate(g.objects_of(name))]
    assert len(out) == N_ROWS.get(name, 2 if name != "frame12x16" else 3)
    absent = [(t, L) for _, t, L, present in out if not present]
    assert absent == ([(t, L) for t in range(2) for L in shape_ref.ABSENT] if name == "small" else [])
    return out


# ---- the shapes ---------------------------------------------------------------------------------------------------------------
def test_winding_shapes_are_what_they_are_called():
    from scipy import ndimage as ndi

    for name in g.WINDING:
        lab = g.winding(name)
        assert lab.dtype == np.uint16 and np.array_equal(lab[1], lab[0][:, ::-1])
        mask, y0, x0 = g.crop(lab[0], 1)
        assert (y0, x0) == (3, 5) and lab.shape[1:] == (mask.shape[0] + 8, mask.shape[1] + 8)
        n_comp = ndi.label(mask, structure=np.ones((3, 3), int))[1]
        assert n_comp == (2 if name == "two_components" else 1), name
    assert g.crop(g.winding("serpentine31x32")[0], 1)[0].shape == (31, 32) and g.crop(g.winding("serpentine32x31")[0], 1)[0].shape == (32, 31)
    assert g.crop(g.winding("spiral33")[0], 1)[0].shape == (33, 33) and g.crop(g.winding("serpentine46x48_thick")[0], 1)[0].shape == (46, 48)
    # the small catalogue's one-pixel spiral is the same construction
    assert np.array_equal(g._square_spiral(7), np.array([[ch == "X" for ch in row] for row in shape_ref.SMALL[19][3]]))
    assert not set(g.WINDING) & set(shape_ref.CASES)


# ---- minimum enclosing circle -------------------------------------------------------------------------------------------------
def test_mec_exact_on_closed_forms():
    F = Fraction
    assert g.mec_exact([(3, 4)]) == (F(3), F(4), F(0))
    assert g.mec_exact([(0, 0), (0, 1)]) == (F(0), F(1, 2), F(1, 4))
    assert g.mec_exact([(0, 0), (0, 1), (1, 0), (1, 1)]) == (F(1, 2), F(1, 2), F(1, 2))
    assert g.mec_exact([(k, k) for k in range(7)]) == (F(3), F(3), F(18))
    # an obtuse triangle: the circle of its longest side; an acute one: its circumcircle
    assert g.mec_exact([(0, 0), (0, 10), (1, 5)]) == (F(0), F(5), F(25))
    assert g.mec_exact([(0, 0), (0, 6), (5, 3)]) == (F(8, 5), F(3), F(8, 5) ** 2 + 9)
    assert g.hull_vertices([(2, 2)]) == [(2, 2)] and len(g.hull_vertices([(k, 3) for k in range(9)])) == 2
    assert len(g.hull_vertices([(r, c) for r in range(5) for c in range(5)])) == 4


def test_certificate_accepts_the_circle_and_refuses_others():
    pts = [(0, 0), (0, 6), (5, 3), (2, 3)]
    ci, cj, r2 = g.mec_exact(pts)
    r = float(r2) ** 0.5
    assert g.mec_certificate(pts, float(ci), float(cj), r)
    assert not g.mec_certificate(pts, float(ci), float(cj), r * (1 + 1e-6))      # encloses, but rests on no point
    assert not g.mec_certificate(pts, float(ci), float(cj), r * (1 - 1e-6))      # leaves points out
    assert not g.mec_certificate(pts, float(ci) + 1e-4, float(cj), r + 1e-4)
    line = [(k, 2 * k) for k in range(5)]
    assert g.mec_certificate(line, 2.0, 4.0, 20 ** 0.5) and not g.mec_certificate(line, 2.0, 4.5, 20.5 ** 0.5)
    # three points on the circle whose triangle does NOT contain the centre prove nothing
    assert not g.mec_certificate([(0, 0), (0, 6), (-1, 3)], *[float(v) for v in g._circle3((0, 0), (0, 6), (-1, 3))[:2]],
                                 float(g._circle3((0, 0), (0, 6), (-1, 3))[2]) ** 0.5)
    assert g.mec_exact_near(pts, float(ci), float(cj), r) == (ci, cj, r2)


def test_only_the_acute_triangle_rests_on_three_pixels():
    """The support of every other circle is a pair of antipodal pixels, which a two-point circle already finds."""
    three = []
    for name in ALL_CASES + ("acute",):
        for circ in g.circles(name):
            if circ is not None and circ[0][2] > 0:
                (ci, cj, r2) = circ[0]
                if (2 * ci).denominator != 1 or (2 * cj).denominator != 1:  # no midpoint of two pixels
                    three.append(name)
    assert three == ["acute", "acute"] and g.circles("acute")[0][0] == (Fraction(18, 5), Fraction(6), Fraction(289, 25))


@pytest.mark.parametrize("name", ALL_CASES + ("acute",))
def test_exact_circle_agrees_with_the_oracle(name):
    want = g.oracle_mec(name)
    lab = g.labels_of(name)
    compared = 0
    for (row, t, L, present), circ in zip(rows(name), g.circles(name)):
        if not present:
            assert circ is None and np.isnan(want[row]).all()
            continue
        (ci, cj, r2), n_hull, enumerated = circ
        assert enumerated == (not name.startswith("arc")), (name, n_hull)
        r = float(mpmath.sqrt(mpmath.mpf(r2.numerator) / r2.denominator))
        assert abs(float(ci) - want[row, 0]) <= 1e-9 and abs(float(cj) - want[row, 1]) <= 1e-9 and abs(r - want[row, 2]) <= 1e-9 * max(r, 1.0), (name, row)
        ys, xs = np.nonzero(lab[t] == L)
        assert g.mec_certificate(list(zip(ys.tolist(), xs.tolist())), *want[row]), (name, row)
        compared += 1
    assert compared == sum(p for *_, p in rows(name))
    if name == "small":  # K of a pixel, of straight lines in every direction
        k = {L: c[1] for (_, t, L, _), c in zip(rows(name), g.circles(name)) if c and t == 0}
        assert k[1] == 1 and k[2] == k[4] == k[5] == k[6] == k[7] == 2 and k[12] == 4
    if name.startswith(("diagonal", "line")):
        assert all(c[1] == 2 for c in g.circles(name))


# ---- Zernike ------------------------------------------------------------------------------------------------------------------
def _direct(mask, y0, x0, circle, weights):
    """The moment sums as they are written down: every term rounded at 50 digits."""
    ci, cj, r2 = circle
    with mpmath.workdps(g.DIGITS):
        r = mpmath.sqrt(mpmath.mpf(r2.numerator) / r2.denominator)
        sums = [mpmath.mpc(0)] * 30
        for i, j in zip(*np.nonzero(mask)):
            y = (int(i) + y0 - mpmath.mpf(ci.numerator) / ci.denominator) / r
            x = (int(j) + x0 - mpmath.mpf(cj.numerator) / cj.denominator) / r
            rr = x * x + y * y
            if rr > 1 + mpmath.mpf(10) ** -40:
                continue
            w = 1 if weights is None else mpmath.mpf(float(weights[i, j]))
            for col, (n, m) in enumerate(g.ZERNIKE_NM):
                s = mpmath.mpf(0)
                for c in g._LUT[(n, m)]:
                    s = s * rr + c
                sums[col] += w * s * mpmath.mpc(y, x) ** m
        norm = mpmath.pi * r * r if weights is None else int(mask.sum())
        return [float(abs(v) / norm) for v in sums], [float(mpmath.atan2(v.real, v.imag)) for v in sums]


def test_exact_sums_equal_the_terms_added_at_50_digits():
    lab = shape_ref.catalogue("small")
    px = g.planes("small", "f32")
    for L in (3, 10, 14, 16, 19):
        mask, y0, x0 = g.crop(lab[1], L)
        circle = g.circles("small")[shape_ref.N_SMALL + L - 1][0]
        for w in (None, px[1, 0, y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]]):
            z = g.zernike_ref(mask, y0, x0, w)
            assert z["circle"] == circle
            mag, phase = _direct(mask, y0, x0, circle, w)
            assert np.allclose(z["mag"], mag, rtol=1e-14, atol=1e-30)
            if w is not None:
                keep = z["mag"] > 1e-12
                assert np.allclose(z["phase"][keep], np.asarray(phase)[keep], rtol=0, atol=1e-13)
            assert (z["S"] / z["normaliser"] >= z["mag"] * (1 - 1e-12)).all()
    # Z_00 = 1 on the disc: the unweighted column 0 is N / (pi r^2), every pixel being inside
    z = g.zernike_ref(*g.crop(lab[0], 12))
    assert z["mag"][0] == pytest.approx(25 / (np.pi * 8.0), rel=1e-15) and z["S"][0] == 25.0
    one = g.zernike_ref(*g.crop(lab[0], 1))
    assert np.isnan(one["mag"]).all() and one["vanishing"] == 0


def test_no_pixel_is_near_the_unit_circle_without_being_on_it():
    """Exact rho^2 of every object pixel: on the circle (== 1) or at least 1e-6 away from it, so membership of the disc is the same
    under the kernel's 1 + 1e-9 guard band and under the reference's > 1."""
    on = seen = 0
    for name in ALL_CASES:
        lab = g.labels_of(name)
        for (row, t, L, present), circ in zip(rows(name), g.circles(name)):
            if not present or circ[0][2] == 0:
                continue
            mask, y0, x0 = g.crop(lab[t], L)
            for v in g.rho2_of_pixels(mask, y0, x0, circ[0]):
                assert v == 1 or abs(v - 1) >= Fraction(1, 10 ** 6), (name, row, float(v))
                assert v <= 1  # (the circle encloses every pixel)
                on += v == 1
                seen += 1
    print(f"[unit circle] {seen} pixels, {on} exactly on their circle")
    assert on >= 2 * len(ALL_CASES)


@pytest.mark.parametrize("family", ("zernike", "u16", "f32"))
def test_oracle_distance_from_the_reference(family):
    """The float64 oracle against the 50-digit reference, per column in units of 2^-53 S / normaliser: the number the GPU tolerance
    is set from.  The oracle must itself be within the project's rule."""
    worst = g.oracle_distance(family)
    col = int(np.argmax(worst))
    print(f"[oracle vs reference, {family}] worst: {worst[col]:.3g} x 2^-53 S / normaliser (column {g.ZERNIKE_NM[col]}); per column: "
          + " ".join(f"{v:.3g}" for v in worst))
    assert worst.max() < 4096  # plain float64 sums of at most 1196 terms
    vanishing = 0
    for name in g.ZERNIKE_CASES:
        ref, got = g.zernike_case(name, family), g.oracle_zernike(name, family)
        for row, t, L, present in rows(name):
            assert ref["present"][row] == present
            if not present or ref["normaliser"][row] == 0:
                assert np.isnan(got[row]).all() and np.isnan(ref["mag"][row]).all()  # absent, or one pixel: r = 0
                continue
            assert (np.abs(got[row] - ref["mag"][row]) <= g.zernike_tolerance(family, ref["S"][row], ref["normaliser"][row], ref["mag"][row])).all()
            vanishing += ref["vanishing"][row]
            # whether a moment has a phase (1e-9) hangs on no rounding: float32 pixels break the symmetry of the symmetric shapes
            # by about 1e-9, so say how near the threshold the nearest moment lies
            assert (np.abs(ref["mag"][row] / g.VANISHING - 1) > 1e-3).all(), (name, row, ref["mag"][row])
    print(f"[oracle vs reference, {family}] vanishing moments (below 1e-9): {vanishing}")


# ---- radial geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES + g.EXTRA)
def test_codes_agree_with_the_oracle(name):
    from oracle import radial_restated as rr

    lab = g.labels_of(name)
    for bin_count, maximum_radius in RADIAL_MODES:
        total, per_row = g.radial_case(name, bin_count, maximum_radius)
        compared = 0
        for (row, t, L, present), ours in zip(rows(name), per_row):
            kw = dict(scaled=maximum_radius is None, bin_count=bin_count, maximum_radius=maximum_radius or 100)
            geo = rr.object_geometry(np.asarray(lab[t]), L, **kw)
            if not present:
                assert geo is None and ours is None
                continue
            sl, m, good, bins, wedge, centre = geo
            codes, _, p = ours
            want = np.zeros(lab[t].shape, np.uint8)
            want[sl][good] = 0x80 | (wedge[good] << 4) | bins[good]
            assert np.array_equal(codes, want), (name, row, bin_count, maximum_radius)
            assert (int(p["ys"][p["centre"]]) - sl[0].start, int(p["xs"][p["centre"]]) - sl[1].start) == centre
            assert not codes[lab[t] != L].any() and (codes[lab[t] == L] != 0).sum() == sum(e >= 0 for e in p["e"])
            compared += 1
        assert compared == sum(p for *_, p in rows(name))
        assert not total[np.asarray(lab) == 0].any()


def test_no_ring_boundary_is_near_a_pixel():
    """bin_count * nrm of every reached pixel is at least 1e-9 away from an integer, so floor() is the same in float64 and at 50
    digits — with one exception that is exact on both sides: a path of diagonal steps only has the integer length d, and in the
    unscaled mode 4 d / 10 is an integer for d = 5, 10, ...; d / 10.0 is then a multiple of 0.5 and 4 * (d / 10.0) is that integer
    in float64 without any rounding.  The centre (nrm = 0) is exact as well."""
    exact = 0
    for name in ALL_CASES + g.EXTRA:
        for bin_count, maximum_radius in RADIAL_MODES:
            for ours in g.radial_case(name, bin_count, maximum_radius)[1]:
                if ours is None:
                    continue
                _, values, p = ours
                reached = [k for k in range(len(p["e"])) if p["e"][k] >= 0]
                assert len(values) == len(reached)
                for k, v in zip(reached, values):
                    off = abs(v - round(v))
                    if off < 1e-9:
                        assert off == 0 and p["e"][k] == 0, (name, bin_count, maximum_radius, k, v)
                        d = p["d"][k]
                        assert d == 0 or (maximum_radius is not None and (d / float(maximum_radius)) * bin_count == float(round(v))
                                          and (2 * d) % maximum_radius == 0)
                        exact += 1
    print(f"[ring boundaries] pixels exactly on one (the centres and pure diagonal paths): {exact}")


def test_paths_on_both_sides_of_the_old_sweep_bound():
    """k_radial_geometry once stopped after 4 (h + w) + 8 sweeps.  The winding shapes need at least 1.3 times as many steps on
    their cheapest path, every object of the small catalogue fewer: both sides of that bound stay tested whatever the kernel does."""
    for name, (_, long_paths) in g.WINDING.items():
        for ours in g.radial_case(name, 4)[1]:
            p = ours[2]
            h, w = int(np.ptp(p["ys"])) + 1, int(np.ptp(p["xs"])) + 1
            steps = g.path_steps(p)
            print(f"[paths] {name}: {steps} steps, the old bound {g.old_sweep_cap(h, w)}, pixels no path reaches: {sum(e < 0 for e in p['e'])}")
            if long_paths:
                assert steps >= 1.3 * g.old_sweep_cap(h, w) and min(p["e"]) >= 0
            else:
                assert sum(e < 0 for e in p["e"]) == 135 and steps < g.old_sweep_cap(h, w)  # the second component, a 15 x 16 serpentine
    for ours in g.radial_case("small", 4)[1]:
        if ours is not None:
            p = ours[2]
            assert g.path_steps(p) < g.old_sweep_cap(int(np.ptp(p["ys"])) + 1, int(np.ptp(p["xs"])) + 1)
    # label 10 of the small catalogue: every pixel is at distance 1, the last one lies in the 1 x 2 component, and the 3 x 2
    # component is out of reach
    p = g.radial_case("small", 4)[1][9][2]
    assert p["n_max"] == 8 and sum(e < 0 for e in p["e"]) == 6 and sum(e >= 0 for e in p["e"]) == 2


def test_the_tie_rule_is_exercised():
    """Several pixels of maximal distance: the centre is the last of them in raster order.  Of the small catalogue the ring has 4
    (the inner corners of its 2-pixel wall), the lines, diagonals, the checkerboard, the S, the spiral and the C have every pixel
    at distance 1, and so have the winding shapes.  The 5 x 5 square and the plus have ONE (their middle, at 3 and sqrt(2)), and so
    has the 2 x 2 in the frame's corner: the frame's border is not background, so its corner pixel is at distance 2 and the other
    three at 1 — there the border rule decides, not the tie rule."""
    per_row = g.radial_case("small", 4)[1]
    tied = {2: 2, 4: 9, 5: 9, 6: 7, 7: 7, 9: 4, 10: 8, 11: 18, 17: 7, 18: 2, 19: 31, 21: 11}
    for L in shape_ref.SMALL:
        for t in range(2):
            p = per_row[t * shape_ref.N_SMALL + L - 1][2]
            assert p["n_max"] == tied.get(L, 1), L
            top = max(p["d2"])
            assert p["centre"] == max(k for k, v in enumerate(p["d2"]) if v == top)
    for t, corner in ((0, (0, 95)), (1, (0, 0))):
        p = per_row[t * shape_ref.N_SMALL + 2][2]
        assert (int(p["ys"][p["centre"]]), int(p["xs"][p["centre"]])) == corner and sorted(p["d2"]) == [1, 1, 1, 4]
    for name in g.WINDING:
        assert all(r[2]["n_max"] > 1 for r in g.radial_case(name, 4)[1]) == (name != "two_components")
    # the border of the frame is not background: the 5 x 6 block in the corner has its centre ON the border, 5 from the row below
    # the block; (0, 0) and (0, 1) tie (column 6 is 6 and 5 away), the later one is taken
    per_row = g.radial_case("frame12x16", 4)[1]
    p = per_row[0][2]
    assert (int(p["ys"][p["centre"]]), int(p["xs"][p["centre"]])) == (0, 1) and max(p["d2"]) == 25 and p["n_max"] == 2
    p = per_row[2][2]
    assert len(p["ys"]) == 12 * 16 - 1 and max(p["d2"]) == 7 ** 2 + 9 ** 2 and p["n_max"] == 1  # (11, 0) from the hole at (4, 9)


def test_columns_agree_with_the_oracle():
    from oracle import radial_restated as rr

    for name in ("small", "serpentine31x32", "two_components", "frame12x16"):
        lab, px = g.labels_of(name), g.planes(name)
        for bin_count, maximum_radius in RADIAL_MODES:
            rings = bin_count if maximum_radius is None else bin_count + 1
            names = rr.names(bin_count, maximum_radius is None)
            per_row = g.radial_case(name, bin_count, maximum_radius)[1]
            row = 0
            for t in range(lab.shape[0]):
                kw = dict(bin_count=bin_count) if maximum_radius is None else dict(bin_count=bin_count, scaled=False, maximum_radius=maximum_radius)
                want = rr.get_radial_distribution(np.asarray(lab[t]), px[t, 0], **kw)
                for k in range(int(lab[t].max())):
                    ours = per_row[row]
                    row += 1
                    if ours is None:
                        assert all(np.isnan(want[n][k]) for n in names)
                        continue
                    got = g.radial_columns(ours[0], px[t, 0], bin_count, rings)
                    assert np.allclose(got, [want[n][k] for n in names], rtol=1e-12, atol=1e-14), (name, t, k)
