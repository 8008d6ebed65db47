"""
tests/intensity_ref.py against oracle/cp_measure_restated.get_intensity and against rows computed by hand, and the preconditions
of tests/test_gpu_pixel_patterns.py on the inputs of tests/pixel_patterns.py.  No GPU.
"""
import functools
import math
import warnings

import numpy as np
import pytest

from tests import coloc3d_ref
from tests import intensity_ref as ref
from tests import pixel_patterns as pp

PAIRS = [(0, 1), (0, 2), (1, 2)]
# (mode, scale_max) of every colocalisation run of tests/test_gpu_pixel_patterns.py
COLOC_RUNS = [("u16", 255.0), ("f32", 255.0), ("u16", 65535.0)]


def _unit(px):
    return (px.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """-> labels [F, Y, X], uint16 pixels [F, C, Y, X], rows per tile"""
    if name in pp.SCENES:
        return pp.SCENES[name]()
    if name == "object_forms":
        from tests.test_gpu_object_forms import scene

        return scene()
    assert name == "synth"
    from aliby_amd import synth

    f = synth.make_fov(1, 3, shape=(160, 176), n_channels=2, n_target=10)
    lab = np.asarray(f["cells"], np.uint16)[None]
    return lab, np.asarray(f["pixels"][:, 0], np.uint16)[None], (int(lab.max()),)


def test_column_names_are_the_kernels():
    from aliby_amd.extraction import features as feat

    for edge in (True, False):
        assert ref.names(edge) == feat.intensity_names(edge)


# ------------------------------------------------------------------------------------------------ reference against oracle
@pytest.mark.parametrize("mode", pp.MODES)
@pytest.mark.parametrize("name", ["tiles", "full_frame", "object_forms", "synth"])
def test_reference_equals_oracle(name, mode):
    """The oracle passes the rule the kernel has to pass (`ref.check`: the same bits in the exact columns, NaN in the same
    places), and the other columns are within 1e-12."""
    from oracle import cp_measure_restated as cpm

    lab, px, counts = _inputs(name)
    px = px if mode == "u16" else _unit(px)
    for edge in (True, False):
        for ch in range(px.shape[1]):
            want, meta = ref.intensity_batch(lab, px, ch, counts, edge)
            rows = []
            for f, n in enumerate(counts):
                res = cpm.get_intensity(lab[f], px[f, ch], edge_measurements=edge)
                assert all(len(v) == n for v in res.values())
                rows.append(np.column_stack([np.asarray(res[k], float) for k in ref.names(edge)]))
            got = np.concatenate(rows)
            # called on a label image that skips a value, the oracle leaves the zeros it initialises the edge columns with in that
            # row (tests/test_gpu_object_forms.py, oracle_intensity): they are no measurement
            absent = np.asarray([m["n"] == 0 for m in meta], bool)
            assert np.isnan(got[absent][:, [j for j, k in enumerate(ref.names(edge)) if k not in ref.EDGE]]).all()
            got[absent] = np.nan
            ref.check(got, want, meta, f"oracle, {name}, channel {ch}, edge {edge}", mode, edge)
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True)


# ------------------------------------------------------------------------------------------------ rows computed by hand
def _row(name, ch=0, mode="u16"):
    lab, _, counts = pp.tiles()
    tile, label = pp.label_of(name)
    cols, meta = ref.one_object(lab[tile], pp.planes("tiles", mode)[tile, ch], label)
    return cols, meta


def test_ellipses_have_187_pixels_in_a_box_of_15_by_17():
    lab = pp.tiles()[0]
    for k in range(len(pp.ELLIPSES)):
        ys, xs = np.nonzero(lab[0] == k + 1)
        assert len(ys) == 187 and (ys.max() - ys.min() + 1, xs.max() - xs.min() + 1) == (15, 17)
    assert max(np.ptp(np.nonzero(lab[f] == L)[a]) + 1 for f in range(2) for L in range(1, int(lab[f].max()) + 1) if (lab[f] == L).any() for a in range(2)) <= 20


def test_pair_5_9():
    """N = 2.  Quartile index N q = 0.5, 1, 1.5.  LQ: qi = 0 < N - 1, qf = .5: 5 * .5 + 9 * .5 = 7.  Median: qi = 1 = N - 1: s[1] = 9.
    UQ: qi = 1 = N - 1: 9.  Deviations from 9: (4, 0), sorted (0, 4); index 1 = N - 1: MAD = 4."""
    c, _ = _row("pair")
    assert (c["Intensity_LowerQuartileIntensity"], c["Intensity_MedianIntensity"], c["Intensity_UpperQuartileIntensity"], c["Intensity_MADIntensity"]) == (7.0, 9.0, 9.0, 4.0)
    assert (c["Intensity_IntegratedIntensity"], c["Intensity_MeanIntensity"], c["Intensity_StdIntensity"]) == (14.0, 7.0, 2.0)
    # x = 3, 4: centre 3.5, weighted (3 * 5 + 4 * 9) / 14 = 51 / 14; displacement 51 / 14 - 7 / 2 = 1 / 7
    assert c["Location_CenterMassIntensity_X"] == 51 / 14 and c["Location_CenterMassIntensity_Y"] == 8.0 and c["Location_CenterMassIntensity_Z"] == 0.0
    assert abs(c["Intensity_MassDisplacement"] - 1 / 7) < 1e-15
    assert (c["Location_MaxIntensity_X"], c["Location_MaxIntensity_Y"], c["Location_MaxIntensity_Z"]) == (4.0, 8.0, 0.0)
    # both pixels have a neighbour of another label: the edge columns repeat the object's
    assert [c[k] for k in ref.EDGE] == [c[k] for k in ref.CORE]


def test_triple_5_5_9():
    """N = 3, sorted (5, 5, 9).  Index N q = 0.75, 1.5, 2.25.  LQ: qi = 0, qf = .75: 5 * .25 + 5 * .75 = 5.  Median: qi = 1 < N - 1,
    qf = .5: 5 * .5 + 9 * .5 = 7.  UQ: qi = 2 = N - 1: s[2] = 9.  Deviations from 7: (2, 2, 2); index 1.5: 2 * .5 + 2 * .5: MAD = 2.
    (The rule is CellProfiler's index N q, as the kernel's and the oracle's headers state it; numpy's median of this list would be 5.)"""
    c, _ = _row("triple")
    assert (c["Intensity_LowerQuartileIntensity"], c["Intensity_MedianIntensity"], c["Intensity_UpperQuartileIntensity"], c["Intensity_MADIntensity"]) == (5.0, 7.0, 9.0, 2.0)
    # two maxima?  No: one 9, at the last pixel.  The tie is in the minimum; channel 1 = (1, 2, 3) has its maximum there too.
    assert (c["Location_MaxIntensity_X"], c["Location_MaxIntensity_Y"]) == (5.0, 12.0)
    # variance ((5 - 19/3)^2 * 2 + (9 - 19/3)^2) / 3 = (32/9 + 64/9) / 3 = 32 / 9
    assert abs(c["Intensity_StdIntensity"] - math.sqrt(32 / 9)) < 1e-15


def test_four_and_five():
    """(7, 1, 12, 4) sorted (1, 4, 7, 12), N = 4: index 1, 2, 3: LQ 4, median 7, UQ s[3] = 12 (qi = N - 1).  Deviations from 7:
    (0, 6, 5, 3) sorted (0, 3, 5, 6); index 2: MAD 5.
    (1..5), N = 5: index 1.25, 2.5, 3.75: LQ 2 * .75 + 3 * .25 = 2.25, median 3 * .5 + 4 * .5 = 3.5, UQ 4 * .25 + 5 * .75 = 4.75.
    Deviations from 3.5: (2.5, 1.5, .5, .5, 1.5) sorted (.5, .5, 1.5, 1.5, 2.5); index 2.5: 1.5 * .5 + 1.5 * .5: MAD 1.5."""
    c, _ = _row("four")
    assert (c["Intensity_LowerQuartileIntensity"], c["Intensity_MedianIntensity"], c["Intensity_UpperQuartileIntensity"], c["Intensity_MADIntensity"]) == (4.0, 7.0, 12.0, 5.0)
    c, _ = _row("five")
    assert (c["Intensity_LowerQuartileIntensity"], c["Intensity_MedianIntensity"], c["Intensity_UpperQuartileIntensity"], c["Intensity_MADIntensity"]) == (2.25, 3.5, 4.75, 1.5)
    c, _ = _row("five", mode="f32")  # the same in units of 1 / 65535, each step exact or correctly rounded
    one = float(np.float32(1.0) / np.float32(65535.0))
    assert abs(c["Intensity_MedianIntensity"] / one - 3.5) < 1e-6 and abs(c["Intensity_MADIntensity"] / one - 1.5) < 1e-6


def test_single_pixels_and_the_absent_label():
    c, m = _row("one_pixel")
    assert m["n"] == 1 and m["flat"] and m["displacement_zero"]
    for k in ("Integrated", "Mean", "Min", "Max", "LowerQuartile", "Median", "UpperQuartile"):
        assert c[f"Intensity_{k}Intensity"] == 321.0, k
    assert c["Intensity_StdIntensity"] == 0.0 and c["Intensity_MADIntensity"] == 0.0 and c["Intensity_MassDisplacement"] == 0.0
    assert (c["Location_CenterMassIntensity_X"], c["Location_CenterMassIntensity_Y"], c["Location_CenterMassIntensity_Z"]) == (8.0, 3.0, 0.0)
    c, m = _row("one_zero")
    assert m["dark"] and all(math.isnan(c[k]) for k in ("Location_CenterMassIntensity_X", "Location_CenterMassIntensity_Y", "Location_CenterMassIntensity_Z", "Intensity_MassDisplacement"))
    assert (c["Location_MaxIntensity_X"], c["Location_MaxIntensity_Y"], c["Intensity_MeanIntensity"], c["Intensity_MADIntensity"]) == (3.0, 3.0, 0.0, 0.0)
    lab = pp.tiles()[0]
    c, m = ref.one_object(lab[1], pp.tiles()[1][1, 0], pp.ABSENT_LABEL)
    assert m["n"] == 0 and all(math.isnan(v) for v in c.values())


def test_zero_ellipse():
    """NaN in CenterMassIntensity X / Y / Z and in MassDisplacement (0 / 0), the position of the maximum is the object's last pixel
    (every pixel ties), 0 in every other column."""
    lab = pp.tiles()[0]
    for mode in pp.MODES:
        for ch in range(3):
            cols, meta = _row("zero", ch, mode)
            ys, xs = np.nonzero(lab[0] == pp.label_of("zero")[1])
            for k, v in cols.items():
                if k in ("Location_CenterMassIntensity_X", "Location_CenterMassIntensity_Y", "Location_CenterMassIntensity_Z", "Intensity_MassDisplacement"):
                    assert math.isnan(v), k
                elif k == "Location_MaxIntensity_X":
                    assert v == xs[-1]
                elif k == "Location_MaxIntensity_Y":
                    assert v == ys[-1]
                else:
                    assert v == 0.0 and not math.copysign(1.0, v) < 0, k
            assert meta["dark"] and meta["flat"] and meta["flat_edge"] and meta["n_edge"] > 0


def test_checkerboard_std_is_the_closed_form():
    """n1 pixels of 65535 and n0 of 0: variance 65535^2 n0 n1 / N^2, close to 32767.5^2."""
    lab, px, _ = pp.tiles()
    m = lab[0] == pp.label_of("checkerboard")[1]
    n1 = int((px[0, 0][m] == 65535).sum())
    n0 = int(m.sum()) - n1
    assert n0 + n1 == 187 and abs(n0 - n1) <= 3 and set(np.unique(px[0, 0][m])) == {0, 65535}
    cols, _ = _row("checkerboard")
    want = 65535.0 * math.sqrt(n0 * n1) / 187.0
    assert abs(cols["Intensity_StdIntensity"] - want) <= 2 * math.ulp(want) and abs(want - 32767.5) < 5.0
    assert cols["Intensity_MedianIntensity"] in (0.0, 65535.0) and cols["Intensity_MADIntensity"] in (0.0, 65535.0)


def test_flat_objects_are_flat_and_exact():
    for name, value in (("flat", 1234), ("saturated", 65535)):
        for mode in pp.MODES:
            v = float(value) if mode == "u16" else float(np.float32(value) / np.float32(65535.0))
            cols, meta = _row(name, 1, mode)
            assert meta["flat"] and meta["flat_edge"] and meta["displacement_zero"] and meta["mad_exact"]
            assert cols["Intensity_MeanIntensity"] == v and cols["Intensity_StdIntensity"] == 0.0 and cols["Intensity_MassDisplacement"] == 0.0
            assert cols["Intensity_MedianIntensity"] == v and cols["Intensity_MADIntensity"] == 0.0 and cols["Intensity_MeanIntensityEdge"] == v


def test_full_frame_has_no_edge_pixel():
    lab, px, _ = pp.full_frame()
    cols, meta = ref.one_object(lab[0], px[0, 0], 1)
    assert meta["n"] == 192 and meta["n_edge"] == 0 and all(cols[k] == 0.0 for k in ref.EDGE)
    assert (cols["Location_MaxIntensity_X"], cols["Location_MaxIntensity_Y"]) == (15.0, 11.0)
    cols, _ = ref.one_object(lab[0], px[0, 1], 1)  # (the falling ramp)
    assert (cols["Location_MaxIntensity_X"], cols["Location_MaxIntensity_Y"]) == (0.0, 0.0)


def test_edge_pixels_of_the_corner_object_ignore_the_frame():
    """3 x 4 in the frame's last corner: only the first row and the first column have a neighbour inside the frame with another
    label (6 pixels); the frame is no boundary."""
    lab, px, _ = pp.tiles()
    _, meta = ref.one_object(lab[1], px[1, 0], pp.CORNER_LABEL)
    assert meta["n"] == 12 and meta["n_edge"] == 6 and lab[1, -1, -1] == pp.CORNER_LABEL


# ------------------------------------------------------------------------------------------------ preconditions
def test_plateau_and_flat_objects_hold_several_maxima_and_the_last_is_not_the_first():
    """The tie rule of Location_MaxIntensity is visible only where the first and the last raveled maximum differ in x AND in y, and
    (for the plateau) where the last one is not simply the object's last pixel."""
    lab, px, _ = pp.tiles()
    for name, n_max in (("plateau", 15), ("flat", 187), ("saturated", 187), ("zero", 187)):
        m = lab[0] == pp.label_of(name)[1]
        ys, xs = np.nonzero(m & (px[0, 0] == px[0, 0][m].max()))
        assert len(ys) == n_max and ys[0] != ys[-1] and xs[0] != xs[-1], name
        cols, _ = _row(name)
        assert (cols["Location_MaxIntensity_X"], cols["Location_MaxIntensity_Y"]) == (xs[-1], ys[-1])
    oy, ox = np.nonzero(lab[0] == pp.label_of("plateau")[1])
    assert ys[-1] < oy.max() and (ys[-1], xs[-1]) != (oy[-1], ox[-1])
    # channel 0 of "ramp" is all distinct, the checkerboard ties 90 or 91 times
    m = lab[0] == pp.label_of("ramp")[1]
    assert len(np.unique(px[0, 0][m])) == 187 and np.array_equal(px[0, 1][m], px[0, 0][m][::-1])


def test_block_ties_its_maximum_256_box_positions_apart():
    """Channel 1 of "block": 32 maxima, at box positions 0..15 and 256..271 (a thread with a stride of 64, 128 or 256 meets two of
    them); the last is at position 271 = 13 * 20 + 11, not the object's last pixel.  Channel 0 is flat."""
    lab, px, _ = pp.tiles()
    m = lab[1] == pp.BLOCK_LABEL
    v = px[1, 1][m]
    assert v.size == 400 and np.array_equal(np.flatnonzero(v == v.max()), np.r_[0:16, 256:272]) and len(np.unique(px[1, 0][m])) == 1
    cols, meta = _row("block", 1)
    assert (cols["Location_MaxIntensity_X"], cols["Location_MaxIntensity_Y"]) == (pp.BLOCK[1].start + 11, pp.BLOCK[0].start + 13)
    assert _row("block", 0)[1]["flat"] and not meta["flat"]


def test_quartile_branches_are_all_taken():
    """Areas 1 to 5: every quartile with qi < N - 1 and with qi = N - 1, and every fractional part."""
    seen = set()
    for n in range(1, 6):
        for q in (0.25, 0.5, 0.75):
            seen.add((int(n * q) < n - 1, n * q - int(n * q)))
    assert {f for _, f in seen} == {0.0, 0.25, 0.5, 0.75} and {b for b, _ in seen} == {True, False}
    lab = pp.tiles()[0]
    assert sorted(int((lab[1] == L).sum()) for L in range(1, 9)) == [1, 1, 2, 3, 4, 4, 5, 5]


@pytest.mark.parametrize("mode,scale_max", COLOC_RUNS)
def test_no_costes_probe_is_near_a_sign_change(mode, scale_max):
    """Every object, pair, dtype and scale_max of the GPU test: the Pearson value of every probe of the oracle's Costes bisection is
    NaN (a channel constant over the probe's pixels, by construction: exactly zero variance in any float64 evaluation, since sums
    of at most 2^10 equal float32 values are exact) or at least PROBE_MARGIN from 0.  A pattern that fails is changed."""
    lab, _, counts = pp.tiles()
    px = pp.planes("tiles", mode)
    worst, n_nan, n_probes = np.inf, 0, 0
    for f, n in enumerate(counts):
        for a, b in PAIRS:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                logs = coloc3d_ref.costes_probes(lab[f][None], px[f, a][None], px[f, b][None], n, scale_max)
            for label, log in enumerate(logs, 1):
                v = np.asarray(log, float)
                n_probes += v.size
                n_nan += int(np.isnan(v).sum())
                v = v[~np.isnan(v)]
                if v.size:
                    worst = min(worst, float(np.abs(v).min()))
                    assert np.abs(v).min() >= coloc3d_ref.PROBE_MARGIN, (mode, scale_max, f, (a, b), label, float(np.abs(v).min()))
    print(f"pixel patterns, {mode}, scale_max {scale_max}: {n_probes} Costes probes, {n_nan} NaN, smallest |Pearson| {worst:.2e}")
    assert n_probes > 0 and np.isfinite(worst)


@pytest.mark.parametrize("mode", pp.MODES)
def test_the_five_oracles_return_on_every_pattern(mode):
    """Intensity, texture (both scales), radial distribution (both binnings), weighted Zernikes and the four colocalisation metrics
    return on every pattern without raising, and NaN / 0 fall as tests/test_gpu_pixel_patterns.py expects them to."""
    from oracle import cp_measure_restated as cpm
    from oracle import radial_restated as rr
    from oracle import texture_restated as tx
    from oracle import zernike_restated as zr

    lab, _, counts = pp.tiles()
    px = pp.planes("tiles", mode)
    zero, flat, bright = pp.row_of("zero"), pp.row_of("flat"), pp.row_of("one_bright")
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for f in range(2):
            for ch in range(2):
                cpm.get_intensity(lab[f], px[f, ch])
                t3 = tx.get_texture(lab[f], px[f, ch])
                tx.get_texture(lab[f], px[f, ch], scale=1)
                r4 = rr.get_radial_distribution(lab[f], px[f, ch], bin_count=4)
                rr.get_radial_distribution(lab[f], px[f, ch], bin_count=3, scaled=False, maximum_radius=6)
                z = zr.get_radial_zernikes(lab[f], px[f, ch])
                if f == 0:
                    assert t3["Correlation_3_00_256"][flat] == 1.0 and t3["InfoMeas1_3_00_256"][flat] == 0.0
                    assert all(np.isnan(v[zero]) for v in t3.values())
                    assert np.isnan(r4["RadialDistribution_RadialCV_1of4"][zero])
                    assert z["RadialDistribution_ZernikeMagnitude_0_0"][zero] == 0.0
                else:
                    assert np.isnan(z["RadialDistribution_ZernikeMagnitude_0_0"][pp.label_of("one_zero")[1] - 1])
        want = np.concatenate([np.concatenate([coloc3d_ref.coloc3d(lab[f][None], px[f, a][None], px[f, b][None], n) for a, b in PAIRS], axis=1)
                               for f, n in enumerate(counts)])
    assert want.shape == (sum(counts), 24)
    assert np.isnan(want[zero, 2:4]).all() and (want[bright, 2:4] == 0).all()  # Manders: 0 / 0 against "no pixel above both"
    assert np.isnan(want[pp.row_of("corner") - 1]).all()  # the absent label
    triple = want[pp.row_of("triple"), 6:8]
    assert (triple == (1.0 if mode == "u16" else 0.0)).all(), triple
    same = want[:, 8:16]  # the pair (0, 2): identical channels
    ok = ~np.isnan(same[:, 0])
    assert np.allclose(same[ok, 0], 1.0, atol=1e-12) and np.allclose(same[ok, 1], 1.0, atol=1e-12)
    assert np.allclose(same[:, 2:4], same[:, 4:6], rtol=1e-12, equal_nan=True)  # RWC equal to Manders
    assert abs(want[pp.row_of("ramp"), 0] + 1.0) < 1e-12  # the reversed ramp
