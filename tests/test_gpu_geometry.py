"""
The three 2-D kernels that an object's geometry drives beside the size/shape ones — k_mec and k_zernike / k_zernike_multi
(aliby_amd/csrc/feat_zernike.hip), k_radial_geometry and k_radial_stats (aliby_amd/csrc/feat_radial.hip) — on the catalogue of
degenerate shapes of tests/shape_ref.py and on the winding shapes of tests/geometry_ref.py, against that file's exact and
50-digit references.  tests/test_cpu_geometry_ref.py pins the references to the oracles and checks, without a GPU, the
preconditions under which the rules below do not hang on a rounding.

Every case runs under the object table's true limits and under the hints "96x96" and "400x400" of tests/test_gpu_object_forms.py
where these are not below the true limits, so that the LDS forms and k_mec<true> / k_radial_geometry<true> see the same shapes.

Rules:
    minimum enclosing circle   centre and radius within 1e-12 relative (1e-12 absolute on the centre) of the exact circle: what
                               the kernel's own stopping rule d^2 <= r^2 (1 + 1e-12) + 1e-12 permits.  K = the hull vertices of a
                               gift wrap over all the pixels.  Absent rows NaN, NaN, NaN, 0.  Bit for bit across the hints.
    Zernike magnitudes         per column 8 max(D, 64) 2^-53 S / normaliser, S the sum of the terms' magnitudes, D the distance
                               of the float64 oracle from the 50-digit reference in that unit, measured on the CPU
                               (geometry_ref.oracle_distance); never looser than 1e-4 relative + 1e-8 absolute.  The worst error in
                               units of the derived tolerance is printed per family.
    Zernike phases             an error of t in each of Re and Im turns a moment of magnitude M by at most 2 t / M; the same cap.
                               Left out where the moment is below 1e-9 on both sides, and only there: their number is the
                               reference's own number of vanishing moments.
    ring / wedge map           byte for byte on every pixel of the frame, 0 wherever no object is.
    FracAtD, MeanFrac          uint16 pixels: 4 ulp (sums of fewer than 2^37 integers below 2^16 are exact in float64 in any order)
    RadialCV                   uint16 pixels: 1e-12 relative + 1e-12 absolute;   float32 pixels: 1e-4 relative + 1e-8 absolute
"""
import numpy as np
import pytest

from tests import geometry_ref as g
from tests import shape_ref
from tests.test_gpu_object_forms import RUNGS, forms, hinted

pytestmark = pytest.mark.gpu

HINTS = ("true", "96x96", "400x400")
RADIAL_MODES = ((4, None), (5, None), (4, 10))
MEC_CASES = tuple(shape_ref.CASES) + tuple(g.WINDING) + ("acute",)
RADIAL_CASES = ("small",) + tuple(g.WINDING) + g.EXTRA

_DEVICE = {}


def _device(engine, name):
    """-> (labels on the GPU, the object table with its true limits), made once per case"""
    if name not in _DEVICE:
        from aliby_amd.extraction.engine import to_device_u16

        lab = g.labels_of(name)
        dl = to_device_u16(np.array(lab))
        tab = engine.object_table(dl)
        assert (tab.max_h, tab.max_w, tab.max_area) == shape_ref.table_limits(lab)
        assert tab.n_obj == len(g.objects_of(name))
        _DEVICE[name] = (dl, tab)
    return _DEVICE[name]


def _tables(tab):
    """-> [(hint, a fresh copy of the table under it)] for the hints that are not below the table's true limits"""
    out = []
    for hint in HINTS:
        lim = RUNGS[hint]
        if lim is None or (lim[0] >= tab.max_h and lim[1] >= tab.max_w and lim[2] >= tab.max_area):
            out.append((hint, hinted(tab, lim)))
    return out


def _planes(name, mode):
    from aliby_amd.extraction.engine import to_device_planes

    key = (name, mode)
    if key not in _DEVICE:
        _DEVICE[key] = to_device_planes(np.array(g.planes(name, mode)))
    return _DEVICE[key]


def test_hints_reach_the_other_forms():
    assert forms(*RUNGS["96x96"])["k_radial_geometry"] == "attr" and forms(*RUNGS["400x400"])["k_radial_geometry"] == "glob"
    lim = shape_ref.table_limits(g.labels_of("serpentine46x48_thick"))
    assert forms(*lim)["k_radial_geometry"] == "lds" and lim[0] <= 96 and lim[1] <= 96


# ---- minimum enclosing circle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MEC_CASES)
def test_mec_against_the_exact_circle(engine, name):
    import mpmath

    dl, tab = _device(engine, name)
    lab = g.labels_of(name)
    runs = {hint: engine.mec(dl, table).cpu().numpy()[: tab.n_obj] for hint, table in _tables(tab)}
    got = runs["true"]
    for hint, other in runs.items():
        assert shape_ref.same_bits(other, got), (name, hint)
    worst = 0.0
    for row, ((t, L), circ) in enumerate(zip(g.objects_of(name), g.circles(name))):
        if circ is None:
            assert np.isnan(got[row, :3]).all() and got[row, 3] == 0, (name, row, got[row])
            continue
        (ci, cj, r2), n_hull, _ = circ
        assert got[row, 3] == n_hull, (name, row, got[row], n_hull)
        want = np.array([float(ci), float(cj), float(mpmath.sqrt(mpmath.mpf(r2.numerator) / r2.denominator, prec=200))])
        if r2 == 0:
            assert n_hull == 1 and np.array_equal(got[row, :3], want), (name, row, got[row])
            continue
        err = np.abs(got[row, :3] - want)
        allow = 1e-12 * np.abs(want) + np.array([1e-12, 1e-12, 0.0])
        worst = max(worst, float((err / allow).max()))
        assert (err <= allow).all(), (name, row, got[row], want)
        if name.startswith("arc"):
            ys, xs = np.nonzero(lab[t] == L)
            assert g.mec_certificate(list(zip(ys.tolist(), xs.tolist())), *got[row, :3]), (name, row, got[row])
    print(f"[mec {name}] hints {list(runs)}; worst error / allowance: {worst:.3g}")


# ---- Zernike ------------------------------------------------------------------------------------------------------------------
def _angle(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def _check_zernike(name, family, got_mag, got_phase):
    """-> worst magnitude error in units of the derived tolerance"""
    ref = g.zernike_case(name, family)
    worst, left_out = 0.0, 0
    for row in range(len(ref["present"])):
        if not ref["present"][row] or ref["normaliser"][row] == 0:  # absent, or one pixel (r = 0): NaN on both sides
            assert np.isnan(got_mag[row]).all() and np.isnan(ref["mag"][row]).all(), (name, family, row)
            assert got_phase is None or np.isnan(got_phase[row]).all()
            continue
        want, S, norm = ref["mag"][row], ref["S"][row], ref["normaliser"][row]
        derived = 8 * np.maximum(g.oracle_distance(family), 64.0) * g.U53 * S / norm
        tol = g.zernike_tolerance(family, S, norm, want)
        err = np.abs(got_mag[row] - want)
        worst = max(worst, float(np.where(err == 0, 0.0, err / np.where(derived > 0, derived, np.finfo(float).tiny)).max()))
        assert (err <= tol).all(), (name, family, row, int(np.argmax(err - tol)), got_mag[row], want)
        if got_phase is not None:
            skip = (np.abs(got_mag[row]) < g.VANISHING) & (want < g.VANISHING)
            left_out += int(skip.sum())
            assert int(skip.sum()) == ref["vanishing"][row], (name, family, row)
            keep = ~skip
            ptol = np.minimum(2 * tol[keep] / want[keep], 1e-4 * np.abs(ref["phase"][row][keep]) + 1e-8)
            diff = _angle(got_phase[row][keep], ref["phase"][row][keep])
            assert (diff <= ptol).all(), (name, family, row, got_phase[row][keep], ref["phase"][row][keep])
    if got_phase is not None:
        assert left_out == int(ref["vanishing"].sum())
    return worst


@pytest.mark.parametrize("name", g.ZERNIKE_CASES)
def test_zernike_against_the_50_digit_reference(engine, name):
    import torch

    dl, tab = _device(engine, name)
    n = tab.n_obj
    worst = {}
    first = None
    for hint, table in _tables(tab):
        res = {}
        out = engine.new_output(n, 30)
        engine.zernike(dl, None, 0, 0, table, out, 0, weighted=False)
        res["zernike"] = out
        for mode in ("u16", "f32"):
            dp, dt = _planes(name, mode)
            for ch in range(3):
                out = engine.new_output(n, 60)
                engine.zernike(dl, dp, dt, ch, table, out, 0, weighted=True)
                res[mode, ch] = out
            for chans in ((0, 1), (2, 0, 1)):
                out = engine.new_output(n, 60 * len(chans) + 3)
                engine.radial_zernikes_multi(dl, dp, dt, chans, table, out, [3 + 60 * k for k in range(len(chans))])
                res[mode, chans] = out
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in res.items()}
        for mode in ("u16", "f32"):  # several channels in one launch: the single-channel bits
            for chans in ((0, 1), (2, 0, 1)):
                assert np.isnan(res[mode, chans][:, :3]).all()
                for k, ch in enumerate(chans):
                    assert shape_ref.same_bits(res[mode, chans][:, 3 + 60 * k: 63 + 60 * k], res[mode, ch]), (name, hint, mode, chans, ch)
        if first is None:
            first = res
            worst["zernike"] = _check_zernike(name, "zernike", res["zernike"], None)
            for mode in ("u16", "f32"):
                worst[mode] = _check_zernike(name, mode, res[mode, 0][:, :30], res[mode, 0][:, 30:])
        else:  # k_mec gives the same circle under every hint, and k_zernike reads nothing else of the table's limits
            for k in res:
                assert shape_ref.same_bits(res[k], first[k]), (name, hint, k)
    print(f"[zernike {name}] worst error / (8 max(D, 64) 2^-53 S / normaliser): " + ", ".join(f"{k}: {v:.3g}" for k, v in worst.items()))


# ---- radial geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RADIAL_CASES)
def test_ring_and_wedge_map_byte_for_byte(engine, name):
    dl, tab = _device(engine, name)
    lab = np.asarray(g.labels_of(name))
    for bin_count, maximum_radius in RADIAL_MODES:
        want, per_row = g.radial_case(name, bin_count, maximum_radius)
        assert not want[lab == 0].any()
        for hint, table in _tables(tab):
            got = engine.radial_geometry(dl, table, bin_count, maximum_radius).cpu().numpy()
            bad = got != want
            lost = bad & (got == 0) & (want != 0)
            assert not bad.any(), (f"{name}, bin_count {bin_count}, maximum_radius {maximum_radius}, table {hint}: {int(bad.sum())} of "
                                   f"{int((lab > 0).sum())} object pixels differ, {int(lost.sum())} of them got no code (no path found), "
                                   f"{int((bad & (lab == 0)).sum())} lie on no object")
    print(f"[radial map {name}] {int((want != 0).sum())} coded pixels, tables {[h for h, _ in _tables(tab)]}")


@pytest.mark.parametrize("name", RADIAL_CASES)
def test_radial_columns(engine, name):
    import torch

    dl, tab = _device(engine, name)
    n = tab.n_obj
    worst_ulp = worst_cv = 0.0
    for bin_count, maximum_radius in RADIAL_MODES:
        rings = bin_count if maximum_radius is None else bin_count + 1
        per_row = g.radial_case(name, bin_count, maximum_radius)[1]
        for mode in ("u16", "f32"):
            dp, dt = _planes(name, mode)
            px = g.planes(name, mode)
            out = engine.new_output(n, 3 * rings)
            kw = {} if maximum_radius is None else dict(scaled=False, maximum_radius=maximum_radius)
            engine.radial_distribution(dl, dp, dt, 0, hinted(tab, None), out, 0, bin_count=bin_count, **kw)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for row, ((t, _), ours) in enumerate(zip(g.objects_of(name), per_row)):
                if ours is None:
                    assert np.isnan(got[row]).all(), (name, row)
                    continue
                want = g.radial_columns(ours[0], px[t, 0], bin_count, rings)
                err = np.abs(got[row] - want)
                where = (name, bin_count, maximum_radius, mode, row, got[row], want)
                if mode == "f32":
                    assert (err <= 1e-4 * np.abs(want) + 1e-8).all(), where
                    continue
                ulps = err[: 2 * rings] / np.spacing(np.abs(want[: 2 * rings]))
                cv = err[2 * rings:] / (1e-12 * np.abs(want[2 * rings:]) + 1e-12)
                worst_ulp, worst_cv = max(worst_ulp, float(ulps.max())), max(worst_cv, float(cv.max()))
                assert (ulps <= 4).all() and (cv <= 1).all(), where
    print(f"[radial columns {name}] uint16: FracAtD / MeanFrac worst {worst_ulp:.3g} ulp; RadialCV worst {worst_cv:.3g} of its allowance")


def test_winding_maps_do_not_depend_on_what_the_scratch_held(engine):
    """The global form keeps its distance and path words in the context's scratch block.  Between two runs of the winding shapes
    the size/shape kernels of the small catalogue run in their global forms and leave their own working sets there."""
    import torch

    def maps():
        out = {}
        for name in g.WINDING:
            dl, tab = _device(engine, name)
            for bin_count, maximum_radius in RADIAL_MODES:
                out[name, bin_count, maximum_radius] = engine.radial_geometry(dl, hinted(tab, RUNGS["400x400"]), bin_count, maximum_radius).cpu().numpy()
        return out

    before = maps()
    dl, tab = _device(engine, "small")
    big = hinted(tab, RUNGS["400x400"])
    f = forms(*RUNGS["400x400"])
    assert f["k_shape_edt"] == f["k_shape_core"] == f["k_radial_geometry"] == "glob"
    out = engine.new_output(tab.n_obj, 78)
    engine.sizeshape(dl, big, out, 0)
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()[0, 0])
    after = maps()
    for key, want in before.items():
        assert np.array_equal(after[key], want), key
        assert np.array_equal(want, g.radial_case(*key)[0]), key
