"""
Every launch form of the ten 2-D per-object launch sites (aliby_amd/csrc/object_launch.h), against the oracle.

A site runs its kernel from dynamic LDS, one workgroup per object ("lds"; "attr" where the working set is so large that the
host first raises hipFuncAttributeMaxDynamicSharedMemorySize — above 48 KiB, the higher of the two thresholds the sites have
used, so the attribute call is made whichever of them holds), or from global scratch with at most 512 workgroups striding over
the objects ("glob").  Which one is decided from the object table's max_h, max_w and max_area alone.  These are capacities: the
kernels size their working sets from them and read each object's own box from the device table, so a copy of the table with
larger hints drives the same small objects through every form without a large image.

Working set in bytes per site (p2(n, lo) = power of two >= n, at least lo; r16 / r4 = rounded up to a multiple of 16 / 4) and
LDS budget:

    k_intensity        4 (p2(a, 64) + p2(a, 64) / 32 + 1)                                  128 KiB
    k_texture          r16(h w) + 4 p2(a, 2048)                                             96 KiB
    k_ranks, k_coloc   16 p2(a, 64)                                                         96 KiB
    k_cell             8 r4((h + 2)(w + 2)) + 4 p2(a, 64)                                  128 KiB
    k_shape_core       r16((h + 4)(w + 4))                                                  96 KiB
    k_shape_edt        r16(4 (h + 2)(w + 2) + 4 max((h + 2)(w + 2), p2(a, 64)))            128 KiB
    k_shape_hull       r16(152 h + 48)                  (sizeshape and feret)               96 KiB
    k_mec              r16(40 h + 32)                                                       96 KiB
    k_radial_geometry  8 r4((h + 2)(w + 2))                                                128 KiB

Form per rung (max_h, max_w, max_area) — every site is reached in all three:

    rung                 intensity texture ranks coloc cell  core  edt   hull  mec   radial_geometry
    true (<= 20, 20)     lds       lds     lds   lds   lds   lds   lds   lds   lds   lds
    (64, 64, 4096)       lds       lds     attr  attr  attr  lds   lds*  lds   lds   lds*
    (96, 96, 8192)       lds*      lds*    glob  glob  attr  lds   attr  lds   lds   attr
    (180, 180, 8192)     lds*      attr    glob  glob  glob  lds*  glob  lds   lds   glob
    (250, 250, 16384)    attr      glob    glob  glob  glob  attr  glob  lds*  lds   glob
    (500, 20, 2048)      lds       lds     lds   lds   attr  lds   attr  attr  lds   attr
    (400, 400, 60000)    glob      glob    glob  glob  glob  glob  glob  attr  lds   glob
    (400, 400, 65536)    glob      glob+   glob  glob  glob  glob  glob  attr  lds   glob
    (1500, 20, 4096)     lds       lds*    attr  attr  glob  lds*  glob  glob  attr  glob
    (2600, 20, 4096)     lds       attr    attr  attr  glob  attr  glob  glob  glob  glob

    *  between 32 and 48 KiB: in LDS, and the attribute is raised where the site's threshold is 32 KiB
    +  max_area >= 65536 turns k_texture's dense 16-bit cell counters off (cap_cells == 0)
    k_intensity is in LDS above 48 KiB only for 8192 < max_area <= 16384 (66 KiB; 32768 takes 132 KiB: global), and k_texture
    at (96, 96, 8192) takes 41 KiB, so (250, 250, 16384) and (180, 180, 8192) are their "attr" rungs.
    A hint is a capacity, so none may lie below the table's true value (`hinted` refuses it): the tall rungs, which are there
    for k_shape_hull and k_mec (working sets of 152 and 40 bytes per row of max_h), keep the true max_w of 20.

`test_rungs_reach_every_form` below recomputes the table from the formulas.

Input: 2 tiles of 96 x 128 with 7 and 6 label values (13 rows), no object above 20 x 20: ellipses, a ring (a hole), a concave
C, a line, a 2 x 2, one pixel, an object on the frame border; label 4 of tile 0 is absent (area 0: the NaN path); 2 channels,
as uint16 and as float32 scaled to [0, 1].

Comparison: per family the oracle call and rule of tests/test_gpu_features.py (exact-column lists) and
tests/test_gpu_edge_cases.py (`_close`: 1e-4 relative, an orientation or a phase compared as the axis or angle it is; the phase
of a vanishing Zernike moment skipped as `_run_both` skips it), the per-cell metrics by tests/cell_ref.check as in
tests/test_gpu_cell.py.  The exact-column lists hold for uint16 pixels, where they are stated; float32 pixels go by `_close`.
Every oracle is computed once per family and pixel type.
"""
import functools
import math

import numpy as np
import pytest

from tests import cell_ref
from tests.test_gpu_edge_cases import _close

pytestmark = pytest.mark.gpu

MODES = ("u16", "f32")
KIB = 1024
RUNGS = {
    "true": None,
    "64x64": (64, 64, 4096),
    "96x96": (96, 96, 8192),
    "180x180": (180, 180, 8192),
    "250x250": (250, 250, 16384),
    "500x20": (500, 20, 2048),
    "400x400": (400, 400, 60000),
    "400x400_sparse_texture": (400, 400, 65536),
    "1500x20": (1500, 20, 4096),
    "2600x20": (2600, 20, 4096),
}
rungs = pytest.mark.parametrize("rung", list(RUNGS))


# ---------------------------------------------------------------------------------------------- the launch forms, restated
def _p2(n, lo):
    p = lo
    while p < n:
        p <<= 1
    return p


def _r(n, m):
    return (n + m - 1) // m * m


def working_sets(h, w, a):
    """site -> (bytes of one workgroup's working set, LDS budget), restated from the host code of aliby_amd/csrc/feat_*.hip"""
    cells = (h + 2) * (w + 2)
    return {
        "k_intensity": (4 * (_p2(a, 64) + _p2(a, 64) // 32 + 1), 128 * KIB),
        "k_texture": (_r(h * w, 16) + 4 * _p2(a, 2048), 96 * KIB),
        "k_ranks": (16 * _p2(a, 64), 96 * KIB),
        "k_coloc": (16 * _p2(a, 64), 96 * KIB),
        "k_cell": (8 * _r(cells, 4) + 4 * _p2(a, 64), 128 * KIB),
        "k_shape_core": (_r((h + 4) * (w + 4), 16), 96 * KIB),
        "k_shape_edt": (_r(4 * cells + 4 * max(cells, _p2(a, 64)), 16), 128 * KIB),
        "k_shape_hull": (_r(4 * (2 * (2 * h + 1) + 2 * h) + 4 * (2 * (2 * h + 1) + 2) * 8, 16), 96 * KIB),
        "k_mec": (_r(2 * h * 4 + 2 * (2 * h + 2) * 8, 16), 96 * KIB),
        "k_radial_geometry": (8 * _r(cells, 4), 128 * KIB),
    }


def forms(h, w, a):
    return {site: "glob" if need > budget else ("attr" if need > 48 * KIB else "lds") for site, (need, budget) in working_sets(h, w, a).items()}


# ---------------------------------------------------------------------------------------------------------------- the input
def _ellipse(lab, L, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
    lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = L


@functools.lru_cache(maxsize=None)
def scene():
    """-> labels uint16 [2, 96, 128], planes uint16 [2, 2, 96, 128], rows per tile"""
    lab = np.zeros((2, 96, 128), np.uint16)
    t = lab[0]
    _ellipse(t, 1, 14.0, 16.0, 8.3, 6.1)
    _ellipse(t, 2, 40.0, 30.0, 9.4, 9.4)
    _ellipse(t, 0, 40.0, 30.0, 3.2, 3.2)  # ... a ring
    t[60:78, 60:66] = 3        # a concave C
    t[60:65, 60:76] = 3
    t[73:78, 60:76] = 3
    #                            label 4 is absent
    t[20, 100] = 5             # one pixel
    t[0:9, 70:88] = 6          # on the frame border
    t[85:87, 10:12] = 7        # 2 x 2
    u = lab[1]
    _ellipse(u, 1, 50.0, 64.0, 9.6, 7.2)
    u[10, 20:33] = 2           # a 1 x 13 line
    _ellipse(u, 3, 20.0, 100.0, 5.2, 9.7)
    u[70:90, 5:25] = 4         # 20 x 20
    u[78:82, 13:17] = 0        # ... with a hole
    _ellipse(u, 5, 80.0, 100.0, 7.7, 8.8)
    u[92:96, 120:128] = 6      # in the last corner of the frame
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:96, 0:128]
    px = np.empty((2, 2, 96, 128), np.uint16)
    for f in range(2):
        for c in range(2):
            smooth = 9000 + 7000 * np.sin(yy / (5.0 + c) + f) * np.cos(xx / (7.0 - c))
            px[f, c] = (smooth + rng.integers(0, 6000 + 20000 * c, size=(96, 128))).clip(0, 65535).astype(np.uint16)
    counts = (7, 6)
    assert [int(lab[f].max()) for f in range(2)] == list(counts)
    return lab, px, counts


def planes_of(mode):
    px = scene()[1]
    return px if mode == "u16" else (px.astype(np.float32) / np.float32(65535.0)).astype(np.float32)


_DEVICE = {}


def device(engine, mode):
    """-> (labels, planes, dtype code, the object table with its true limits) on the GPU, made once per pixel type"""
    if mode not in _DEVICE:
        from aliby_amd.extraction.engine import to_device_planes, to_device_u16

        dl = to_device_u16(scene()[0])
        dp, dt = to_device_planes(planes_of(mode))
        tab = engine.object_table(dl)
        assert tab.n_obj == 13 and tab.max_h <= 20 and tab.max_w <= 20 and int((tab.host["area"] == 0).sum()) == 1 and int(tab.host["area"][tab.host["area"] > 0].min()) == 1
        _DEVICE[mode] = (dl, dp, dt, tab)
    return _DEVICE[mode]


def hinted(tab, hint):
    """A copy of the table that announces larger objects (nothing else changes), without the results cached on the original."""
    big = type(tab).__new__(type(tab))
    big.__dict__.update(tab.__dict__)
    for cached in ("_mec", "_binmaps", "_ranks"):
        big.__dict__.pop(cached, None)
    if hint is not None:
        assert hint[0] >= tab.max_h and hint[1] >= tab.max_w and hint[2] >= tab.max_area
        big.max_h, big.max_w, big.max_area = hint
    return big


def _per_tile(fn):
    """the oracle's rows of both tiles, tile after tile: name -> [13]"""
    lab, _, counts = scene()
    out = {}
    for f in range(len(counts)):
        for k, v in fn(f, lab[f]).items():
            out.setdefault(k, []).append(np.asarray(v, float))
    res = {k: np.concatenate(v) for k, v in out.items()}
    assert all(len(v) == sum(counts) for v in res.values())
    return res


def compare(names, got, want, exact=()):
    got = np.asarray(got, float)
    assert got.shape == (len(want[names[0]]), len(names)), got.shape
    for j, name in enumerate(names):
        g, r = got[:, j], np.asarray(want[name], float)
        if name in exact:
            assert np.array_equal(np.nan_to_num(g, nan=-1), np.nan_to_num(r, nan=-1)), (name, g, r)
            continue
        if "ZernikePhase" in name:  # the phase of a vanishing moment is rounding noise (tests/test_gpu_edge_cases.py, _run_both)
            m = names.index(name.replace("ZernikePhase", "ZernikeMagnitude"))
            keep = ~((np.abs(got[:, m]) < 1e-9) & (np.abs(np.asarray(want[names[m]], float)) < 1e-9))
            g, r = g[keep], r[keep]
        _close(g, r, name)


def as_dict(names, block):
    return {n: block[:, j] for j, n in enumerate(names)}


INTENSITY_EXACT = ("Intensity_MinIntensity", "Intensity_MaxIntensity", "Intensity_IntegratedIntensity", "Location_MaxIntensity_X",
                   "Location_MaxIntensity_Y")
SIZESHAPE_EXACT = ("Area", "BoundingBoxArea", "BoundingBoxMaximum_X", "BoundingBoxMaximum_Y", "BoundingBoxMinimum_X", "BoundingBoxMinimum_Y",
                   "EulerNumber", "ConvexArea")
COLOC_NAMES = ["Correlation_Pearson", "Correlation_Slope", "Correlation_Manders_1", "Correlation_Manders_2", "Correlation_RWC_1",
               "Correlation_RWC_2", "Correlation_Costes_1", "Correlation_Costes_2"]
COLOC_COLS = dict(pearson=0, manders_fold=2, rwc=4, costes=6)


# ------------------------------------------------------------------------------------- the oracles, once per family and type
@functools.lru_cache(maxsize=None)
def oracle_intensity(mode, ch, edge):
    from oracle import cp_measure_restated as cpm

    res = _per_tile(lambda f, lab: cpm.get_intensity(lab, planes_of(mode)[f, ch], edge_measurements=edge))
    # The reference measures one full-frame binary mask per object (oracle/aliby_extract.py), and an all-False mask has no row at
    # all: the kernel writes NaN there (tests/test_gpu_edge_cases.py, test_label_values_up_to_uint16_limit).  Called on a label image
    # that skips a value, the oracle leaves the zeros it initialises the five edge columns with in that row; they are no measurement.
    absent = np.concatenate([np.bincount(scene()[0][f].ravel(), minlength=n + 1)[1:n + 1] == 0 for f, n in enumerate(scene()[2])])
    assert absent.sum() == 1 and all(np.isnan(v[absent]).all() or "Edge" in k for k, v in res.items())
    return {k: np.where(absent, np.nan, v) for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def oracle_sizeshape():
    from oracle import cp_measure_restated as cpm

    return _per_tile(lambda f, lab: cpm.get_sizeshape(lab))


@functools.lru_cache(maxsize=None)
def oracle_feret():
    from oracle import cp_measure_restated as cpm

    return _per_tile(lambda f, lab: cpm.get_feret(lab))


@functools.lru_cache(maxsize=None)
def oracle_mec():
    from oracle import zernike_restated as zr

    lab, _, counts = scene()
    rows = []
    for f, n in enumerate(counts):
        idx = np.arange(1, n + 1)
        centres, radii = zr.minimum_enclosing_circle(lab[f], idx)
        rows.append(np.column_stack([np.asarray(centres, float).reshape(n, 2), np.asarray(radii, float)]))
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def oracle_zernike(mode, ch):
    from oracle import zernike_restated as zr

    if ch is None:
        return _per_tile(lambda f, lab: zr.get_zernike(lab))
    return _per_tile(lambda f, lab: zr.get_radial_zernikes(lab, planes_of(mode)[f, ch]))


@functools.lru_cache(maxsize=None)
def oracle_texture(mode, ch):
    from oracle import texture_restated as tx

    return _per_tile(lambda f, lab: tx.get_texture(lab, planes_of(mode)[f, ch]))


@functools.lru_cache(maxsize=None)
def oracle_radial(mode, ch, bin_count, maximum_radius):
    from oracle import radial_restated as rr

    kw = dict(bin_count=bin_count) if maximum_radius is None else dict(bin_count=bin_count, scaled=False, maximum_radius=maximum_radius)
    return _per_tile(lambda f, lab: rr.get_radial_distribution(lab, planes_of(mode)[f, ch], **kw))


@functools.lru_cache(maxsize=None)
def oracle_coloc(mode):
    """One full-frame binary mask per object, as the reference evaluates it (tests/test_gpu_features.py)."""
    from oracle import cp_measure_restated as cpm

    def tile(f, lab):
        p = planes_of(mode)[f]
        ref = {}
        for L in range(1, int(lab.max()) + 1):
            one = (lab == L).astype(np.uint16)
            for fn in cpm.get_correlation_measurements().values():
                for k, v in fn(p[0], p[1], one).items():
                    ref.setdefault(k, []).append(v[0] if len(v) else np.nan)
        return ref

    return _per_tile(tile)


@functools.lru_cache(maxsize=None)
def oracle_cell(mode, ch):
    lab, _, counts = scene()
    want, meta = cell_ref.cell_metrics_batch(lab, planes_of(mode), ch, counts)
    for m in meta:  # the precondition of cell_ref.check: neither axis rounding near a tie
        assert m["n"] == 0 or m["all_top"] or (m["tie"] >= cell_ref.TIE_MARGIN and m["sqrt_tie"] >= cell_ref.TIE_MARGIN), m
    return want, meta


# ------------------------------------------------------------------------------------------------------------------ the tests
def test_rungs_reach_every_form():
    """The table of the module docstring, recomputed: every site has a rung in each of its three forms."""
    seen = {}
    for name, hint in RUNGS.items():
        for site, form in forms(*(hint or (20, 20, 400))).items():
            seen.setdefault(site, {}).setdefault(form, name)
    assert len(seen) == 10
    for site, by_form in seen.items():
        assert set(by_form) == {"lds", "attr", "glob"}, (site, by_form)
    f = forms(*RUNGS["96x96"])
    assert f["k_coloc"] == f["k_ranks"] == "glob" and f["k_cell"] == f["k_shape_edt"] == f["k_radial_geometry"] == "attr"
    assert forms(*RUNGS["64x64"])["k_coloc"] == "attr" and forms(*RUNGS["250x250"])["k_shape_core"] == "attr"
    assert forms(*RUNGS["500x20"])["k_shape_hull"] == "attr" and forms(*RUNGS["1500x20"])["k_mec"] == "attr"
    assert forms(*RUNGS["1500x20"])["k_shape_hull"] == "glob" and forms(*RUNGS["2600x20"])["k_mec"] == "glob"
    assert forms(*RUNGS["180x180"])["k_texture"] == "attr" and forms(*RUNGS["250x250"])["k_intensity"] == "attr"
    assert all(v == "glob" for k, v in forms(*RUNGS["400x400"]).items() if k not in ("k_shape_hull", "k_mec"))


@rungs
@pytest.mark.parametrize("mode", MODES)
def test_intensity(engine, rung, mode):
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, mode)
    big = hinted(tab, RUNGS[rung])
    for edge in (True, False):
        names = feat.intensity_names(edge)
        for ch in range(2):
            out = engine.new_output(tab.n_obj, len(names))
            engine.intensity(dl, dp, dt, ch, big, out, 0, edge_measurements=edge)
            torch.cuda.synchronize()
            compare(names, out.cpu().numpy(), oracle_intensity(mode, ch, edge), exact=INTENSITY_EXACT if mode == "u16" else ())


@rungs
def test_sizeshape_and_feret(engine, rung):
    import torch
    from aliby_amd.extraction import features as feat

    dl, _, _, tab = device(engine, "u16")
    big = hinted(tab, RUNGS[rung])
    names = feat.sizeshape_names()
    out = engine.new_output(tab.n_obj, len(names))
    engine.sizeshape(dl, big, out, 0)
    fer = engine.new_output(tab.n_obj, 2)
    engine.feret(dl, big, fer, 0)
    torch.cuda.synchronize()
    compare(names, out.cpu().numpy(), oracle_sizeshape(), exact=SIZESHAPE_EXACT)
    compare(["MinFeretDiameter", "MaxFeretDiameter"], fer.cpu().numpy(), oracle_feret())


@rungs
@pytest.mark.parametrize("mode", MODES)
def test_mec_and_zernike(engine, rung, mode):
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, mode)
    big = hinted(tab, RUNGS[rung])
    mec = engine.mec(dl, big).cpu().numpy()[: tab.n_obj]
    want = oracle_mec()
    present = tab.host["area"] > 0
    # (the rule of tests/test_gpu_features.py; the circle of an absent label is not defined and no kernel reads it)
    assert np.allclose(mec[present, 2], want[present, 2], rtol=1e-9), (mec, want)
    assert np.allclose(mec[present, :2], want[present, :2], rtol=1e-9, atol=1e-9)
    out = engine.new_output(tab.n_obj, 30)
    engine.zernike(dl, None, 0, 0, big, out, 0, weighted=False)
    torch.cuda.synchronize()
    compare(feat.zernike_names(), out.cpu().numpy(), oracle_zernike(mode, None))
    for ch in range(2):
        out = engine.new_output(tab.n_obj, 60)
        engine.zernike(dl, dp, dt, ch, big, out, 0, weighted=True)
        torch.cuda.synchronize()
        compare(feat.radial_zernike_names(), out.cpu().numpy(), oracle_zernike(mode, ch))


@rungs
@pytest.mark.parametrize("mode", MODES)
def test_texture(engine, rung, mode):
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, mode)
    big = hinted(tab, RUNGS[rung])
    for ch in range(2):
        out = engine.new_output(tab.n_obj, 52)
        engine.texture(dl, dp, dt, ch, big, out, 0)
        torch.cuda.synchronize()
        compare(feat.texture_names(3, 256), out.cpu().numpy(), oracle_texture(mode, ch))


@rungs
@pytest.mark.parametrize("mode", MODES)
def test_radial_geometry_and_distribution(engine, rung, mode):
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, mode)
    big = hinted(tab, RUNGS[rung])
    for bin_count, maximum_radius in ((4, None), (3, 6)):
        names = feat.radial_distribution_names(bin_count, scaled=maximum_radius is None)
        for ch in range(2):
            out = engine.new_output(tab.n_obj, len(names))
            if maximum_radius is None:
                engine.radial_distribution(dl, dp, dt, ch, big, out, 0, bin_count=bin_count)
            else:
                engine.radial_distribution(dl, dp, dt, ch, big, out, 0, bin_count=bin_count, scaled=False, maximum_radius=maximum_radius)
            torch.cuda.synchronize()
            compare(names, out.cpu().numpy(), oracle_radial(mode, ch, bin_count, maximum_radius))


@rungs
@pytest.mark.parametrize("mode", MODES)
def test_cell_metrics(engine, rung, mode):
    dl, dp, dt, tab = device(engine, mode)
    big = hinted(tab, RUNGS[rung])
    for ch in range(2):
        want, meta = oracle_cell(mode, ch)
        got = engine.cell_metrics(dl, dp, dt, ch, big).cpu().numpy()
        cell_ref.check(got, want, meta, f"rung {rung}, channel {ch}", mode)
    mask_only = engine.cell_metrics(dl, None, dt, 0, big).cpu().numpy()
    cell_ref.check(mask_only, want, meta, f"rung {rung}, mask only", mode, pixels=False)


@rungs
@pytest.mark.parametrize("mode", MODES)
def test_ranks_and_coloc(engine, rung, mode):
    import torch

    dl, dp, dt, tab = device(engine, mode)
    big = hinted(tab, RUNGS[rung])
    out = engine.new_output(tab.n_obj, 8)
    engine.coloc(dl, dp, dt, 0, 1, big, out, COLOC_COLS)  # (rwc: the rank planes of both channels through k_ranks, same table)
    torch.cuda.synchronize()
    assert set(big._ranks[("ranks", dp.data_ptr())]["done"]) == {0, 1}
    compare(COLOC_NAMES, out.cpu().numpy(), oracle_coloc(mode))


# ---------------------------------------------------------------------------------------- more objects than workgroups
STRIDE_HINTS = {"700x24": (700, 24, 16384), "700x24_area32768": (700, 24, 32768), "2600x4": (2600, 4, 4096)}


@functools.lru_cache(maxsize=None)
def stride_scene():
    """One tile of 128 x 128 with 600 objects, 2 x 2 and 3 x 3 in turn, on a grid of pitch 5."""
    lab = np.zeros((1, 128, 128), np.uint16)
    for k in range(600):
        y, x = 5 * (k // 25) + 1, 5 * (k % 25) + 1
        s = 2 + (k + k // 25) % 2
        lab[0, y:y + s, x:x + s] = k + 1
    px = np.random.default_rng(5).integers(100, 60000, size=(1, 2, 128, 128)).astype(np.uint16)
    return lab, px


def test_stride_hints_put_every_site_in_the_global_form():
    """... except k_shape_core, whose global form takes (h + 4)(w + 4) > 96 KiB per workgroup: about 0.5 GB for 512 of them at
    the smallest box that still holds the other hints.  Its stride loop is not covered here.  k_intensity and k_texture need
    max_area 32768 (132 KiB; 16 800 + 128 KiB), at which k_coloc and k_ranks would take 512 x 512 KiB = 256 MiB: they get the
    hint of their own.  The largest scratch any launch of the test asks for is 512 x 256 KiB = 128 MiB (k_coloc at 16384)."""
    a, b, c = (forms(*STRIDE_HINTS[k]) for k in ("700x24", "700x24_area32768", "2600x4"))
    for site in ("k_ranks", "k_coloc", "k_cell", "k_shape_edt", "k_shape_hull", "k_radial_geometry"):
        assert a[site] == "glob", site
    assert b["k_intensity"] == b["k_texture"] == "glob" and c["k_mec"] == "glob" and a["k_shape_core"] != "glob"
    worst = max(min(600, 512) * working_sets(*STRIDE_HINTS[k])[site][0] for k, sites in
                (("700x24", ("k_ranks", "k_coloc", "k_cell", "k_shape_edt", "k_shape_hull", "k_radial_geometry", "k_mec")),
                 ("700x24_area32768", ("k_intensity", "k_texture")), ("2600x4", ("k_mec", "k_shape_hull"))) for site in sites)
    assert worst < 256 * KIB * KIB, worst


@pytest.mark.parametrize("mode", MODES)
def test_global_form_strides_over_600_objects(engine, mode):
    """600 rows through at most 512 workgroups: every workgroup of the first 88 takes a second object.  Compared with the run of
    the same input under the table's true limits (the LDS form that the rest of the suite checks against the oracle; the oracle on
    600 objects takes too long here), by the same rules.  k_shape_core stays in LDS (see above): not covered."""
    import torch
    from aliby_amd.extraction import features as feat
    from aliby_amd.extraction.engine import to_device_planes, to_device_u16

    lab, px = stride_scene()
    if mode == "f32":
        px = (px.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    dl = to_device_u16(lab)
    dp, dt = to_device_planes(px)
    tab = engine.object_table(dl)
    assert tab.n_obj == 600 and (tab.max_h, tab.max_w, tab.max_area) == (3, 3, 9) and (tab.host["area"] > 0).all()

    def run(hint_a, hint_b, hint_c):
        res = {}
        ta, tb, tc = hinted(tab, hint_a), hinted(tab, hint_b), hinted(tab, hint_c)
        for edge in (True, False):
            out = engine.new_output(600, len(feat.intensity_names(edge)))
            engine.intensity(dl, dp, dt, 1, tb, out, 0, edge_measurements=edge)
            res["intensity", edge] = out
        out = engine.new_output(600, 52)
        engine.texture(dl, dp, dt, 0, tb, out, 0, scale=1)  # (scale 1: a 2 x 2 object has pixel pairs)
        res["texture"] = out
        out = engine.new_output(600, 78)
        engine.sizeshape(dl, ta, out, 0)
        res["sizeshape"] = out
        out = engine.new_output(600, 2)
        engine.feret(dl, ta, out, 0)
        res["feret"] = out
        res["mec"] = engine.mec(dl, tc)
        out = engine.new_output(600, 60)
        engine.zernike(dl, dp, dt, 0, tc, out, 0, weighted=True)
        res["radial_zernikes"] = out
        out = engine.new_output(600, 12)
        engine.radial_distribution(dl, dp, dt, 1, ta, out, 0, bin_count=4)
        res["radial_distribution"] = out
        res["cell"] = engine.cell_metrics(dl, dp, dt, 0, ta)
        out = engine.new_output(600, 8)
        engine.coloc(dl, dp, dt, 0, 1, ta, out, COLOC_COLS)
        res["coloc"] = out
        torch.cuda.synchronize()
        return {k: v.cpu().numpy()[:600] for k, v in res.items()}

    want = run(None, None, None)
    got = run(STRIDE_HINTS["700x24"], STRIDE_HINTS["700x24_area32768"], STRIDE_HINTS["2600x4"])
    for edge in (True, False):
        names = feat.intensity_names(edge)
        compare(names, got["intensity", edge], as_dict(names, want["intensity", edge]), exact=INTENSITY_EXACT if mode == "u16" else ())
    names = feat.texture_names(1, 256)
    assert np.isfinite(want["texture"]).any()
    compare(names, got["texture"], as_dict(names, want["texture"]))
    names = feat.sizeshape_names()
    compare(names, got["sizeshape"], as_dict(names, want["sizeshape"]), exact=SIZESHAPE_EXACT)
    compare(["MinFeretDiameter", "MaxFeretDiameter"], got["feret"], as_dict(["MinFeretDiameter", "MaxFeretDiameter"], want["feret"]))
    assert np.allclose(got["mec"][:, :3], want["mec"][:, :3], rtol=1e-9, atol=1e-9)
    names = feat.radial_zernike_names()
    compare(names, got["radial_zernikes"], as_dict(names, want["radial_zernikes"]))
    names = feat.radial_distribution_names(4)
    compare(names, got["radial_distribution"], as_dict(names, want["radial_distribution"]))
    meta = [dict(n=int(a), n_top=int(math.ceil(int(a) * 0.025))) for a in tab.host["area"]]
    cell_ref.check(got["cell"], want["cell"], meta, "600 objects, global form against the LDS form", mode)
    compare(COLOC_NAMES, got["coloc"], as_dict(COLOC_NAMES, want["coloc"]))
