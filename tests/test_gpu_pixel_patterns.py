"""
The per-channel 2-D feature kernels on flat, dark and tied pixels (tests/pixel_patterns.py): k_intensity against the exact
reference of tests/intensity_ref.py, k_texture, k_radial_stats and the weighted Zernike kernel against their oracles by the
project's rule (`compare` of tests/test_gpu_object_forms.py: 1e-4 relative / 1e-8 absolute, NaN only against NaN), k_ranks,
k_coloc and k_coloc_pairs against the per-object full-frame oracle.

Every test runs for uint16 and unit-float32 pixels and under three table hints of tests/test_gpu_object_forms.py:
    "true"      64-thread workgroups; k_intensity stages by ballot
    "96x96"     128 threads; k_intensity stages by atomics; k_coloc and k_ranks in the global form
    "400x400"   every kernel in the global form
(k_coloc_pairs has no global form: where the hint exceeds its LDS budget it declines, which is asserted, and it runs under the
table's true limits.)

tests/test_cpu_intensity_ref.py checks the preconditions: the reference against the oracle, several maxima where the tie rule is
tested, no Costes probe near a sign change.  Every oracle is computed once per family, pixel type and parameter set.
"""
import functools
import warnings

import numpy as np
import pytest

from tests import coloc3d_ref
from tests import intensity_ref
from tests import pixel_patterns as pp
from tests.test_gpu_object_forms import COLOC_COLS, COLOC_NAMES, RUNGS, compare, hinted

pytestmark = pytest.mark.gpu

HINTS = ("true", "96x96", "400x400")
PAIRS = [(0, 1), (0, 2), (1, 2)]
SCALE_MAX = {"u16": (255.0, 65535.0), "f32": (255.0,)}
hints = pytest.mark.parametrize("hint", HINTS)
modes = pytest.mark.parametrize("mode", pp.MODES)

_DEVICE = {}


def device(engine, name, mode):
    """-> (labels, planes, dtype code, object table with its true limits) of a scene on the GPU, made once per pixel type"""
    if (name, mode) not in _DEVICE:
        from aliby_amd.extraction.engine import to_device_planes, to_device_u16

        lab, _, counts = pp.SCENES[name]()
        dl = to_device_u16(lab)
        dp, dt = to_device_planes(pp.planes(name, mode))
        tab = engine.object_table(dl)
        assert tab.n_obj == sum(counts) and tab.max_h <= 20 and tab.max_w <= 20
        _DEVICE[name, mode] = (dl, dp, dt, tab)
    return _DEVICE[name, mode]


def _quiet(fn):
    """The oracles divide 0 by 0 on these inputs, on purpose."""
    def run(*a, **k):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fn(*a, **k)
    return run


def _per_tile(fn):
    lab, _, counts = pp.tiles()
    out = {}
    for f in range(len(counts)):
        for k, v in _quiet(fn)(f, lab[f]).items():
            out.setdefault(k, []).append(np.asarray(v, float))
    res = {k: np.concatenate(v) for k, v in out.items()}
    assert all(len(v) == sum(counts) for v in res.values())
    return res


@functools.lru_cache(maxsize=None)
def reference_intensity(name, mode, ch, edge):
    lab, _, counts = pp.SCENES[name]()
    return intensity_ref.intensity_batch(lab, pp.planes(name, mode), ch, counts, edge)


@functools.lru_cache(maxsize=None)
def oracle_texture(mode, ch, scale):
    from oracle import texture_restated as tx

    return _per_tile(lambda f, lab: tx.get_texture(lab, pp.planes("tiles", mode)[f, ch], scale=scale, gray_levels=256))


@functools.lru_cache(maxsize=None)
def oracle_radial(mode, ch, bin_count, maximum_radius):
    from oracle import radial_restated as rr

    kw = dict(bin_count=bin_count) if maximum_radius is None else dict(bin_count=bin_count, scaled=False, maximum_radius=maximum_radius)
    return _per_tile(lambda f, lab: rr.get_radial_distribution(lab, pp.planes("tiles", mode)[f, ch], **kw))


@functools.lru_cache(maxsize=None)
def oracle_zernike(mode, ch):
    from oracle import zernike_restated as zr

    return _per_tile(lambda f, lab: zr.get_radial_zernikes(lab, pp.planes("tiles", mode)[f, ch]))


@functools.lru_cache(maxsize=None)
def oracle_coloc(mode, pair, scale_max):
    """One full-frame binary mask per object, as the reference pipeline evaluates it; the absent label is a row of NaN."""
    lab, _, counts = pp.tiles()
    px = pp.planes("tiles", mode)
    a, b = pair
    rows = np.concatenate([_quiet(coloc3d_ref.coloc3d)(lab[f][None], px[f, a][None], px[f, b][None], n, scale_max=scale_max) for f, n in enumerate(counts)])
    assert list(coloc3d_ref.NAMES) == COLOC_NAMES
    return {k: rows[:, j] for j, k in enumerate(COLOC_NAMES)}


# ------------------------------------------------------------------------------------------------------------------ the tests
@hints
@modes
def test_intensity(engine, hint, mode):
    """Every column by tests/intensity_ref.check, edge on and off, every channel, on both pattern tiles and on the frame that is
    one object (where the five edge columns are 0)."""
    import torch

    for name in ("tiles", "full_frame"):
        dl, dp, dt, tab = device(engine, name, mode)
        big = hinted(tab, RUNGS[hint])
        for edge in (True, False):
            order = intensity_ref.names(edge)
            for ch in range(3):
                out = engine.new_output(tab.n_obj, len(order))
                engine.intensity(dl, dp, dt, ch, big, out, 0, edge_measurements=edge)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                want, meta = reference_intensity(name, mode, ch, edge)
                intensity_ref.check(got, want, meta, f"{name}, hint {hint}, channel {ch}, edge {edge}", mode, edge)
                if name == "full_frame" and edge:
                    assert meta[0]["n_edge"] == 0 and (got[0, 5:10] == 0.0).all(), got[0, 5:10]


@hints
@modes
def test_texture(engine, hint, mode):
    """256 levels, at scale 3 and at scale 1 (a tiny object has pixel pairs only at scale 1)."""
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, "tiles", mode)
    big = hinted(tab, RUNGS[hint])
    for scale in (3, 1):
        for ch in range(2):
            out = engine.new_output(tab.n_obj, 52)
            engine.texture(dl, dp, dt, ch, big, out, 0, scale=scale, gray_levels=256)
            torch.cuda.synchronize()
            compare(feat.texture_names(scale, 256), out.cpu().numpy(), oracle_texture(mode, ch, scale))


@hints
@modes
def test_radial_distribution(engine, hint, mode):
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, "tiles", mode)
    big = hinted(tab, RUNGS[hint])
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


@hints
@modes
def test_weighted_zernikes(engine, hint, mode):
    import torch
    from aliby_amd.extraction import features as feat

    dl, dp, dt, tab = device(engine, "tiles", mode)
    big = hinted(tab, RUNGS[hint])
    for ch in range(2):
        out = engine.new_output(tab.n_obj, 60)
        engine.zernike(dl, dp, dt, ch, big, out, 0, weighted=True)
        torch.cuda.synchronize()
        compare(feat.radial_zernike_names(), out.cpu().numpy(), oracle_zernike(mode, ch))


@hints
@modes
def test_ranks_and_coloc(engine, hint, mode):
    """The four metrics of the three pairs, pair by pair (k_ranks, k_coloc) and in one launch (k_coloc_pairs), against the oracle;
    the two launches agree to 1e-9."""
    import torch

    dl, dp, dt, tab = device(engine, "tiles", mode)
    for scale_max in SCALE_MAX[mode]:
        big = hinted(tab, RUNGS[hint])
        per_pair = []
        for a, b in PAIRS:
            out = engine.new_output(tab.n_obj, 8)
            engine.coloc(dl, dp, dt, a, b, big, out, COLOC_COLS, scale_max=scale_max)
            torch.cuda.synchronize()
            per_pair.append(out.cpu().numpy())
        spec = [(pr, {k: 8 * i + c for k, c in COLOC_COLS.items()}) for i, pr in enumerate(PAIRS)]
        allout = engine.new_output(tab.n_obj, 8 * len(PAIRS))
        launched = engine.coloc_pairs(dl, dp, dt, spec, big, allout, scale_max=scale_max)
        cap = 64
        while cap < big.max_area:
            cap <<= 1
        assert launched == (3 * cap * 4 * 2 <= 144 * 1024), (hint, cap)  # (the kernel's LDS budget: feat_coloc.hip)
        if not launched:
            assert engine.coloc_pairs(dl, dp, dt, spec, hinted(tab, None), allout, scale_max=scale_max)
        torch.cuda.synchronize()
        allgot = allout.cpu().numpy()
        for i, pair in enumerate(PAIRS):
            want = oracle_coloc(mode, pair, scale_max)
            tag = f"pair {pair}, scale_max {scale_max}"
            try:
                compare(COLOC_NAMES, per_pair[i], want)
                compare(COLOC_NAMES, allgot[:, 8 * i: 8 * i + 8], want)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from e
            assert np.allclose(allgot[:, 8 * i: 8 * i + 8], per_pair[i], rtol=1e-9, atol=1e-12, equal_nan=True), tag
        same = per_pair[1]  # identical channels: Pearson and slope 1 where defined, RWC equal to Manders
        ok = ~np.isnan(same[:, 0])
        assert ok.any() and np.allclose(same[ok, :2], 1.0, rtol=1e-12) and np.allclose(same[:, 2:4], same[:, 4:6], rtol=1e-12, equal_nan=True)

