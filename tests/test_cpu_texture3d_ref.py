"""
Pins tests/texture3d_ref.py, the reference that tests/test_gpu_texture3d.py compares `FeatureEngine.texture3d` with, so that a
misreading shared by kernel and reference cannot hide (no GPU needed):

  * on a stack of one plane the four in-plane directions equal the oracle's 2-D `get_texture` bit for bit, the other nine are NaN;
  * the matrices equal a brute-force loop over voxel pairs, and all 13 statistics equal textbook double sums over a dense
    256 x 256 matrix written out here, sharing no code with the reference;
  * permuting the axes of volume and pixels permutes the direction blocks and changes nothing else (this pins the handling of
    the directions without pinning their order, which is mahotas' as recalled);
  * the 169 names.
"""
import itertools
import warnings

import numpy as np
import pytest

from tests import texture3d_ref as ref
from tests.coloc3d_ref import irregular, unit_float


@pytest.fixture(autouse=True)
def _quiet_numpy():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


# ------------------------------------------------------------------------------------------------ 1. one plane = the 2-D oracle
@pytest.mark.parametrize("mode,scale,gl", [("u16", 3, 256), ("f32_unit", 3, 256), ("u16", 1, 64)])
def test_a_stack_of_one_plane_equals_the_2d_oracle_bit_for_bit(mode, scale, gl):
    from oracle.texture_restated import HARALICK, get_texture

    vol, n, px = irregular(5, (1, 64, 72))
    px = px[0] if mode == "u16" else unit_float(px[0])
    got = ref.texture3d(vol, px, n, scale, gl)
    want = get_texture(vol[0], px[0], scale, gl)
    assert got.shape == (n, 169) and n >= 6
    finite = 0
    for d3 in range(13):
        block = got[:, d3 * 13:(d3 + 1) * 13]
        if d3 not in ref.IN_PLANE:
            assert np.isnan(block).all(), d3
            continue
        assert ref.DELTAS_3D[d3][0] == 0
        for k, h in enumerate(HARALICK):
            w = want[f"{h}_{scale}_{ref.IN_PLANE[d3]:02d}_{gl}"]
            assert np.array_equal(block[:, k].view(np.int64), w.view(np.int64)), (d3, h)  # the same bits, NaN included
        finite += int(np.isfinite(block).sum())
    assert finite > 4 * 13 * n // 2  # the comparison was about numbers, not NaN


# ------------------------------------------------------------------------------------------------ 2. brute force + textbook sums
def _brute_matrix(volume, grey, label, delta, scale):
    """Dense symmetric 256 x 256 count matrix of the pairs (p, p + scale * delta), both voxels inside the label's bounding box,
    voxels of other labels and grey level 0 dropped: one Python loop over the voxels, no slicing tricks."""
    zs, ys, xs = np.nonzero(volume == label)
    lo = (zs.min(), ys.min(), xs.min())
    hi = (zs.max(), ys.max(), xs.max())
    m = np.zeros((256, 256), np.int64)
    for z in range(lo[0], hi[0] + 1):
        for y in range(lo[1], hi[1] + 1):
            for x in range(lo[2], hi[2] + 1):
                z2, y2, x2 = z + scale * delta[0], y + scale * delta[1], x + scale * delta[2]
                if not (lo[0] <= z2 <= hi[0] and lo[1] <= y2 <= hi[1] and lo[2] <= x2 <= hi[2]):
                    continue
                if volume[z, y, x] != label or volume[z2, y2, x2] != label:
                    continue
                a, b = int(grey[z, y, x]), int(grey[z2, y2, x2])
                if a == 0 or b == 0:
                    continue
                m[a, b] += 1
                m[b, a] += 1
    return m, int(max(grey[volume == label].max(), 0)) + 1


def _textbook(m, maxv):
    """Haralick's 13 from a dense count matrix by their defining double sums (entropies in bits; SumVariance about SumAverage;
    DifferenceVariance = the variance of the vector p_{x-y}(0 .. maxv - 1), mahotas' reading)."""
    T = float(m.sum())
    p = m / T
    n = p.shape[0]
    i, j = np.mgrid[:n, :n]
    px = p.sum(axis=1)
    mu = float((np.arange(n) * px).sum())
    var = float((((np.arange(n) - mu) ** 2) * px).sum())
    lg = lambda a: np.log2(np.where(a > 0, a, 1.0))
    psum = np.asarray([p[(i + j) == k].sum() for k in range(2 * n - 1)])
    pdif = np.asarray([p[np.abs(i - j) == k].sum() for k in range(n)])
    sa = float((np.arange(2 * n - 1) * psum).sum())
    hxy = float(-(p * lg(p)).sum())
    hx = float(-(px * lg(px)).sum())
    pp = np.outer(px, px)
    hxy1 = float(-(p * lg(pp)).sum())
    hxy2 = float(-(pp * lg(pp)).sum())
    return np.asarray([
        (p ** 2).sum(),
        (((i - j) ** 2) * p).sum(),
        1.0 if var == 0 else ((i * j * p).sum() - mu * mu) / var,
        var,
        (p / (1.0 + (i - j) ** 2)).sum(),
        sa,
        (((np.arange(2 * n - 1) - sa) ** 2) * psum).sum(),
        -(psum * lg(psum)).sum(),
        hxy,
        pdif[:maxv].var(),
        -(pdif * lg(pdif)).sum(),
        (hxy - hxy1) if hx == 0 else (hxy - hxy1) / hx,
        np.sqrt(max(0.0, 1.0 - np.exp(-2.0 * (hxy2 - hxy)))),
    ])


@pytest.mark.parametrize("scale,gl", [(1, 256), (2, 256), (2, 64)])
def test_matrices_equal_a_brute_force_loop_and_statistics_equal_textbook_sums(scale, gl):
    vol, n, px = irregular(3, (6, 22, 26), n_seeds=4)
    grey = ref.grey_levels(px[1], gl)
    got = ref.texture3d(vol, px[1], n, scale, gl)
    crops = ref.object_crops(vol, grey, n)
    compared = 0
    for lab in range(1, n + 1):
        for d, delta in enumerate(ref.DELTAS_3D):
            m, maxv = _brute_matrix(vol, grey, lab, delta, scale)
            c = ref.cooccurrence3d(crops[lab - 1], delta, scale)
            c[0] = 0
            c[:, 0] = 0  # (the reference leaves grey level 0 to haralick_features)
            assert c.shape == (maxv, maxv) and np.array_equal(c, m[:maxv, :maxv]) and m.sum() == c.sum(), (lab, d)
            block = got[lab - 1, d * 13:(d + 1) * 13]
            if m.sum() == 0:
                assert np.isnan(block).all(), (lab, d)
                continue
            # double sums over 65536 cells against numpy dot products over maxv^2: 1e-9 is four orders above their rounding
            np.testing.assert_allclose(block, _textbook(m, maxv), rtol=1e-9, atol=1e-12, err_msg=f"label {lab} direction {d}")
            compared += 1
    assert compared >= 13 * n // 2


# ------------------------------------------------------------------------------------------------ 3. axes
def test_permuting_the_axes_permutes_the_direction_blocks_and_nothing_else():
    vol, n, px = irregular(8, (9, 20, 24), n_seeds=5)
    base = ref.texture3d(vol, px[0], n, 2)
    assert np.isfinite(base).sum() > base.size // 2
    index = {d: k for k, d in enumerate(ref.DELTAS_3D)}
    assert len(index) == 13 and all(tuple(-c for c in d) not in index for d in index)  # one half of the 26 neighbours
    for perm in itertools.permutations(range(3)):
        got = ref.texture3d(np.transpose(vol, perm), np.transpose(px[0], perm), n, 2)
        seen = set()
        for k, d in enumerate(ref.DELTAS_3D):
            moved = tuple(d[a] for a in perm)  # the same pair of voxels, named on the permuted axes
            k2 = index.get(moved, index.get(tuple(-c for c in moved)))
            assert k2 is not None and k2 not in seen
            seen.add(k2)
            assert np.array_equal(got[:, k2 * 13:(k2 + 1) * 13], base[:, k * 13:(k + 1) * 13], equal_nan=True), (perm, k, k2)
        assert len(seen) == 13


def test_a_plate_thinner_than_the_scale_has_numbers_in_its_plane_only():
    vol, n, px, boxes = ref.budget_volume(24576)
    assert boxes[-1] == 9 and vol.shape[0] > 3
    tiny = np.where(vol == 5, 1, 0).astype(np.uint16)
    one = ref.texture3d(tiny, px[0], 1, 1)[0].reshape(13, 13)
    in_plane = [k for k, d in enumerate(ref.DELTAS_3D) if d[0] == 0]
    assert sorted(in_plane) == sorted(ref.IN_PLANE) and np.isfinite(one[in_plane]).all()
    assert np.isnan(np.delete(one, in_plane, axis=0)).all()
    assert np.isnan(ref.texture3d(tiny, px[0], 1, 3)).all()


# ------------------------------------------------------------------------------------------------ 4. names
def test_names_are_169_unique_and_direction_major():
    from aliby_amd.extraction import features as feat
    from oracle.texture_restated import HARALICK

    names = feat.texture3d_names(3, 256)
    assert len(names) == 169 == ref.N_COLS and len(set(names)) == 169
    assert names[:13] == [f"{h}_3_00_256" for h in HARALICK] and names[13] == "AngularSecondMoment_3_01_256" and names[-1] == "InfoMeas2_3_12_256"
    assert feat.texture3d_names(2, 64)[14] == "Contrast_2_01_64"
    # the four in-plane blocks carry the 2-D family's statistic names
    two = feat.texture_names(3, 256)
    for d3, d2 in ref.IN_PLANE.items():
        assert [s.split("_")[0] for s in names[d3 * 13:(d3 + 1) * 13]] == [s.split("_")[0] for s in two[d2 * 13:(d2 + 1) * 13]]
