"""
Pins the float32 restatement of cellpose's 3-D dynamics (tests/cellpose3d_ref.py) to the primitives cellpose itself uses: PyTorch's
grid_sample / max_pool3d and scipy's binary_fill_holes (CPU; no GPU needed).  The GPU kernels are then tested against the
restatement bit for bit (tests/test_gpu_cellpose3d.py).
"""
import numpy as np
import pytest
from scipy import ndimage as ndi

from aliby_amd import synth
from tests import cellpose3d_ref as ref


def _steps_interp_torch(dPs, inds, niter):
    """cellpose's steps_interp for a 3-D field, literally: grid_sample(align_corners=False) + clamp, float32 on the CPU."""
    import torch

    shape = dPs.shape[1:]
    ndim = 3
    pt = torch.zeros((1, 1, 1, len(inds[0]), ndim), dtype=torch.float32)
    im = torch.zeros((1, ndim, *shape), dtype=torch.float32)
    for n in range(ndim):  # grid_sample's (x, y, z) order
        pt[..., n] = torch.from_numpy(inds[ndim - n - 1].astype(np.float32))
        im[0, ndim - n - 1] = torch.from_numpy(dPs[n])
    sz = np.array(shape)[::-1].astype("float") - 1
    for k in range(ndim):
        im[:, k] *= 2.0 / sz[k]
        pt[..., k] /= sz[k]
    pt *= 2
    pt -= 1
    for _ in range(niter):
        dPt = torch.nn.functional.grid_sample(im, pt, align_corners=False)
        for k in range(ndim):
            pt[..., k] = torch.clamp(pt[..., k] + dPt[:, k], -1.0, 1.0)
    pt += 1
    pt *= 0.5
    for k in range(ndim):
        pt[..., k] *= sz[k]
    return np.stack([pt[0, 0, 0, :, ndim - 1 - d].numpy() for d in range(3)])  # (z, y, x)


def _volume(seed, shape=(48, 56), n_z=10, n_target=5):
    f = synth.make_fov(5, seed, shape=shape, n_channels=1, n_z=n_z, n_target=n_target)
    return synth.ellipsoid_planes(f["nuclei"], n_z, seed=seed)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restated_following_equals_grid_sample_loop(seed):
    rng = np.random.default_rng(seed)
    gt = _volume(seed)
    dP, prob = synth.analytic_flows_3d(gt)
    dP = dP + rng.normal(0, 0.5, dP.shape).astype(np.float32)  # not only the analytic field
    fg = prob > 0
    inds = np.nonzero(fg)
    dPs = np.where(fg[None], dP, np.float32(0)).astype(np.float32) / np.float32(5.0)
    got = ref.follow_flows_3d(dPs, inds, niter=60)
    want = _steps_interp_torch(dPs, inds, niter=60)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-5


@pytest.mark.parametrize("seed", [0, 1])
def test_seed_rule_equals_max_pool3d(seed):
    import torch

    rng = np.random.default_rng(seed)
    h1 = rng.poisson(3.0, (14, 20, 22)).astype(np.int64)
    peaks = rng.random(h1.shape) < 0.02
    h1[peaks] += rng.integers(5, 40, int(peaks.sum()))
    h1[3, 4, 5] = 50
    h1[3, 5, 5] = 50  # a plateau: both are seeds
    pooled = torch.nn.functional.max_pool3d(torch.from_numpy(h1).double()[None, None], kernel_size=5, stride=1, padding=2)[0, 0]
    want = (torch.from_numpy(h1).double() == pooled).numpy() & (h1 > 10)
    got = ref.seed_mask(h1)
    assert want.any() and np.array_equal(got, want)


def test_restated_fill_equals_binary_fill_holes():
    vol = np.zeros((12, 24, 26), np.uint16)
    vol[1:8, 2:12, 2:12] = 1
    vol[3:6, 5:9, 5:9] = 0  # an enclosed cavity
    vol[2:10, 14:22, 3:13] = 2
    vol[4:7, 16:20, 6:10] = 0  # a cavity ...
    vol[5, 18, 6:13] = 0  # ... opened to the outside along X: not a hole
    vol[1:11, 2:20, 15:25] = 3
    vol[3:8, 6:14, 18:22] = 0
    vol[5, 9, 19] = 4  # a small mask inside mask 3's cavity (dropped by min_size, its voxel then filled by 3)
    out = ref.fill_holes_and_remove_small_masks_3d(vol, min_size=2)
    for lab, new in ((1, 1), (2, 2), (3, 3)):
        want = ndi.binary_fill_holes(vol == lab)
        assert np.array_equal(out == new, want), lab
    assert (out == 4).sum() == 0


@pytest.mark.parametrize("seed", [4, 5])
def test_analytic_flows_3d_recover_the_objects(seed):
    gt = _volume(seed, shape=(64, 64), n_z=12, n_target=4)
    dP, prob = synth.analytic_flows_3d(gt)
    labels, n, _ = ref.compute_masks_3d(dP, prob)
    present = np.unique(gt[gt > 0])
    big = [k for k in present if (gt == k).sum() >= 15]
    assert n == len(big) > 0
    pairs = np.unique(np.stack([gt[labels > 0], labels[labels > 0]]), axis=1)
    assert pairs.shape[1] == n and len(np.unique(pairs[0])) == n and len(np.unique(pairs[1])) == n
    for k in big:
        assert np.array_equal(np.unique(labels[gt == k]), np.unique(pairs[1][pairs[0] == k]))
