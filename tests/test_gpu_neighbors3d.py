"""
`FeatureEngine.neighbors3d` on the GPU (aliby_amd/csrc/feat_neighbors3d.hip) against tests/neighbors3d_ref.py, the NumPy restatement
that tests/test_cpu_neighbors3d_ref.py pins to hand values, scipy.ndimage and the 2-D restatement.  Parity with cp_measure /
CellProfiler is unpinned (neither can be run here).

Pass bar: NumberOfNeighbors, PercentTouching and the two object numbers (columns 0, 1, 2, 4) bit-equal to the restatement; the two
distances and the angle (columns 3, 5, 6) under the project's float rule (tests/volume_checks.py: rtol 1e-4, atol 1e-9, NaN exactly
where the restatement has NaN).  On one plane columns 0-5 are bit-equal to the 2-D family's on the same device.  Every comparison
prints its worst relative error first; on an MI355X the largest over the file was 2.45e-16 (the small batch), 1.55e-16 at the cap
and 0 elsewhere: one sqrt or atan2 apart, the bar stays the project's.
"""
from functools import partial

import numpy as np
import pytest

from tests import neighbors3d_ref as ref
from tests import neighbors_ref as ref2d
from tests.volume_checks import bits as _bits, check, quiet_numpy  # noqa: F401 (quiet_numpy: an autouse fixture)

pytestmark = pytest.mark.gpu

_check = partial(check, "neighbors3d")


def _run(engine, vols, counts, distance=None):
    """vols [F][Z,Y,X] -> the device result [sum counts, 7]"""
    import torch

    stack = np.stack([np.asarray(v, np.uint16) for v in vols])
    got = engine.neighbors3d(torch.from_numpy(stack).cuda(), counts, distance=distance)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (int(sum(counts)), 7)
    return got


def _compare(got, want, tag):
    _check(got, want, tag)
    g = got.cpu().numpy()
    for c in ref.EXACT:
        assert np.array_equal(g[:, c].copy().view(np.int64), np.ascontiguousarray(want[:, c]).view(np.int64)), (tag, ref.STEMS[c], g[:, c], want[:, c])
    return g


def _rows(scenes, name):
    lo = 0
    for k, (_, n) in scenes.items():
        if k == name:
            return slice(lo, lo + n)
        lo += n
    raise KeyError(name)


def _want(scenes, distance):
    return np.concatenate([ref.expected(k, lab, n=n, distance=distance) for k, (lab, n) in scenes.items()])


# ------------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_worked_case(engine, distance):
    got = _compare(_run(engine, [ref.worked()], [3], distance), ref.expected("worked", ref.worked(), n=3, distance=distance), f"worked d={distance}")
    if distance is None:  # the contact along an edge across planes tells S from T
        assert got[:, 0].tolist() == [1, 1, 0] and got[:, 1].tolist() == [50.0, 62.5, 25.0]
        assert got[0, 2:4].tolist() == [2, 2.0] and got[1, 6] == 90.0


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_small_batch(engine, distance):
    """One call: an empty stack, one object, two, objects on every face, edge and corner, an object filling the volume, a one-voxel
    object beside a block, coincident centres, ties at every rank, gaps in the numbering, the crowd over a dozen bitmap words and
    values above the count."""
    scenes = ref.small_scenes()
    got = _compare(_run(engine, [lab for lab, _ in scenes.values()], [n for _, n in scenes.values()], distance), _want(scenes, distance),
                   f"small batch d={distance}")
    r = lambda name: got[_rows(scenes, name)]  # noqa: E731
    assert r("empty").shape == (0, 7) and r("one").tolist() == [[0.0] * 7] and r("full").tolist() == [[0.0] * 7]
    assert (r("two")[:, 4:] == 0).all() and r("two")[:, 2].tolist() == [2, 1]
    assert r("faces_edges_corners").shape == (27, 7) and not np.isnan(r("faces_edges_corners")).any()
    assert r("sparse")[2, 0] == 0 and r("sparse")[2, 1] == 0.0 and r("sparse")[0, :2].tolist() == [1, 100.0]
    shell = r("shell")
    assert shell[1, 2] == 1 and shell[1, 3] == 0.0 and np.isnan(shell[1, 6]) and np.isnan(shell[0, 6]) and shell[2, 6] == 0.0
    cross = r("cross")
    assert cross[3, [2, 4]].tolist() == [1, 2] and cross[0, [2, 4]].tolist() == [4, 2] and cross[6, [2, 4]].tolist() == [4, 2]
    gaps = r("gaps")
    assert np.isnan(gaps[[0, 2, 3, 6, 7]]).all() and not np.isnan(gaps[[1, 4, 5, 8]]).any()
    assert r("above").shape == (2, 7) and r("above")[:, 2].tolist() == [2, 1] and (r("above")[:, 4:] == 0).all()
    if distance is None:
        assert r("above")[:, 0].tolist() == [1, 1]  # 7 and 9 touch, and are not counted
    if distance == 5:
        assert r("crowd")[0, 0] > 64


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_labels_39999_and_40000(engine, distance):
    """The bitmap near its upper size (1251 words) and the closest scan over 40 000 rows of which two are present."""
    lab = ref.high_labels()
    got = _compare(_run(engine, [lab], [40000], distance), ref.expected("high", lab, n=40000, distance=distance), f"labels 39999, 40000 d={distance}")
    assert np.isnan(got[:39998]).all()
    assert got[39998:, 0].tolist() == [1, 1] and got[39998:, 2].tolist() == [40000, 39999] and (got[39998:, 4:] == 0).all()


@pytest.mark.parametrize("distance", [None, 2])
def test_one_large_box(engine, distance):
    """A 24 x 96 x 96 object: every lane of its workgroup strides 864 times.  (The restatement of this scene at d = 16 walks 19 k
    shifted copies of 260 k voxels, some ten seconds on a CPU, too slow to run with the suite: the cap is exercised on
    `test_distance_cap`'s scene.)"""
    lab = ref.big_box()
    got = _compare(_run(engine, [lab], [2], distance), ref.expected("big", lab, n=2, distance=distance), f"large box d={distance}")
    assert got[:, 0].tolist() == [1, 1] and got[:, 2].tolist() == [2, 1]


def test_distance_cap(engine):
    """d = 16 on [12, 40, 40]: every ball leaves the volume on every side."""
    lab = ref.cap_scene()
    got = _compare(_run(engine, [lab], [4], 16), ref.expected("cap", lab, n=4, distance=16), "cap d=16")
    assert got[:, 0].tolist() == [1, 2, 1, 0]  # 2 is within 16 of 1 and of 3, the corner voxel of nothing


# ------------------------------------------------------------------------------------------------------- against the 2-D family
@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_one_plane_equals_the_2d_family(engine, distance):
    import torch

    from aliby_amd.extraction.engine import to_device_u16

    planes = np.stack(list(ref2d.small_scenes().values()))
    dl = to_device_u16(planes)
    tab = engine.object_table(dl)
    flat = engine.new_output(tab.n_obj, 7)
    engine.neighbors(dl, tab, flat, 0, distance=distance)
    torch.cuda.synchronize()
    counts = [int(p.max()) for p in planes]
    assert sum(counts) == tab.n_obj
    got = _run(engine, planes[:, None], counts, distance)
    assert torch.equal(_bits(got[:, :6]), _bits(flat[:, :6]))
    _check(got[:, 6:], flat[:, 6:].cpu().numpy(), f"one plane, angle d={distance}")


# ------------------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("distance", [None, 5])
def test_rows_carry_the_same_bits_alone_reversed_and_again(engine, distance):
    import torch

    scenes = ref.small_scenes()
    vols, counts = [lab for lab, _ in scenes.values()], [n for _, n in scenes.values()]
    batch = _run(engine, vols, counts, distance)
    assert torch.equal(_bits(_run(engine, vols, counts, distance)), _bits(batch))
    back = _run(engine, vols[::-1], counts[::-1], distance)
    hi = sum(counts)
    for name, n in zip(scenes, counts):
        rows = batch[_rows(scenes, name)]
        hi -= n
        assert torch.equal(_bits(back[hi : hi + n]), _bits(rows)), name  # (its rows in the reversed call begin where the later stacks' end)
        if n:
            assert torch.equal(_bits(_run(engine, [scenes[name][0]], [n], distance)), _bits(rows)), name
    assert hi == 0


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch(engine):
    import torch

    vol = torch.from_numpy(np.stack([ref.worked(), ref.worked()])).cuda()
    for bad in (0, 17, 2.5, True, "3"):
        with pytest.raises(ValueError):
            engine.neighbors3d(vol, [3, 3], distance=bad)
    with pytest.raises(TypeError):
        engine.neighbors3d(vol.to(torch.int32), [3, 3])
    with pytest.raises(TypeError):
        engine.neighbors3d(ref.worked()[None], [3])
    with pytest.raises(ValueError):
        engine.neighbors3d(vol[0], [3])  # [Z,Y,X]
    with pytest.raises(ValueError):
        engine.neighbors3d(vol.cpu(), [3, 3])
    for bad in ([3], [3, 3, 3], [3, 65536], [3, -1]):
        with pytest.raises(ValueError):
            engine.neighbors3d(vol, bad)
    empty = engine.neighbors3d(vol, [0, 0])
    assert tuple(empty.shape) == (0, 7) and empty.dtype == torch.float64
    # the C entry keeps the cap and refuses a NULL output
    fn, off = engine.lib.aliby_features_neighbors3d, np.asarray([0, 3, 6], np.int32)
    out, centres = engine.new_output(6, 7), torch.empty((6, 3), dtype=torch.float64, device="cuda")
    args = lambda d, o: (engine.ctx.handle, vol.data_ptr(), 2, 4, 6, 8, off.ctypes.data, d, centres.data_ptr(), o, 7, 0,  # noqa: E731
                         torch.cuda.current_stream().cuda_stream)
    assert fn(*args(17, out.data_ptr())) == 1 and fn(*args(0, out.data_ptr())) == 1 and fn(*args(1, 0)) == 1 and fn(*args(16, out.data_ptr())) == 0
    assert torch.equal(_bits(out), _bits(engine.neighbors3d(vol, [3, 3], distance=16)))
