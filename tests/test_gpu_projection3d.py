"""
`FeatureEngine.projection3d` (csrc/feat_projection3d.hip) on the device against the NumPy restatement tests/projection3d_ref.py, bit
for bit: the counts and the label are integers, the fraction is one float64 division, so every comparison is `==`.
"""
import numpy as np
import pytest

from tests import projection3d_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.hand_cases()


def _run(engine, volume, counts, **kw):
    import torch

    return engine.projection3d(torch.from_numpy(np.ascontiguousarray(volume)).cuda(), counts, **kw).cpu().numpy()


def _ellipsoids(seed, shape=(6, 37, 70), n=12):
    """About n ellipsoids painted in label order (a later one overwrites an earlier one where they meet), flat in z so that they
    overlap in projection; label 1 lies wholly under label n; two columns hold more than two labels with re-entries."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
    vol = np.zeros(shape, np.uint16)

    def paint(label, centre, radii):
        inside = sum(((g - c) / r) ** 2 for g, c, r in zip((zz, yy, xx), centre, radii)) <= 1.0
        vol[inside] = label

    paint(1, (0.5, 18, 30), (1.0, 3.5, 4.5))
    for label in range(2, n):
        paint(label, (rng.uniform(0, Z - 1), rng.uniform(3, Y - 3), rng.uniform(3, X - 3)),
              (rng.uniform(0.8, 2.0), rng.uniform(3, 8), rng.uniform(3, 11)))
    paint(n, (4.0, 18, 30), (1.5, 7.0, 9.0))
    vol[:2][((yy[:2] - 18) / 3.0) ** 2 + ((xx[:2] - 30) / 3.9) ** 2 <= 1.0] = 1  # (label 1 back where others took it)
    vol[:, 0, 0] = (1, 2, 3, 0, 3, 4)[:Z]
    vol[:, Y - 1, X - 1] = (5, 6, 7, 8, 7, 5)[:Z]
    return vol


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(engine, name):
    volume, counts, want = CASES[name]
    got = _run(engine, volume, counts)
    assert got.dtype == np.float64 and ref.same_rows(got, want), (got, want)
    assert ref.same_rows(got, ref.projection3d(volume, counts))


def test_random_stack(engine):
    vol = _ellipsoids(3)
    assert vol.shape[2] % 16 and vol.shape[2] % 64 and vol.shape[1] * vol.shape[2] > 2 * 256  # odd X, more than one workgroup
    counts = [12]
    vol[5, 30:33, 60:64] = 14  # above the count: no row, but it hides what lies under it
    want = ref.projection3d(vol[None], counts)
    assert want[0, 0] > 0 and want[0, 1] == 0 and want[0, 3] == 0  # label 1 is fully hidden
    assert ((want[:, 1] > 0) & (want[:, 1] < want[:, 0])).sum() >= 3  # objects overlap in projection
    got = _run(engine, vol[None], counts)
    assert ref.same_rows(got, want), np.argwhere(got != want)
    assert ref.same_rows(_run(engine, vol[None], counts), got)  # run to run


def test_batch_rows_equal_each_stack_alone(engine):
    vols = np.stack([_ellipsoids(s, n=n) for s, n in ((3, 12), (4, 9), (5, 12))])
    counts = [12, 7, 0]  # the second stack holds values above its count, the third gets no row
    got = _run(engine, vols, counts)
    assert got.shape == (19, 4) and ref.same_rows(got, ref.projection3d(vols, counts))
    alone = [_run(engine, vols[f:f + 1], counts[f:f + 1]) for f in range(3)]
    assert alone[2].shape == (0, 4)
    assert ref.same_rows(got, np.concatenate(alone, 0))


def test_label_is_the_collapsed_image(engine):
    """Projection_Label against the collapse a 3-D segment step returns: for every object, the pixels of the collapse that carry
    its label are exactly the columns whose top it is."""
    import torch

    from aliby_amd.segment.cellpose_hip import CellposeModel

    model = CellposeModel(flows_override=lambda x: None)
    vols = np.stack([_ellipsoids(6), _ellipsoids(7)])
    counts = [int(v.max()) for v in vols]
    rows = _run(engine, vols, counts)
    dev = torch.from_numpy(vols).cuda()
    row = 0
    for f in range(2):
        flat = model.max_project_and_relabel(dev[f]).cpu().numpy()
        assert np.array_equal(flat, ref.collapse(vols[f]))
        top = vols[f].max(axis=0)
        seen = set()
        for L in range(1, counts[f] + 1):
            label = int(rows[row, 3])
            if label:
                assert np.array_equal(flat == label, top == L) and label not in seen
                seen.add(label)
            else:
                assert not (top == L).any()
            row += 1
        assert seen == set(np.unique(flat)) - {0}  # every label of the collapse is some object's


def test_grid_stride_rounds(engine):
    """More columns than the launch's grid holds lanes (4096 workgroups x 256): the columns of the second round are compared too.
    Z = 1, 2.5 MB of labels."""
    Y, X = 1024, 1229
    assert Y * X > 4096 * 256 + 64 * X
    rng = np.random.default_rng(11)
    vol = np.zeros((1, 1, Y, X), np.uint16)
    blocks = rng.integers(0, 40, size=(Y // 32, (X + 31) // 32)).astype(np.uint16)
    vol[0, 0] = np.kron(blocks, np.ones((32, 32), np.uint16))[:, :X]
    vol[0, 0, Y - 3:, :] = 41  # the last rows: lanes of the second round only
    counts = [41]
    want = np.zeros((41, 4))
    area = np.bincount(vol.ravel(), minlength=42)[1:]
    want[:, 0] = want[:, 1] = area
    want[:, 2] = np.where(area > 0, 1.0, np.nan)
    present = np.flatnonzero(area > 0)
    want[present, 3] = np.arange(1, len(present) + 1)
    assert want[40, 0] == 3 * X
    got = _run(engine, vol, counts)
    assert ref.same_rows(got, want)


def test_out_and_col0_write_in_place(engine):
    import torch

    volume, counts, want = CASES["two_stacks"]
    dev = torch.from_numpy(volume).cuda()
    out = torch.full((3, 9), -1.0, dtype=torch.float64, device="cuda")
    view = engine.projection3d(dev, counts, out=out, col0=3)
    assert view.data_ptr() == out[:, 3:7].data_ptr() and tuple(view.shape) == (3, 4)
    host = out.cpu().numpy()
    assert ref.same_rows(host[:, 3:7], want) and (host[:, :3] == -1).all() and (host[:, 7:] == -1).all()
    with pytest.raises(ValueError):
        engine.projection3d(dev, counts, out=out, col0=6)
    with pytest.raises(ValueError):
        engine.projection3d(dev, counts, out=out[:2], col0=0)
    with pytest.raises(TypeError):
        engine.projection3d(dev, counts, out=out.float(), col0=0)


def test_refusals(engine):
    import torch

    dev = torch.zeros((1, 2, 3, 4), dtype=torch.uint16, device="cuda")
    with pytest.raises(TypeError):
        engine.projection3d(dev.to(torch.int32), [1])
    with pytest.raises(ValueError):
        engine.projection3d(dev[0], [1])
    with pytest.raises(ValueError):
        engine.projection3d(dev, [1, 1])
    with pytest.raises(ValueError):
        engine.projection3d(dev.cpu(), [1])
