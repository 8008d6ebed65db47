"""
`volume_secondary=True` end to end through `run_pipeline_and_post` with ONE 3-D segment step (analytic flows of six ellipsoid nuclei,
as tests/test_gpu_relate3d_pipeline.py feeds them): the `volumesecondary_cell` step's kept volume is the restatement
(tests/secondary3d_ref.py) of the kept nuclei volume, the tertiary volume and the relate3d rows are taken from it, and
profiles3d/<name>.parquet carries nuclei, cell and cytoplasm rows that join on the volume label.
"""
import numpy as np
import pytest

from aliby_amd import synth
from tests import secondary3d_ref as ref

pytestmark = pytest.mark.gpu

DISTANCE = 4
VOLUME = "None/None/sizeshape3d/Volume"


def _stack(seed=4):
    """A 6 x 48 x 64, 2-channel stack with six ellipsoid nuclei -> (pixels uint16 [1,C,Z,Y,X], nuclei uint16 [Z,Y,X])."""
    rng = np.random.default_rng(seed)
    Z, Y, X = 6, 48, 64
    zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
    nuclei = np.zeros((Z, Y, X), np.uint16)
    for label, (cy, cx) in enumerate([(12, 11), (12, 32), (12, 53), (36, 11), (36, 32), (36, 53)], 1):
        c = (rng.uniform(2.0, 3.0), cy + rng.uniform(-1, 1), cx + rng.uniform(-1, 1))
        r = (rng.uniform(1.3, 1.8), rng.uniform(3, 5), rng.uniform(3, 5))
        nuclei[sum(((g - ci) / ri) ** 2 for g, ci, ri in zip((zz, yy, xx), c, r)) <= 1.0] = label
    assert len(np.unique(nuclei)) == 7
    base = rng.integers(200, 1200, size=(Z, Y, X))
    pixels = np.stack([base + np.where(nuclei > 0, 9000, 0) + rng.integers(0, 3000, size=(Z, Y, X)),
                       base // 2 + rng.integers(0, 6000, size=(Z, Y, X))]).astype(np.uint16)
    return pixels[None], nuclei


def test_three_volume_compartments_from_one_segmentation(tmp_path, engine):
    import pyarrow.parquet as pq
    import torch

    from aliby_amd import pipe_core
    from aliby_amd.pipe import init_step
    from aliby_amd.pipe_builder import build_pipeline_steps

    pixels, nuclei = _stack()
    dP, prob = synth.analytic_flows_3d(nuclei)

    def flows_override(x):
        assert tuple(x.shape) == (1, 6, 48, 64)
        return torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()

    def configure(p):
        p["steps"]["tile"]["image_kwargs"] = {"source": pixels}  # T = 1: [T,C,Z,Y,X] = 1 x 2 x 6 x 48 x 64
        p["steps"]["segment_nuclei"]["segmenter_kwargs"].update(volume_mode="flows3d", setup_params=dict(flows_override=flows_override))
        return p

    common = dict(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("intensity",),
                  volume_features=("intensity3d",), secondary={"cell": ("nuclei", DISTANCE)})
    linked = dict(relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")}, volume_relate=True)
    pipeline = configure(build_pipeline_steps(**common, **linked, volume_secondary=True))
    pipeline["save"] = [*pipeline["save"], "volumesecondary_cell"]
    made = {}

    def init(step_name, parameters, other_steps=None):
        made[step_name] = init_step(step_name, parameters, other_steps)
        return made[step_name]

    _, post = pipe_core._run_pipeline_and_post_impl(pipeline, "grown", tmp_path, init_step_fn=init)
    table = post["profiles3d"]
    assert pq.read_table(tmp_path / "profiles3d" / "grown.parquet").num_rows == table.num_rows > 0

    # the kept volume is the restatement of the kept nuclei volume, with the nuclei's counts
    vn, cn = made["segment_nuclei"].last_volume
    vc, cc = made["volumesecondary_cell"].last_volume
    vt, ct = made["volumetertiary_cytoplasm"].last_volume
    n = int(cn[0])
    assert n == 6 and int(cc[0]) == n and int(ct[0]) == n
    host_n, host_c = vn[0].cpu().numpy(), vc[0].cpu().numpy()
    assert vc.dtype == torch.uint16 and tuple(vc.shape) == tuple(vn.shape) == (1, 6, 48, 64)
    assert np.array_equal(host_c, ref.secondary_stack(host_n, DISTANCE)[0])
    assert (host_c != 0).sum() > (host_n != 0).sum() and (host_c == 0).any() and np.array_equal(host_c[host_n != 0], host_n[host_n != 0])
    assert torch.equal(vt.view(torch.int16), engine.tertiary_volume(vc, vn, shrink_inner=True).view(torch.int16))

    # nuclei, cell and cytoplasm rows, in the order of the volume steps, joined on the label
    objects = table.column("metadata_object").to_pylist()
    assert objects == ["nuclei"] * n + ["cell"] * n + ["cytoplasm"] * n
    assert table.column("metadata_label").to_pylist() == [*range(1, n + 1)] * 3
    volume = table.column(VOLUME).to_pylist()
    for k, label in enumerate(range(1, n + 1)):
        assert volume[k] == float((host_n == label).sum()) < volume[n + k] == float((host_c == label).sum())
        assert volume[2 * n + k] == float((vt[0].cpu().numpy() == label).sum()) < volume[n + k]
    # Parent_cell of a nuclei row is its own label, and every cell has its one nucleus
    parents = table.column("None/None/relate3d/Parent_cell").to_pylist()
    assert parents[:n] == [float(label) for label in range(1, n + 1)] and all(p is None for p in parents[n:])
    children = table.column("None/None/relate3d/Children_nuclei_Count").to_pylist()
    assert children[n:2 * n] == [1.0] * n
    assert table.column("None/None/relate3d/Parent_nuclei").to_pylist()[n:2 * n] == [float(label) for label in range(1, n + 1)]

    # the listed step was saved like a segment step's masks
    with np.load(tmp_path / "steps" / "grown" / "volumesecondary_cell" / "0000.npz") as z:
        assert list(z.keys()) == ["arr_0"] and np.array_equal(z["arr_0"], host_c)

    # with volume_secondary=False the steps are absent (and the linked keywords are refused, as before)
    plain = build_pipeline_steps(**common, volume_secondary=False)
    assert not any(s.startswith("volumesecondary_") for s in plain["steps"]) and "volume_cell" not in plain["steps"]
    with pytest.raises(ValueError, match="no volume form"):
        build_pipeline_steps(**common, **linked, volume_secondary=False)
