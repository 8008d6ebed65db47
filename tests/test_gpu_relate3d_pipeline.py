"""
`volume_relate=True` end to end through `run_pipeline_and_post`: two 3-D segment steps (analytic flows of nuclei and of the same
ellipsoids dilated: every nucleus has a cell), the `volumetertiary_cytoplasm`, `volume_*` and `volumerelate_*` steps, and the table
profiles3d/<name>.parquet with nuclei, cell and cytoplasm rows and the relate3d columns joined on.  Every comparison is with the direct
engine call on the volumes the steps kept (the same kernels and launches): bit for bit.
"""
import numpy as np
import pytest

from aliby_amd import synth
from tests import relate3d_ref as ref

pytestmark = pytest.mark.gpu


def _stacks(seed=4):
    """A 6 x 48 x 64, 2-channel stack: six ellipsoid nuclei (channel 0), and the same ellipsoids dilated as cells (channel 1)
    -> (pixels uint16 [1,C,Z,Y,X], nuclei uint16 [Z,Y,X], cells uint16 [Z,Y,X])."""
    rng = np.random.default_rng(seed)
    Z, Y, X = 6, 48, 64
    zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
    nuclei, cells = np.zeros((Z, Y, X), np.uint16), np.zeros((Z, Y, X), np.uint16)
    for label, (cy, cx) in enumerate([(12, 11), (12, 32), (12, 53), (36, 11), (36, 32), (36, 53)], 1):
        c = (rng.uniform(2.0, 3.0), cy + rng.uniform(-1, 1), cx + rng.uniform(-1, 1))
        r = (rng.uniform(1.3, 1.8), rng.uniform(3, 5), rng.uniform(3, 5))
        for vol, grow in ((cells, (1.2, 3.5, 3.5)), (nuclei, (0, 0, 0))):
            vol[sum(((g - ci) / (ri + gi)) ** 2 for g, ci, ri, gi in zip((zz, yy, xx), c, r, grow)) <= 1.0] = label
    assert len(np.unique(nuclei)) == 7 and len(np.unique(cells)) == 7 and (cells[nuclei > 0] == nuclei[nuclei > 0]).all()
    base = rng.integers(200, 1200, size=(Z, Y, X))
    pixels = np.stack([base + np.where(nuclei > 0, 9000, 0) + rng.integers(0, 3000, size=(Z, Y, X)),
                       base // 2 + np.where(cells > 0, 5000, 0) + rng.integers(0, 6000, size=(Z, Y, X))]).astype(np.uint16)
    return pixels[None], nuclei, cells


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b):
    return _bits(a).shape == _bits(b).shape and np.array_equal(_bits(a), _bits(b))


def _same_table(a, b):
    if a.column_names != b.column_names or a.num_rows != b.num_rows:
        return False
    for name in a.column_names:
        x, y = a.column(name).to_pylist(), b.column(name).to_pylist()
        if x != y and not _same([np.nan if v is None else v for v in x], [np.nan if v is None else v for v in y]):
            return False
        if [v is None for v in x] != [v is None for v in y]:
            return False
    return True


def test_volume_relate_end_to_end(tmp_path, engine):
    import pyarrow.parquet as pq
    import torch

    from aliby_amd import pipe_core
    from aliby_amd.extraction.extract import format_extraction, process_tree_volumes
    from aliby_amd.pipe import init_step, run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    pixels, nuclei, cells = _stacks()
    flows = {"nuclei": synth.analytic_flows_3d(nuclei), "cell": synth.analytic_flows_3d(cells)}

    def override(obj):
        def flows_override(x):
            assert tuple(x.shape) == (1, 6, 48, 64)
            return torch.from_numpy(flows[obj][0][None]).cuda(), torch.from_numpy(flows[obj][1][None]).cuda()
        return flows_override

    def configure(p):
        p["steps"]["tile"]["image_kwargs"] = {"source": pixels}  # T = 1: [T,C,Z,Y,X] = 1 x 2 x 6 x 48 x 64
        for obj in ("nuclei", "cell"):
            p["steps"][f"segment_{obj}"]["segmenter_kwargs"].update(volume_mode="flows3d", setup_params=dict(flows_override=override(obj)))
        return p

    common = dict(channels_to_segment={"nuclei": 0, "cell": 1}, channels_to_extract=[0, 1], features_to_extract=("intensity",),
                  volume_features=("intensity3d",), relate=[("nuclei", "cell")], tertiary={"cytoplasm": ("cell", "nuclei")})
    pipeline = configure(build_pipeline_steps(**common, volume_relate=True))
    pipeline["save"] = [*pipeline["save"], "volumetertiary_cytoplasm"]
    made = {}

    def init(step_name, parameters, other_steps=None):
        made[step_name] = init_step(step_name, parameters, other_steps)
        return made[step_name]

    profiles, post = pipe_core._run_pipeline_and_post_impl(pipeline, "rel", tmp_path, init_step_fn=init)
    table = post["profiles3d"]
    # the file is the returned table
    on_disk = pq.read_table(tmp_path / "profiles3d" / "rel.parquet")
    assert on_disk.num_rows == table.num_rows > 0 and _same_table(on_disk, table)

    # nuclei, cell and cytoplasm rows, in the order of the volume steps
    (vn, cn), (vc, cc) = made["segment_nuclei"].last_volume, made["segment_cell"].last_volume
    vt, ct = made["volumetertiary_cytoplasm"].last_volume
    n_n, n_c = int(cn[0]), int(cc[0])
    assert n_n == 6 and n_c == 6 and int(ct[0]) == n_c
    objects = table.column("metadata_object").to_pylist()
    assert objects == ["nuclei"] * n_n + ["cell"] * n_c + ["cytoplasm"] * n_c
    labels = table.column("metadata_label").to_pylist()
    assert labels == [*range(1, n_n + 1), *range(1, n_c + 1), *range(1, n_c + 1)]
    rows = {obj: [i for i, o in enumerate(objects) if o == obj] for obj in ("nuclei", "cell", "cytoplasm")}

    # the relate3d columns are FeatureEngine.relate3d on the kept volumes
    want_n, want_c = engine.relate3d(vn, cn, vc, cc)
    want_n, want_c = want_n.cpu().numpy(), want_c.cpu().numpy()
    for other, mine, want in (("cell", "nuclei", want_n), ("nuclei", "cell", want_c)):
        for k, name in enumerate(ref.names(other)):
            col = table.column(f"None/None/relate3d/{name}").to_pylist()
            assert _same([col[i] for i in rows[mine]], want[:, k]), (mine, name)
            assert all(col[i] is None for i in range(table.num_rows) if i not in rows[mine]), (mine, name)
    # every nucleus has a parent, and it is a cell row's label; the segmentation gave the nucleus the label of its own cell or not,
    # the overlap decides: compare with the restatement on the kept volumes
    parents = [int(table.column("None/None/relate3d/Parent_cell")[i].as_py()) for i in rows["nuclei"]]
    assert all(p in [labels[i] for i in rows["cell"]] for p in parents) and len(set(parents)) == n_n
    ra, rb = ref.relate3d(vn[0].cpu().numpy(), vc[0].cpu().numpy(), n_n, n_c)
    assert np.array_equal(want_n[:, :3], ra[:, :3]) and np.array_equal(want_c[:, :3], rb[:, :3])
    assert np.allclose(want_n[:, 3:], ra[:, 3:], rtol=ref.RTOL, atol=ref.ATOL) and np.allclose(want_c[:, 3:], rb[:, 3:], rtol=ref.RTOL, atol=ref.ATOL)
    assert (want_c[:, 2] == 1).all()  # every cell has its one child

    # the cytoplasm rows are process_tree_volumes on tertiary_volume(cells, nuclei)
    want_t = engine.tertiary_volume(vc, vn, shrink_inner=True)
    assert torch.equal(vt.view(torch.int16), want_t.view(torch.int16))
    assert np.array_equal(vt[0].cpu().numpy(), ref.tertiary(vc[0].cpu().numpy(), vn[0].cpu().numpy(), True))
    tree = pipeline["steps"]["volume_cytoplasm"]["tree"]
    for obj, vol, counts in (("cytoplasm", want_t, cc), ("nuclei", vn, cn), ("cell", vc, cc)):
        want = format_extraction(process_tree_volumes(tree, vol, pixels, counts=counts))
        features = [c for c in want.column_names if c not in ("tile", "label")]
        assert "0/None/intensity3d/Intensity_MeanIntensity" in features and "None/None/sizeshape3d/Volume" in features
        for c in features:
            assert _same([table.column(c)[i].as_py() for i in rows[obj]], want.column(c).to_numpy()), (obj, c)
    cyto_volume = [table.column("None/None/sizeshape3d/Volume")[i].as_py() for i in rows["cytoplasm"]]
    cell_volume = [table.column("None/None/sizeshape3d/Volume")[i].as_py() for i in rows["cell"]]
    assert all(0 < t < c for t, c in zip(cyto_volume, cell_volume))

    # the tertiary volume was saved like a segment step's masks
    saved = np.load(tmp_path / "steps" / "rel" / "volumetertiary_cytoplasm" / "0000.npz")
    assert np.array_equal(saved["arr_0"], vt[0].cpu().numpy())

    # the 2-D table is the same pipeline's without volume_relate
    plain = configure(build_pipeline_steps(**common))
    assert not any(n.startswith(("volumetertiary_", "volumerelate_")) for n in plain["steps"])
    want2d, post2d = run_pipeline_and_post(pipeline=plain, pipeline_name="plain", output_path=tmp_path)
    assert profiles.num_rows > 0 and _same_table(profiles, want2d)
    assert _same_table(pq.read_table(tmp_path / "profiles" / "rel.parquet"), pq.read_table(tmp_path / "profiles" / "plain.parquet"))
    # and its volume table is this one's nuclei and cell rows without the relate3d columns
    plain3d = post2d["profiles3d"]
    assert plain3d.num_rows == n_n + n_c and not [c for c in plain3d.column_names if "relate3d" in c]
    assert _same_table(table.slice(0, n_n + n_c).select(plain3d.column_names), plain3d)
