"""
The volume instruction tree on the device: `process_tree_volumes` against the direct engine calls of the same families with the same
keywords (the same kernels and the same launches, so every comparison is bit for bit), its input forms, and the `volume_<obj>`
step end to end through `run_pipeline_and_post` (profiles3d/<name>.parquet beside profiles/<name>.parquet).
"""
import numpy as np
import pytest

from aliby_amd import synth
from aliby_amd.extraction import features as feat

pytestmark = pytest.mark.gpu

EXAMPLE = {"None": {"None": ["sizeshape3d", "neighbors3d", "projection3d"]},
           0: {"None": ["intensity3d", "intensity3d_detail", "texture3d"]},
           1: {"None": ["intensity3d", "granularity3d"]},
           (0, 1): {"None": ["pearson", "manders_fold", "rwc", "costes"]}}
COLOC = ("pearson", "manders_fold", "rwc", "costes")


def _stack(seed=3):
    """A 6 x 48 x 64, 2-channel stack with 6 ellipsoids -> (pixels uint16 [1,C,Z,Y,X], volume uint16 [1,Z,Y,X], counts).  (The
    objects of synth.make_fov do not fit a frame this small.)"""
    rng = np.random.default_rng(seed)
    Z, Y, X = 6, 48, 64
    zz, yy, xx = np.mgrid[0:Z, 0:Y, 0:X]
    volume = np.zeros((Z, Y, X), np.uint16)
    centres = [(12, 11), (12, 32), (12, 53), (36, 11), (36, 32), (36, 53)]
    for label, (cy, cx) in enumerate(centres, 1):
        c = (rng.uniform(1.5, 3.5), cy + rng.uniform(-2, 2), cx + rng.uniform(-2, 2))
        r = (rng.uniform(1.6, 2.6), rng.uniform(5, 9), rng.uniform(5, 9))
        volume[sum(((g - ci) / ri) ** 2 for g, ci, ri in zip((zz, yy, xx), c, r)) <= 1.0] = label
    assert len(np.unique(volume)) == 7
    base = rng.integers(200, 1200, size=(Z, Y, X))
    glow = np.where(volume > 0, 4000 + 900 * volume.astype(np.int64), 0)
    pixels = np.stack([base + glow + rng.integers(0, 3000, size=(Z, Y, X)),
                       base // 2 + glow // 3 + rng.integers(0, 6000, size=(Z, Y, X))]).astype(np.uint16)
    return pixels[None], volume[None], [6]


@pytest.fixture(scope="module")
def stack():
    import torch

    pixels, volume, counts = _stack()
    return dict(pixels=pixels, volume=volume, counts=counts, px=torch.from_numpy(pixels).cuda(), vol=torch.from_numpy(volume).cuda())


def _bits(a):
    import torch

    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return _bits(a).shape == _bits(b).shape and np.array_equal(_bits(a), _bits(b))


def _direct(engine, vol, px, counts, kw=None):
    """The blocks of EXAMPLE from the engine's own methods, one call per family, in the tree's order."""
    kw = kw or {}
    blocks = [engine.sizeshape3d(vol, counts, **kw.get("sizeshape3d", {})), engine.neighbors3d(vol, counts, **kw.get("neighbors3d", {})),
              engine.projection3d(vol, counts), engine.intensity3d(vol, px, 0, counts),
              engine.intensity3d_detail(vol, px, 0, counts, **kw.get("intensity3d_detail", {})),
              engine.texture3d(vol, px, 0, counts, **kw.get("texture3d", {})), engine.intensity3d(vol, px, 1, counts),
              engine.granularity3d(vol, px, 1, counts, **kw.get("granularity3d", {}))]
    thr = kw.get("manders_fold", {}).get("thr")
    if thr is None or thr == kw.get("rwc", {}).get("thr", 15.0):
        blocks.append(engine.coloc3d(vol, px, [(0, 1)], counts, metrics=COLOC, thr=15.0 if thr is None else float(thr)))
    else:  # manders_fold's threshold is its own: two calls
        blocks.append(engine.coloc3d(vol, px, [(0, 1)], counts, metrics=COLOC[:2], thr=float(thr)))
        blocks.append(engine.coloc3d(vol, px, [(0, 1)], counts, metrics=COLOC[2:], thr=float(kw.get("rwc", {}).get("thr", 15.0))))
    return blocks


def _expected_names(kw=None):
    kw = kw or {}
    names = [f"None/None/sizeshape3d/{n}" for n in feat.sizeshape3d_names(kw.get("sizeshape3d", {}).get("surface_area", False))]
    names += [f"None/None/neighbors3d/{n}" for n in feat.neighbors3d_names(kw.get("neighbors3d", {}).get("distance"))]
    names += [f"None/None/projection3d/{n}" for n in feat.projection3d_names()]
    names += [f"0/None/intensity3d/{n}" for n in feat.intensity3d_names()]
    names += [f"0/None/intensity3d_detail/{n}" for n in feat.intensity3d_detail_names(kw.get("intensity3d_detail", {}).get("edge_measurements", True))]
    names += [f"0/None/texture3d/{n}" for n in feat.texture3d_names()]
    names += [f"1/None/intensity3d/{n}" for n in feat.intensity3d_names()]
    names += [f"1/None/granularity3d/{n}" for n in feat.granularity3d_names(kw.get("granularity3d", {}).get("granular_spectrum_length", 16))]
    names += [f"(0, 1)/None/{m}/{n}" for m in COLOC for n in feat.COLOC[m]]
    return names


def _check_against_direct(engine, stack, kw):
    import torch

    from aliby_amd.extraction.extract import format_extraction, process_tree_volumes

    inst, res = process_tree_volumes(EXAMPLE, stack["vol"], stack["px"], counts=stack["counts"], cp_measure_kwargs=kw)
    want = torch.cat(_direct(engine, stack["vol"], stack["px"], stack["counts"], kw), 1)
    n = stack["counts"][0]
    assert res.matrix.shape == tuple(want.shape) == (n, len(_expected_names(kw)))
    assert res.column_names() == _expected_names(kw)
    for (c0, names), inst_k in zip(res.blocks, res.instructions):
        assert _same(res.matrix[:, c0:c0 + len(names)], want[:, c0:c0 + len(names)]), inst_k
    assert res.objects == [(0, lab) for lab in range(1, n + 1)]
    assert len(inst) == len(res) == n * len(res.instructions) and inst[0] == ((0, 1), ("None", "None", "sizeshape3d"))
    table = format_extraction((inst, res))
    assert table.num_rows == n and table.column("label").to_pylist() == list(range(1, n + 1))
    assert set(table.column_names) == {"tile", "label", *_expected_names(kw)}
    col = "None/None/projection3d/Projection_Label"
    assert _same(table.column(col).to_numpy(), want[:, res.column_names().index(col)])
    return res


def test_example_tree_equals_the_direct_calls(engine, stack):
    res = _check_against_direct(engine, stack, None)
    assert res.matrix.shape[1] == 260
    assert res[0]["Volume"].shape == (1,) and res[0]["Volume"][0] > 0  # the reference's dict per (object, instruction)


def test_keywords_reach_the_families(engine, stack):
    kw = {"sizeshape3d": {"spacing": (2.0, 0.5, 0.5), "surface_area": True}, "intensity3d_detail": {"edge_measurements": False},
          "neighbors3d": {"distance": 3}, "granularity3d": {"granular_spectrum_length": 3, "element_size": 2},
          "manders_fold": {"thr": 30}}
    res = _check_against_direct(engine, stack, kw)
    names = res.column_names()
    assert "None/None/sizeshape3d/SurfaceArea" in names and "None/None/neighbors3d/Neighbors_PercentTouching_3" in names
    assert "1/None/granularity3d/Granularity_3" in names and "1/None/granularity3d/Granularity_4" not in names
    assert "0/None/intensity3d_detail/Intensity_MeanIntensityEdge" not in names
    # the keywords changed the numbers too: the default tree's blocks differ
    from aliby_amd.extraction.extract import process_tree_volumes

    _, plain = process_tree_volumes(EXAMPLE, stack["vol"], stack["px"], counts=stack["counts"])
    assert not _same(res.matrix[:, 0:1], plain.matrix[:, 0:1])  # Volume scaled by the spacing
    k, j = names.index("(0, 1)/None/manders_fold/Correlation_Manders_1"), plain.column_names().index("(0, 1)/None/manders_fold/Correlation_Manders_1")
    r, q = names.index("(0, 1)/None/rwc/Correlation_RWC_1"), plain.column_names().index("(0, 1)/None/rwc/Correlation_RWC_1")
    assert _same(res.matrix[:, r], plain.matrix[:, q])  # rwc keeps its own threshold
    assert not _same(res.matrix[:, k], plain.matrix[:, j])


def test_stack_without_objects(engine, stack):
    import torch

    from aliby_amd.extraction.extract import format_extraction, process_tree_volumes

    empty = torch.zeros_like(stack["vol"])
    for counts in (None, [0]):
        inst, res = process_tree_volumes(EXAMPLE, empty, stack["px"], counts=counts)
        assert res.matrix.shape == (0, 260) and len(inst) == len(res) == 0 and res.objects == []
        assert format_extraction((inst, res)).num_rows == 0


def test_host_and_list_inputs_equal_the_device_tensor(engine, stack):
    from aliby_amd.extraction.extract import process_tree_volumes

    tree = {"None": {"None": ["sizeshape3d", "projection3d"]}, 0: {"None": ["intensity3d"]}, (0, 1): {"None": ["pearson"]}}
    _, want = process_tree_volumes(tree, stack["vol"], stack["px"], counts=stack["counts"])
    forms = {"host [F,Z,Y,X]": (stack["volume"], stack["pixels"]), "host [Z,Y,X]": (stack["volume"][0], stack["pixels"]),
             "list of [Z,Y,X]": ([stack["volume"][0]], stack["pixels"]), "int32 labels": (stack["volume"].astype(np.int32), stack["px"])}
    for name, (vol, px) in forms.items():
        for counts in (None, stack["counts"]):
            inst, got = process_tree_volumes(tree, vol, px, counts=counts)
            assert _same(got.matrix, want.matrix) and got.objects == want.objects, name
    # two stacks as a list: rows of each stack alone, tile by tile
    other = np.ascontiguousarray(stack["volume"][0, ::-1])
    both_px = np.concatenate([stack["pixels"], stack["pixels"][:, :, ::-1]], 0)
    _, two = process_tree_volumes(tree, [stack["volume"][0], other], both_px)
    n = stack["counts"][0]
    assert two.objects == [(f, lab) for f in (0, 1) for lab in range(1, n + 1)]
    assert _same(two.matrix[:n], want.matrix)
    _, second = process_tree_volumes(tree, other, both_px[1:])
    assert _same(two.matrix[n:], second.matrix)


def test_float32_pixels(engine, stack):
    import torch

    from aliby_amd.extraction.extract import process_tree_volumes

    pxf = stack["pixels"].astype(np.float32) / 65535.0
    with pytest.raises(TypeError, match="intensity3d"):
        process_tree_volumes({0: {"None": ["intensity3d"]}}, stack["vol"], pxf, counts=stack["counts"])
    tree = {0: {"None": ["intensity3d_detail", "texture3d"]}, 1: {"None": ["granularity3d"]}, (0, 1): {"None": list(COLOC)}}
    kw = {"granularity3d": {"granular_spectrum_length": 2}}
    _, res = process_tree_volumes(tree, stack["vol"], pxf, counts=stack["counts"], cp_measure_kwargs=kw)
    dev = torch.from_numpy(pxf).cuda()
    vol, counts = stack["vol"], stack["counts"]
    want = torch.cat([engine.intensity3d_detail(vol, dev, 0, counts), engine.texture3d(vol, dev, 0, counts),
                      engine.granularity3d(vol, dev, 1, counts, granular_spectrum_length=2),
                      engine.coloc3d(vol, dev, [(0, 1)], counts, metrics=COLOC)], 1)
    assert _same(res.matrix, want)


# ------------------------------------------------------------------------------------------------ the pipeline step
def _same_table(a, b):
    if a.column_names != b.column_names or a.num_rows != b.num_rows:
        return False
    for name in a.column_names:
        x, y = a.column(name).to_pylist(), b.column(name).to_pylist()
        if x != y and not (all(isinstance(v, float) for v in x + y) and _same(np.asarray(x), np.asarray(y))):
            return False
    return True


def test_volume_step_end_to_end(tmp_path, engine):
    import pyarrow.parquet as pq
    import torch

    from aliby_amd import pipe_core
    from aliby_amd.extraction.extract import format_extraction, process_tree_volumes
    from aliby_amd.pipe import init_step, run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    pixels, volume, _ = _stack(4)
    dP, prob = synth.analytic_flows_3d(volume[0])

    def override(x):
        assert tuple(x.shape) == (1, 6, 48, 64)
        return torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()

    def configure(p, **segmenter_kwargs):
        p["steps"]["tile"]["image_kwargs"] = {"source": pixels}  # T = 1: [T,C,Z,Y,X] = 1 x 2 x 6 x 48 x 64
        p["steps"]["segment_nuclei"]["segmenter_kwargs"].update(volume_mode="flows3d", setup_params=dict(flows_override=override),
                                                                **segmenter_kwargs)
        return p

    common = dict(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("intensity",))
    pipeline = configure(build_pipeline_steps(**common, volume_features=("intensity3d", "intensity3d_detail"), volume_coloc=True))
    assert pipeline["steps"]["segment_nuclei"]["segmenter_kwargs"]["do_3D"] is True
    made = {}

    def init(step_name, parameters, other_steps=None):
        made[step_name] = init_step(step_name, parameters, other_steps)
        return made[step_name]

    profiles, post = pipe_core._run_pipeline_and_post_impl(pipeline, "vol", tmp_path, init_step_fn=init)
    table3d = post["profiles3d"]
    # the file is the returned table
    assert (tmp_path / "profiles3d" / "vol.parquet").exists() and (tmp_path / "profiles" / "vol.parquet").exists()
    on_disk = pq.read_table(tmp_path / "profiles3d" / "vol.parquet")
    assert on_disk.num_rows == table3d.num_rows > 0 and _same_table(on_disk, table3d)
    # its rows are process_tree_volumes on the volume the segment step kept
    vol_dev, counts = made["segment_nuclei"].last_volume
    assert tuple(vol_dev.shape) == (1, 6, 48, 64) and int(counts[0]) == table3d.num_rows
    tree = pipeline["steps"]["volume_nuclei"]["tree"]
    want = format_extraction(process_tree_volumes(tree, vol_dev, pixels, counts=counts))
    assert table3d.column("metadata_label").to_pylist() == want.column("label").to_pylist() == list(range(1, int(counts[0]) + 1))
    assert table3d.column("metadata_object").to_pylist() == ["nuclei"] * table3d.num_rows
    assert set(table3d.column("metadata_tp").to_pylist()) == {0} and set(table3d.column("metadata_tile").to_pylist()) == {0}
    features = [c for c in want.column_names if c not in ("tile", "label")]
    assert sorted(features) == sorted(c for c in table3d.column_names if not c.startswith("metadata_"))
    for c in features:
        assert _same(table3d.column(c).to_numpy(), want.column(c).to_numpy()), c
    assert "0/None/intensity3d/Intensity_MeanIntensity" in features and "(0, 1)/None/pearson/Correlation_Pearson" in features
    assert "None/None/sizeshape3d/Volume" in features and "1/None/intensity3d_detail/Intensity_MedianIntensity" in features
    # the 2-D table is what the same pipeline without the volume step measures on the collapse
    plain = configure(build_pipeline_steps(**common), do_3D=True)
    assert "volume_nuclei" not in plain["steps"]
    want2d, post2d = run_pipeline_and_post(pipeline=plain, pipeline_name="flat", output_path=tmp_path)
    assert post2d == {} and not (tmp_path / "profiles3d" / "flat.parquet").exists()
    assert profiles.num_rows > 0 and _same_table(profiles, want2d)
    assert _same_table(pq.read_table(tmp_path / "profiles" / "vol.parquet"), pq.read_table(tmp_path / "profiles" / "flat.parquet"))
    # the join key: every non-zero Projection_Label is a label of the 2-D table, and every 2-D label appears exactly once
    keys = [int(v) for v in table3d.column("None/None/projection3d/Projection_Label").to_pylist() if v]
    assert sorted(keys) == sorted(profiles.column("metadata_label").to_pylist()) and len(set(keys)) == len(keys)
    # a stack of one plane takes the 2-D path and keeps no volume: the volume step says so
    dP2, prob2 = synth.analytic_flows(volume[0].max(axis=0))
    flat = build_pipeline_steps(**common, volume_features=("intensity3d",))
    flat["steps"]["tile"]["image_kwargs"] = {"source": np.ascontiguousarray(pixels[:, :, :1])}
    flat["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(
        flows_override=lambda x: (torch.from_numpy(dP2[None]).cuda(), torch.from_numpy(prob2[None]).cuda()))
    with pytest.raises(ValueError, match="single plane"):
        run_pipeline_and_post(pipeline=flat, pipeline_name="one_plane", output_path=tmp_path)
