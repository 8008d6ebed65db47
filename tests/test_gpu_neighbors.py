"""
The `neighbors` family on the GPU (aliby_amd/csrc/feat_neighbors.hip) against tests/neighbors_ref.py, the NumPy restatement that
tests/test_cpu_neighbors_ref.py pins to hand values and scipy.ndimage, through every layer: the engine call, the planner's
side-stream fan-out, the extraction tree (plain and overlapping masks) and run_positions.  Parity with cp_measure / CellProfiler is
unpinned (neither can be run here).

Every scene runs at distance None, 2, 5 and 9; at 9 the discs leave the 64 x 64 frames on every side.

Pass bar: NumberOfNeighbors, PercentTouching and the two object numbers (columns 0, 1, 2, 4) bit-equal to the restatement; the two
distances and the angle (columns 3, 5, 6) under the project's float rule, rtol 1e-4, atol 1e-9, NaN equal to NaN.  Every comparison
prints its largest relative error first.  Measured on an MI355X: see `compare`.
"""
import numpy as np
import pytest

from tests import neighbors_ref as ref

pytestmark = pytest.mark.gpu

FLOAT = tuple(c for c in range(7) if c not in ref.EXACT)
_DEVICE = {}


def batches():
    small = ref.small_scenes()
    big = ref.big_scenes()
    return {
        "worked": {"worked": ref.worked()},
        "small": small,
        "high": {"high": ref.high_labels(), "cross": small["cross"]},
        "big": {"big": big["big"], "crowd256": big["crowd256"], "empty256": np.zeros(ref.BIG, np.uint16)},
        "crowd256": {"crowd256": big["crowd256"]},
    }


def device(engine, batch):
    """-> (labels [F,Y,X] on the GPU, object table) of a batch, made once"""
    if batch not in _DEVICE:
        from aliby_amd.extraction.engine import to_device_u16

        dl = to_device_u16(np.stack(list(batches()[batch].values())))
        _DEVICE[batch] = (dl, engine.object_table(dl))
    return _DEVICE[batch]


def want(batch, distance):
    return np.concatenate([ref.expected(name, lab, distance=distance) for name, lab in batches()[batch].items()])


def rows_of(batch, name):
    lo = 0
    for k, lab in batches()[batch].items():
        if k == name:
            return slice(lo, lo + int(lab.max()))
        lo += int(lab.max())
    raise KeyError(name)


def run(engine, batch, distance):
    import torch

    dl, tab = device(engine, batch)
    out = engine.new_output(tab.n_obj, 9)
    assert engine.neighbors(dl, tab, out, 1, distance=distance) == 7
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:, 0]).all() and np.isnan(got[:, 8]).all()  # only columns col0 .. col0 + 6 are written
    return got[:, 1:8].copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def compare(got, wanted, what):
    """Measured on an MI355X, largest relative error of a float column against the restatement over every comparison of this
    file: 2.12e-16 (small batch and the extraction tree; 1.48e-16 in the batch with the 200 x 200 object, 1.54e-16 through
    run_positions, 0 on labels 39 999 / 40 000).  A few parts in 1e16, as expected of one sqrt or atan2: the bar stays the project's."""
    got, wanted = np.asarray(got, float), np.asarray(wanted, float)
    assert got.shape == wanted.shape, (what, got.shape, wanted.shape)
    g, w = got[:, FLOAT], wanted[:, FLOAT]
    both = ~(np.isnan(g) | np.isnan(w))
    rel = np.where(g[both] == w[both], 0.0, np.abs(g[both] - w[both]) / np.maximum(np.abs(w[both]), 1e-300))
    print(f"neighbors {what}: largest relative error of a float column {rel.max() if rel.size else 0.0:.3g} over {len(got)} rows")
    for c in ref.EXACT:
        assert same_bits(got[:, c], wanted[:, c]), (what, ref.STEMS[c], got[:, c], wanted[:, c])
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, g, w)
    assert np.allclose(g, w, rtol=1e-4, atol=1e-9, equal_nan=True), (what, g, w)


# ------------------------------------------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_worked_case(engine, distance):
    got = run(engine, "worked", distance)
    compare(got, want("worked", distance), f"worked d={distance}")
    if distance is None:  # the diagonal contact tells S from T
        assert got[:, 0].tolist() == [1, 1, 0] and got[:, 1].tolist() == [50.0, 75.0, 25.0]
        assert got[0, 2] == 2 and got[0, 3] == 2.0


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_small_batch(engine, distance):
    """Tiles with 0, 1 and 2 objects, objects in every corner and on every edge, a one-pixel object, an object farther than d from
    everything, coincident centres, distance ties, gaps in the numbering and the crowd, in one launch (the ring's 57 x 57 box makes
    it a two-wave launch)."""
    got = run(engine, "small", distance)
    compare(got, want("small", distance), f"small batch d={distance}")
    r = lambda name: got[rows_of("small", name)]  # noqa: E731
    assert r("one").tolist() == [[0.0] * 7]
    assert (r("two")[:, 4:] == 0).all() and r("two")[:, 2].tolist() == [2, 1]
    assert r("sparse")[2, 0] == 0 and r("sparse")[2, 1] == 0.0  # nothing within reach
    ring = r("ring")
    assert ring[1, 2] == 1 and ring[1, 3] == 0.0 and np.isnan(ring[1, 6]) and np.isnan(ring[0, 6]) and ring[2, 6] == 0.0
    cross = r("cross")
    assert cross[2, [2, 4]].tolist() == [1, 2] and cross[0, [2, 4]].tolist() == [3, 2] and cross[4, [2, 4]].tolist() == [3, 2]
    gaps = r("gaps")
    assert np.isnan(gaps[[0, 2, 3, 6, 7]]).all() and not np.isnan(gaps[[1, 4, 5, 8]]).any()
    if distance == 5:
        assert r("crowd")[0, 0] > 64  # counted over a dozen bitmap words


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_labels_39999_and_40000(engine, distance):
    """The bitmap near its upper size (1251 words) and the closest scan over 40 000 rows of which two are present."""
    got = run(engine, "high", distance)
    compare(got, want("high", distance), f"labels 39999, 40000 d={distance}")
    assert np.isnan(got[:39998]).all()
    assert got[39998:40000, 0].tolist() == [1, 1] and got[39998:40000, 2].tolist() == [40000, 39999] and (got[39998:40000, 4:] == 0).all()


@pytest.mark.parametrize("distance", ref.DISTANCES)
def test_big_object_batch_and_alone(engine, distance):
    """A 200 x 200 object makes the launch four waves wide; the crowd tile's rows carry the same bits as when it runs alone (one
    wave)."""
    got = run(engine, "big", distance)
    compare(got, want("big", distance), f"big batch d={distance}")
    alone = run(engine, "crowd256", distance)
    assert same_bits(got[rows_of("big", "crowd256")], alone)


def test_side_stream_fan_out_carries_the_same_bits(engine):
    """Inside the planner's fan-out (sizeshape, zernike and neighbors on side streams) the block is the one of the direct call."""
    import torch

    from aliby_amd.extraction import families

    dl, tab = device(engine, "small")
    assert tab.lds_resident  # the fan-out's condition
    inst = [("None", "None", "sizeshape"), ("None", "None", "neighbors"), ("None", "None", "zernike"), (0, "max", "neighbors")]
    for distance in (None, 5):
        kw = {} if distance is None else {"neighbors": {"distance": distance}}
        matrix, blocks = families.evaluate(engine, dl, tab, None, inst, kw)
        torch.cuda.synchronize()
        m = matrix.cpu().numpy()
        direct = run(engine, "small", distance)
        assert blocks[1] == (78, ref.names(distance)) and blocks[3][1] == ref.names(distance)
        assert same_bits(m[:, 78:85], direct) and same_bits(m[:, blocks[3][0] : blocks[3][0] + 7], direct)


def test_bad_distance_is_refused(engine):
    dl, tab = device(engine, "worked")
    out = engine.new_output(tab.n_obj, 7)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            engine.neighbors(dl, tab, out, 0, distance=bad)
    fn = engine.lib.aliby_features_neighbors  # the C entry keeps the cap too
    import torch

    centres = torch.empty((tab.n_obj, 2), dtype=torch.float64, device="cuda")
    off = torch.from_numpy(tab.offsets).cuda()
    args = lambda d: (engine.ctx.handle, dl.data_ptr(), 1, 6, 8, tab.dev.data_ptr(), tab.n_obj, tab.max_h, tab.max_w, off.data_ptr(), 3,  # noqa: E731
                      d, centres.data_ptr(), out.data_ptr(), 7, 0, torch.cuda.current_stream().cuda_stream)
    assert fn(*args(65)) == 1 and fn(*args(0)) == 1 and fn(*args(64)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ through the layers
TREE = {"None": {"None": ["sizeshape", "neighbors"]}}


@pytest.mark.parametrize("distance", [None, 5])
def test_process_tree_masks(engine, distance):
    from aliby_amd.extraction.extract import extract_tree, format_extraction, process_tree_masks

    sc = ref.small_scenes()
    masks = [sc[k] for k in ("corners_edges", "empty", "gaps", "cross")]
    kw = {} if distance is None else {"cp_measure_kwargs": {"neighbors": {"distance": distance}}}
    inst, res = process_tree_masks(TREE, masks, None, extract_tree, **kw)
    t = format_extraction((inst, res))
    keys = [f"None/None/neighbors/{n}" for n in ref.names(distance)]
    assert sorted(c for c in t.column_names if "/neighbors/" in c) == sorted(keys)
    assert ("None/None/neighbors/Neighbors_NumberOfNeighbors_Adjacent" in t.column_names) == (distance is None)
    assert "None/None/sizeshape/Area" in t.column_names
    wanted = np.concatenate([ref.expected(k, sc[k], distance=distance) for k in ("corners_edges", "empty", "gaps", "cross")])
    got = np.stack([np.asarray(t[k].to_numpy(zero_copy_only=False), float) for k in keys], axis=1)
    assert t.num_rows == len(wanted)
    compare(got, wanted, f"process_tree_masks d={distance}")


def test_overlapping_masks_measure_each_plane_on_its_own(engine):
    from functools import partial

    from aliby_amd.extraction.extract import extract_tree, process_tree_masks_overlap

    sc = ref.small_scenes()
    masks = [np.stack([sc["two"], sc["cross"]]).astype(np.int32), sc["corners_edges"][None].astype(np.int32)]
    inst, res = process_tree_masks_overlap(TREE, masks, None, partial(extract_tree, overlap=True))
    objs = list(dict.fromkeys(t[0] for t in inst))
    assert len(res) == 2 * len(objs)
    got = np.asarray([[res[2 * i + 1][n][0] for n in ref.names(None)] for i in range(len(objs))], float)
    wanted = np.concatenate([ref.expected(k, sc[k]) for k in ("two", "cross", "corners_edges")])
    compare(got, wanted, "overlap planes")


def test_run_positions_writes_the_columns(tmp_path, engine):
    import pyarrow.parquet
    from aliby_amd import synth
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe_builder import build_pipeline_steps
    from tests.test_gpu_configs import _keyed_override

    fovs = [synth.make_fov(2, 80 + i, shape=(224, 256), n_channels=2, n_target=8) for i in range(2)]
    override = _keyed_override(fovs)
    pipes = []
    for f in fovs:
        p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[1], features_to_extract=("intensity", "neighbors"),
                                 cp_measure_feature_kwargs={"neighbors": {"distance": 9}})
        p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
        p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
        pipes.append(p)
    names = ["N00__1", "N01__1"]
    got = run_positions(pipes, names, tmp_path, batch_size=2)
    keys = [f"1/max/neighbors/{n}" for n in ref.names(9)]
    for (prof, _), nm in zip(got, names):
        on_disk = pyarrow.parquet.read_table(tmp_path / "profiles" / f"{nm}.parquet")
        assert set(keys) <= set(on_disk.column_names) and prof.num_rows > 1
        with np.load(tmp_path / "steps" / nm / "segment_nuclei" / "0000.npz") as z:
            lab = z["arr_0"].reshape(224, 256)
        wanted = ref.neighbors(lab, distance=9)[prof["metadata_label"].to_numpy() - 1]
        compare(np.stack([on_disk[k].to_numpy() for k in keys], axis=1), wanted, f"run_positions {nm}")
