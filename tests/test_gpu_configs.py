"""
BASELINE.json's configurations exercised AS configurations on the GPU (VERDICT r1 "Next round" 1a/1b), through the step
API and the C ABI, against the CPU oracle:

  * C2-shaped: one 1024x1024, 5-channel FOV with ~256 nuclei, the builder's full default mono + multi trees through
    build_pipeline_steps -> run_pipeline_and_post; a fixed subsample of objects against the oracle at 1e-4, every object
    through size-independent properties (finite values, Area == bincount, row order, label image bit-exact);
  * C4-shaped: a 512x512, Z=5 time-lapse with a drifting trap grid: trap detection + drift + per-tile segmentation + IoU
    tracking + sizeshape/intensity in ONE pipeline, T = 10, checked against the oracle and the committed trap fixture
    (tests/golden/reference_traps.json = outputs of the reference's own segment_traps);
  * the reference's own analytic tests (tests/extraction/test_volume.py:32-74: discs / ellipses within 1 % of closed form),
    driven directly at aliby_features_cell;
  * per-metric colocalisation kwargs.
"""

import json
from copy import deepcopy
from pathlib import Path

import numpy as np
import pytest

from aliby_amd import synth

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"


# ----------------------------------------------------------------------------------------------------------- C2
def test_config2_full_default_tree_1024_5ch(tmp_path, engine):
    import pyarrow.parquet
    import torch

    from aliby_amd.extraction.extract import format_extraction
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps
    from oracle import aliby_extract as ox
    from oracle import cellpose_restated as cr

    f = synth.make_fov(2, 0)  # 5 x 1 x 1024 x 1024, ~250 nuclei
    assert f["pixels"].shape == (5, 1, 1024, 1024)
    dP, prob = synth.analytic_flows(f["nuclei"])
    pipeline = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1, 2, 3, 4])
    trees = {k: deepcopy(pipeline["steps"][k]["tree"]) for k in ("extract_nuclei", "extractmulti_nuclei")}
    pipeline["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
    pipeline["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(
        flows_override=lambda x: (torch.from_numpy(dP[None]).cuda(), torch.from_numpy(prob[None]).cuda()))
    profiles, _ = run_pipeline_and_post(pipeline=pipeline, pipeline_name="C2__0", output_path=tmp_path)

    # ---- segmentation: label image bit-exact vs the oracle's dynamics
    want_mask = cr.finish_labels(cr.compute_masks(dP, prob))
    with np.load(tmp_path / "steps" / "C2__0" / "segment_nuclei" / "0000.npz") as z:
        got_mask = z["arr_0"]
    assert np.array_equal(got_mask, want_mask)
    n = int(want_mask.max())
    assert 200 <= n <= 300

    # ---- table shape: 4 metadata + sizeshape + 5 x the six per-channel families + 10 pairs x 8 colocalisation keys
    per_channel = 60 + 21 + 2 + 52 + 12 + 30
    assert len(profiles.column_names) == 4 + 78 + 5 * per_channel + 10 * 8 == 1047
    assert profiles.num_rows == n
    got = profiles.to_pandas()
    assert got["metadata_label"].tolist() == list(range(1, n + 1))  # first-seen (tile, label) row order
    assert (got["metadata_tile"] == 0).all() and (got["metadata_object"] == "nuclei").all() and (got["metadata_tp"] == 0).all()
    on_disk = pyarrow.parquet.read_table(tmp_path / "profiles" / "C2__0.parquet")
    assert on_disk.schema.equals(profiles.schema)
    assert all(np.array_equal(on_disk[c].to_numpy(), profiles[c].to_numpy(), equal_nan=True) for c in profiles.column_names
               if c != "metadata_object")

    # ---- every object: size-independent properties
    area = np.bincount(want_mask.ravel())[1:]
    assert np.array_equal(got["None/None/sizeshape/Area"].to_numpy(), area.astype(float))
    values = got.drop(columns=["metadata_object"])
    nan_cols = sorted(c for c in values.columns if not np.isfinite(values[c].to_numpy(float)).all())
    # NaN only where the definition is: scikit-image's normalised moments of order < 2
    assert nan_cols == [f"None/None/sizeshape/NormalizedMoment_{i}_{j}" for i, j in ((0, 0), (0, 1), (1, 0))], nan_cols
    for c in range(5):
        px = f["pixels"][c, 0].astype(np.float64)
        tot = np.bincount(want_mask.ravel(), weights=px.ravel())[1:]
        assert np.allclose(got[f"{c}/max/intensity/Intensity_IntegratedIntensity"].to_numpy(), tot, rtol=1e-12)
        for metric, keys in (("manders_fold", ("Manders_1", "Manders_2")), ("rwc", ("RWC_1", "RWC_2")), ("costes", ("Costes_1", "Costes_2"))):
            for c1 in range(c + 1, 5):
                for key in keys:
                    v = got[f"({c}, {c1})/None/max/{metric}/Correlation_{key}"].to_numpy()
                    assert ((v >= 0) & (v <= 1 + 1e-12)).all(), (c, c1, key)

    # ---- a fixed subsample of objects against the oracle run in the reference's structure (per-object full-frame masks)
    sample = sorted({1, 2, n // 5, n // 3, n // 2, (2 * n) // 3, n - 1, n})
    objects = [(0, l) for l in sample]
    pixels = f["pixels"][None]
    t1 = format_extraction(ox.process_tree_masks(trees["extract_nuclei"], want_mask, pixels, ox.extract_tree, objects=objects))
    t2 = format_extraction(ox.process_tree_masks(trees["extractmulti_nuclei"], want_mask, pixels, ox.extract_tree_multi,
                                                 objects=objects))
    want = t1.to_pandas().merge(t2.to_pandas(), on=["tile", "label"]).set_index("label").sort_index()
    assert want.index.tolist() == sample
    sub = got.set_index("metadata_label").loc[sample]
    assert set(want.columns) - {"tile"} == set(got.columns) - {"metadata_tile", "metadata_label", "metadata_object", "metadata_tp"}
    worst = 0.0
    for col in want.columns:
        if col == "tile":
            continue
        a, b = sub[col].to_numpy(float), want[col].to_numpy(float)
        if col.endswith("Orientation"):
            flip = np.isclose(np.abs(a), 45.0) & np.isclose(np.abs(b), 45.0)
            a, b = a[~flip], b[~flip]
        if "ZernikePhase" in col:  # a phase is defined modulo 2 pi, and undefined where the magnitude vanishes
            mag = sub[col.replace("Phase", "Magnitude")].to_numpy(float)
            d = np.abs(np.angle(np.exp(1j * (a - b))))
            assert (d[mag > 1e-9] < 1e-4).all(), col
            continue
        assert np.allclose(a, b, rtol=1e-4, atol=1e-8, equal_nan=True), (col, a, b)  # north_star: float features within 1e-4 rel
        ok = np.isfinite(a) & np.isfinite(b) & (np.abs(b) > 1e-6)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))))
    print(f"C2 parity: {len(sample)} objects x {len(want.columns) - 1} columns, worst relative error {worst:.2e}")


# ----------------------------------------------------------------------------------------------------------- C4
def test_config4_traps_drift_track_extract_in_one_pipeline(tmp_path, engine):
    import torch

    from aliby_amd.extraction.extract import format_extraction
    from aliby_amd.pipe import init_step
    from aliby_amd.pipe_core import get_profiles_from_state, run_pipeline_return_state
    from oracle import aliby_extract as ox
    from oracle import cellpose_restated as cr
    from oracle import tiler_ref
    from oracle.drift_restated import phase_cross_correlation as oracle_pcc
    from oracle.track_restated import stitch_rois as oracle_rois
    from oracle.traps_restated import segment_traps as oracle_traps

    T, tile, half = 10, 117, 117 // 2
    tl = synth.make_timelapse(T=T, seed=11)
    frames = tl["pixels"]  # [T,1,5,512,512]

    # ---------------- oracle side: trap centres, drifts, windows, per-tile masks, tracks, features
    fixture = json.loads((G / "reference_traps.json").read_text())["cases"][0]
    assert fixture["seed"] == 11 and fixture["tile_size"] == tile
    found = [tuple(int(v) for v in c) for c in oracle_traps(frames[0, 0, 0], tile)]
    assert found == [tuple(c) for c in fixture["segment_traps"]]  # the reference's own segment_traps output, cells or not
    centres = [c for c in found if half < c[0] < 512 - half and half < c[1] < 512 - half]
    assert len(centres) == 9
    drifts, o_pixels, o_masks, o_flows = [], [], [], []
    for t in range(T):
        drifts.append(oracle_pcc(frames[max(0, t - 1), 0, 0], frames[t, 0, 0]).tolist())
        cum = np.sum(drifts, axis=0)
        ranges = []
        for cy, cx in centres:
            y, x = (np.array([cy, cx]) - cum).astype(int)
            ranges.append((slice(int(y) - half, int(y) - half + tile), slice(int(x) - half, int(x) - half + tile)))
        assert all(r[0].start >= 0 and r[1].start >= 0 and r[0].stop <= 512 and r[1].stop <= 512 for r in ranges)
        o_pixels.append(tiler_ref.get_fczyx(frames[t], ranges))  # [9,1,5,117,117]
        gt = [tl["labels"][t][r] for r in ranges]
        flows = [synth.analytic_flows(tiler_ref.relabel_sequential(g)) for g in gt]
        o_flows.append((np.stack([fl[0] for fl in flows]), np.stack([fl[1] for fl in flows])))
        o_masks.append([cr.finish_labels(cr.compute_masks(*fl)) for fl in flows])
    assert np.array_equal(np.array(drifts[1:]), -np.diff(tl["shifts"], axis=0).astype(float))  # the walk that was applied
    tree = {"None": {"None": ["sizeshape"]}, 0: {"max": ["intensity"]}}

    # ---------------- GPU side: ONE pipeline dict through the engine
    calls = {"n": 0}

    def override(x):  # x: device uint16 [F,117,117] = max over Z of the tile stack of this timepoint
        t = calls["n"]
        calls["n"] += 1
        assert np.array_equal(x.cpu().numpy(), o_pixels[t][:, 0].max(axis=1)), f"tile windows differ at tp {t}"
        return torch.from_numpy(o_flows[t][0]).cuda(), torch.from_numpy(o_flows[t][1]).cuda()

    pipeline = {
        "ntps": T,
        "steps": {
            "tile": {"image_kwargs": {"source": frames}, "tile_size": tile, "ref_channel": 0, "calculate_drift": True},
            "segment_cells": {"segmenter_kwargs": {"kind": "cellpose", "per_tile": True, "setup_params": {"flows_override": override}},
                              "channel_to_segment": 0},
            "track": {"kind": "stitch", "stitch_threshold": 0.25},
            "extract_cells": {"tree": tree},
        },
        "passed_data": {"track": [("masks", "segment_cells"), ("track_info", "track")],
                        "extract_cells": [("masks", "segment_cells"), ("pixels", "tile")]},
        "passed_methods": {"segment_cells": ("tile", "get_fczyx")},
        "save": ("segment_cells",),
        "save_interval": 1,
        "retain": {"tile": 1, "segment_cells": 2},
    }
    state = run_pipeline_return_state(pipeline, tmp_path / "steps" / "pos", init_step)
    assert calls["n"] == T
    tiler = state["fn"]["tile"]
    assert [list(map(int, c)) for c in tiler.tile_locs.initial_location] == [list(c) for c in centres]
    assert tiler.tile_locs.drifts == drifts

    # masks written per timepoint: a list result goes through np.asarray -> one stacked `arr_0` (write.py:25-51)
    for t in range(T):
        with np.load(tmp_path / "steps" / "pos" / "segment_cells" / f"{t:04d}.npz") as z:
            assert list(z.keys()) == ["arr_0"] and z["arr_0"].shape == (9, tile, tile)
            for k in range(9):
                assert np.array_equal(z["arr_0"][k], o_masks[t][k]), (t, k)

    # tracks: same state machine as the engine's wiring, on the oracle's masks
    info = None
    for t in range(T):
        if t == 0:
            want = {k: {"labels": list(range(1, int(o_masks[0][k].max()) + 1)), "max_label": int(o_masks[0][k].max())} for k in range(9)}
        else:
            want = oracle_rois([[o_masks[t - 1][k], o_masks[t][k]] for k in range(9)], info)
        assert dict(state["data"]["track"][t]) == want, t
        info = want
    # cells are born, none vanish and the tiles follow the sample: identities persist, new cells get new ids
    last = state["data"]["track"][-1]
    assert all(sorted(last[k]["labels"]) == list(range(1, last[k]["max_label"] + 1)) for k in range(9))
    assert all(last[k]["max_label"] == 3 for k in range(9))

    # features
    profiles = get_profiles_from_state(state, pipeline).to_pandas()
    assert sorted(profiles["metadata_tp"].unique().tolist()) == list(range(T))
    for t in range(T):
        want = format_extraction(ox.process_tree_masks(tree, o_masks[t], o_pixels[t], ox.extract_tree)).to_pandas()
        sub = profiles[profiles["metadata_tp"] == t]
        assert sub[["metadata_tile", "metadata_label"]].to_numpy().tolist() == want[["tile", "label"]].to_numpy().tolist()
        for col in want.columns:
            if col in ("tile", "label") or col.endswith("Orientation"):
                continue
            assert np.allclose(sub[col].to_numpy(float), want[col].to_numpy(float), rtol=1e-4, atol=1e-8, equal_nan=True), (t, col)


# --------------------------------------------------------------------------------- the reference's analytic cell.py tests
def _ellipse(x, y, rotate):
    """Pixels strictly inside the rotated ellipse of semi-axes (x rows, y cols) centred in a (4x, 4y) frame."""
    rr, cc = np.mgrid[: 4 * x, : 4 * y].astype(np.float64)
    r, c = rr - 2 * x, cc - 2 * y
    phi = np.deg2rad(rotate) % np.pi
    a = (r * np.cos(phi) + c * np.sin(phi)) / x
    b = (r * np.sin(phi) - c * np.cos(phi)) / y
    return a * a + b * b < 1


def test_reference_volume_tests_on_the_gpu_kernel(engine):
    """tests/extraction/test_volume.py:32-74 (the only numeric assertions the reference holds on this path): volume of
    discs and rotated ellipses, min/maj axis approximation and eccentricity, with the reference's own thresholds and
    parametrisation (9 radii x 9 eccentricities x 9 rotations + 9 discs), evaluated by aliby_features_cell through the C ABI."""
    from aliby_amd.extraction.engine import to_device_u16

    threshold = 0.01
    radii = list(range(10, 100, 10))
    eccentricities = np.arange(0, 0.9, 0.1)
    rotations = [10, 20, 30, 40, 50, 60, 70, 80, 90]
    cols = {n: engine.CELL_COLUMNS.index(n) for n in ("volume", "min_ax", "maj_ax", "eccentricity", "area")}
    n_cases = 0
    for x in radii:
        cases = [(x, int(np.round(np.sqrt(x**2 / (1 - ecc**2)))), rot) for ecc in eccentricities for rot in rotations]
        H, W = 4 * x, 4 * max(c[1] for c in cases)
        stack = np.zeros((len(cases) + 1, max(H, 2 * x + 1), max(W, 2 * x + 1)), np.uint16)
        for k, (xx, yy, rot) in enumerate(cases):
            stack[k, : 4 * xx, : 4 * yy] = _ellipse(xx, yy, rot)
        gy, gx = np.mgrid[-x : x + 1, -x : x + 1]
        stack[-1, : 2 * x + 1, : 2 * x + 1] = gx * gx + gy * gy <= x * x  # skimage.morphology.disk(x)
        dl = to_device_u16(stack)
        tab = engine.object_table(dl)
        assert tab.n_obj == len(cases) + 1
        out = engine.cell_metrics(dl, None, 0, 0, tab).cpu().numpy()
        assert np.array_equal(out[:, cols["area"]], stack.reshape(len(stack), -1).sum(1).astype(float))
        for k, (xx, yy, rot) in enumerate(cases):
            v, mn, mj, e = (out[k, cols[n]] for n in ("volume", "min_ax", "maj_ax", "eccentricity"))
            real_v = 4 * np.pi * xx * yy * xx / 3
            assert abs(v - real_v) / real_v < threshold, (xx, yy, rot, v, real_v)  # test_volume_ellipsoid
            assert np.allclose([mn, mj], [xx, yy], rtol=threshold * min(xx, yy)), (xx, yy, rot, mn, mj)  # test_approximation
            real_ecc = np.sqrt(yy**2 - xx**2) / yy
            assert np.isclose(real_ecc, e, rtol=threshold * real_ecc), (xx, yy, rot, e, real_ecc)  # test_roundness
            n_cases += 3
        real_v = 4 * np.pi * x**3 / 3
        assert abs(out[-1, cols["volume"]] - real_v) / real_v < threshold  # test_volume_circular
        n_cases += 1
    assert n_cases == 2196  # the count the reference's own run reports


# --------------------------------------------------------------------------------- per-metric colocalisation kwargs
def test_coloc_kwargs_are_per_metric(engine):
    """cp_measure_kwargs={'manders_fold': {'thr': 30}} must leave rwc at its default thr=15 (loaders.py:71-77 bakes kwargs
    into one partial per feature name); both thresholds in one tree."""
    from aliby_amd.extraction.extract import extract_tree_multi, process_tree_masks
    from oracle import aliby_extract as ox

    f = synth.make_fov(1, 3, shape=(256, 256), n_channels=3, n_target=20)
    labels, pixels = f["nuclei"], f["pixels"][None]
    tree = {(0, 1): {"None": {"max": ["pearson", "manders_fold", "rwc", "costes"]}},
            (1, 2): {"None": {"max": ["manders_fold", "rwc"]}}, (0, 2): {"None": {"max": ["rwc"]}}}
    for kw in ({"manders_fold": {"thr": 30}}, {"rwc": {"thr": 40}, "manders_fold": {"thr": 5}}, {}):
        inst, res = process_tree_masks(tree, labels, pixels, extract_tree_multi, cp_measure_kwargs=kw)
        inst_o, res_o = ox.process_tree_masks(tree, labels, pixels, ox.extract_tree_multi, cp_measure_kwargs=kw)
        assert inst == inst_o and len(res) == len(res_o)
        for a, b in zip(res, res_o):
            for k in b:
                assert np.allclose(a[k], b[k], rtol=1e-4, atol=1e-9, equal_nan=True), (kw, k)
    # and the two settings really differ on this data
    a = process_tree_masks(tree, labels, pixels, extract_tree_multi, cp_measure_kwargs={"manders_fold": {"thr": 60}})[1]
    b = process_tree_masks(tree, labels, pixels, extract_tree_multi, cp_measure_kwargs={})[1]
    assert any(not np.allclose(x["Correlation_Manders_1"], y["Correlation_Manders_1"]) for x, y in zip(a, b) if "Correlation_Manders_1" in x)
    assert all(np.allclose(x["Correlation_RWC_1"], y["Correlation_RWC_1"]) for x, y in zip(a, b) if "Correlation_RWC_1" in x)
    # a keyword the kernels do not implement is refused, not dropped (the reference hands it to the cp_measure function, where
    # an unknown keyword is an error too); keywords of families that the tree does not use are nobody's business
    from aliby_amd.extraction.extract import extract_tree

    with pytest.raises(NotImplementedError, match="costes"):
        process_tree_masks(tree, labels, pixels, extract_tree_multi, cp_measure_kwargs={"costes": {"fast_costes": "Accurate"}})
    mono = {0: {"max": ["intensity"]}, "None": {"None": ["sizeshape"]}}
    with pytest.raises(NotImplementedError, match="sizeshape"):
        process_tree_masks(mono, labels, pixels, extract_tree, cp_measure_kwargs={"sizeshape": {"calculate_advanced": False}})
    process_tree_masks(mono, labels, pixels, extract_tree, cp_measure_kwargs={"texture": {"no_such": 1}})  # (texture is not in the tree)


# --------------------------------------------------------------------------------- the position-batched runner
def _keyed_override(fovs, key_channel=0):
    """flows_override for a batch: each plane of x [N,Y,X] is looked up by its bytes, so the same closure serves single calls
    (N = 1) and batched calls (N = positions) in any order."""
    import torch

    table = {}
    for f in fovs:
        dP, prob = synth.analytic_flows(f["nuclei"])
        table[f["pixels"][key_channel].max(axis=0).tobytes()] = (dP, prob)

    def override(x):
        host = x.cpu().numpy()
        flows = [table[host[i].tobytes()] for i in range(host.shape[0])]
        return (torch.from_numpy(np.stack([fl[0] for fl in flows])).cuda(), torch.from_numpy(np.stack([fl[1] for fl in flows])).cuda())

    return override


def test_run_positions_writes_what_single_calls_write(tmp_path, engine):
    """aliby_amd.runner.run_positions (B positions per device step) against N calls of run_pipeline_and_post: the same
    parquet bytes, the same mask arrays, the same returned tables; resume-by-skip per position (pipe_core.py:408,446-448)."""
    import pyarrow.parquet

    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    n = 7
    fovs = [synth.make_fov(2, 40 + i, shape=(224, 256), n_channels=3, n_target=10 + i) for i in range(n)]
    override = _keyed_override(fovs)

    def pipelines():
        out = []
        for f in fovs:
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1, 2],
                                     cp_measure_feature_kwargs={"texture": {"scale": 2}})
            p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            out.append(p)
        return out

    names = [f"P{i:02d}__1" for i in range(n)]
    single, batched = tmp_path / "single", tmp_path / "batched"
    want = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=single)[0] for p, nm in zip(pipelines(), names)]
    got = run_positions(pipelines(), names, batched, batch_size=3)  # batches of 3, 3, 1
    assert len(got) == n
    for i, nm in enumerate(names):
        prof, post = got[i]
        assert post == {} and prof.schema.equals(want[i].schema) and prof.num_rows == want[i].num_rows > 0
        for c in prof.column_names:
            a, b = prof[c].to_numpy(zero_copy_only=False), want[i][c].to_numpy(zero_copy_only=False)
            assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), (nm, c)
        assert (batched / "profiles" / f"{nm}.parquet").read_bytes() == (single / "profiles" / f"{nm}.parquet").read_bytes()
        with np.load(batched / "steps" / nm / "segment_nuclei" / "0000.npz") as za, \
                np.load(single / "steps" / nm / "segment_nuclei" / "0000.npz") as zb:
            assert list(za.keys()) == list(zb.keys()) == ["arr_0"] and np.array_equal(za["arr_0"], zb["arr_0"])
    # resume: nothing to do -> (None, None) everywhere; after deleting one file only that position is redone
    assert run_positions(pipelines(), names, batched, overwrite=False) == [(None, None)] * n
    (batched / "profiles" / f"{names[4]}.parquet").unlink()
    again = run_positions(pipelines(), names, batched, overwrite=False)
    assert [a[0] is not None for a in again] == [i == 4 for i in range(n)]
    assert (batched / "profiles" / f"{names[4]}.parquet").read_bytes() == (single / "profiles" / f"{names[4]}.parquet").read_bytes()


def test_eight_bit_sources_through_the_pipeline(tmp_path, engine):
    """uint8 stacks (8-bit TIFF plates): stored as uint16 on the device, handed on as uint8, and measured as the reference's
    CPU path measures uint8 arrays — in particular `texture`, whose grey levels are the values themselves for uint8
    (skimage.util.img_as_ubyte) and value >> 8 for uint16.  Single calls, the position-batched runner and the oracle agree."""
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps
    from oracle import texture_restated as tx

    fovs = [synth.make_fov(2, 140 + i, shape=(224, 256), n_channels=2, n_target=8) for i in range(3)]
    px8 = [(f["pixels"] >> 6).clip(0, 255).astype(np.uint8) for f in fovs]
    assert all(len(np.unique(p)) > 100 for p in px8)
    override = _keyed_override([dict(nuclei=f["nuclei"], pixels=p.astype(np.uint16)) for f, p in zip(fovs, px8)])

    def pipelines(widen):
        out = []
        for p8 in px8:
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1],
                                     features_to_extract=("sizeshape", "intensity", "texture"))
            p["steps"]["tile"]["image_kwargs"] = {"source": (p8.astype(np.uint16) if widen else p8)[None]}
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            out.append(p)
        return out

    names = [f"E{i}" for i in range(3)]
    single = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=tmp_path / "s8")[0] for p, nm in zip(pipelines(False), names)]
    batched = [r[0] for r in run_positions(pipelines(False), names, tmp_path / "b8", batch_size=3)]
    wide = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=tmp_path / "s16")[0] for p, nm in zip(pipelines(True), names)]
    for i, nm in enumerate(names):
        assert single[i].num_rows == batched[i].num_rows == wide[i].num_rows > 0
        with np.load(tmp_path / "s8" / "steps" / nm / "segment_nuclei" / "0000.npz") as z:
            labels = z["arr_0"]
        for c in single[i].column_names:
            a = single[i][c].to_numpy(zero_copy_only=False)
            b = batched[i][c].to_numpy(zero_copy_only=False)
            w = wide[i][c].to_numpy(zero_copy_only=False)
            if a.dtype.kind != "f":
                assert np.array_equal(a, b) and np.array_equal(a, w), c
                continue
            assert np.allclose(a, b, rtol=1e-9, atol=1e-12, equal_nan=True), c
            if "/texture/" not in c:
                assert np.allclose(a, w, rtol=1e-9, atol=1e-12, equal_nan=True), c  # (the same values in either storage)
        for ch in (0, 1):
            ref = tx.get_texture(labels, px8[i][ch].max(axis=0))
            for key, want in ref.items():
                got = single[i][f"{ch}/max/texture/{key}"].to_numpy(zero_copy_only=False)
                assert np.allclose(got, want, rtol=1e-4, atol=1e-8, equal_nan=True), (nm, ch, key)
            ent = single[i][f"{ch}/max/texture/Entropy_3_00_256"].to_numpy(zero_copy_only=False)
            assert np.nanmax(ent) > 1.0  # (value >> 8 would have left one grey level: no entropy at all)


def test_float_sources_through_the_pipeline(tmp_path, engine):
    """float stacks (data normalised upstream): float32 on the device, one tile per position; single calls and the batched
    runner agree, the numbers are those of the float pixels (checked on the mean intensity against NumPy)."""
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    fovs = [synth.make_fov(2, 150 + i, shape=(224, 256), n_channels=2, n_target=8) for i in range(2)]
    pf = [(f["pixels"].astype(np.float32) / np.float32(30000.0)).clip(0, 1) for f in fovs]
    override = _keyed_override([dict(nuclei=f["nuclei"], pixels=p) for f, p in zip(fovs, pf)])

    def pipelines(dtype):
        out = []
        for p32 in pf:
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1],
                                     features_to_extract=("sizeshape", "intensity", "texture"))
            p["steps"]["tile"]["image_kwargs"] = {"source": p32.astype(dtype)[None]}
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            out.append(p)
        return out

    names = ["F0", "F1"]
    single = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=tmp_path / "s")[0] for p, nm in zip(pipelines(np.float32), names)]
    batched = [r[0] for r in run_positions(pipelines(np.float32), names, tmp_path / "b", batch_size=2)]
    double = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=tmp_path / "d")[0] for p, nm in zip(pipelines(np.float64), names)]
    for i, nm in enumerate(names):
        assert single[i].num_rows == batched[i].num_rows == double[i].num_rows == int(fovs[i]["nuclei"].max())
        for c in single[i].column_names:
            a, b, d = (t[i][c].to_numpy(zero_copy_only=False) for t in (single, batched, double))
            if a.dtype.kind != "f":
                assert np.array_equal(a, b) and np.array_equal(a, d), c
            else:
                assert np.allclose(a, b, rtol=1e-9, atol=1e-12, equal_nan=True), c
                assert np.allclose(a, d, rtol=1e-9, atol=1e-12, equal_nan=True), c  # (float64 stacks are float32 on the device)
        with np.load(tmp_path / "s" / "steps" / nm / "segment_nuclei" / "0000.npz") as z:
            labels = z["arr_0"]
        want = np.array([pf[i][1, 0][labels == k].astype(np.float64).mean() for k in range(1, int(labels.max()) + 1)])
        got = single[i]["1/max/intensity/Intensity_MeanIntensity"].to_numpy(zero_copy_only=False)
        assert np.allclose(got, want, rtol=1e-6)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_run_positions_mixed_save_and_host_only_steps(tmp_path, engine):
    """Two things a batch must not get wrong (VERDICT r2 items 8 / ADVICE r2): (i) positions whose `save` lists differ do not
    share a device batch — the one that saves its tile step gets the same .npz a single call writes; (ii) a step without a
    batched form (here a custom host-side consumer of `masks`, wired with passed_data like pipe_core.py:188-205) sees finished
    label arrays, not a pinned buffer whose download is still in flight."""
    import zlib

    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import init_step, run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    n = 6
    fovs = [synth.make_fov(2, 70 + i, shape=(224, 256), n_channels=2, n_target=8 + i) for i in range(n)]
    override = _keyed_override(fovs)
    seen = {}

    def init(name, params, other=None):
        if name.startswith("hostsum"):
            def consume(masks, **kw):
                arr = masks[0] if isinstance(masks, list) else masks
                key = int(params["position"])
                seen.setdefault(key, []).append((zlib.crc32(np.ascontiguousarray(arr).tobytes()), int(arr.max())))
                return {"crc": seen[key][-1][0]}
            return consume
        return init_step(name, params, other)

    def pipelines(with_host_step):
        out = []
        for i, f in enumerate(fovs):
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("intensity",))
            p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            if i in (1, 2, 4):
                p["save"] = ("tile", "segment_nuclei")
            if with_host_step:
                steps = {}
                for k, v in p["steps"].items():  # right after the segmenter: the download has had no time to finish
                    steps[k] = v
                    if k == "segment_nuclei":
                        steps["hostsum_nuclei"] = {"position": i}
                p["steps"] = steps
                p["passed_data"]["hostsum_nuclei"] = [("masks", "segment_nuclei")]
            out.append(p)
        return out

    names = [f"Q{i:02d}" for i in range(n)]
    single, batched = tmp_path / "single", tmp_path / "batched"
    for p, nm in zip(pipelines(False), names):
        run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=single)
    got = run_positions(pipelines(True), names, batched, batch_size=4, init_step_fn=init)
    assert all(g[0] is not None and g[0].num_rows > 0 for g in got)
    for i, nm in enumerate(names):
        assert (batched / "profiles" / f"{nm}.parquet").read_bytes() == (single / "profiles" / f"{nm}.parquet").read_bytes()
        with np.load(single / "steps" / nm / "segment_nuclei" / "0000.npz") as z:
            masks = z["arr_0"]
        assert seen[i] == [(zlib.crc32(np.ascontiguousarray(masks).tobytes()), int(masks.max()))], nm
        tile_npz = batched / "steps" / nm / "tile" / "0000.npz"
        assert tile_npz.exists() == (i in (1, 2, 4))
        if tile_npz.exists():
            # (the reference writes a tile step's dict as a pickled 0-d object array, write.py:50; both files are this test's own)
            with np.load(tile_npz, allow_pickle=True) as za, np.load(single / "steps" / nm / "tile" / "0000.npz", allow_pickle=True) as zb:
                da, db = za["arr_0"].item(), zb["arr_0"].item()
                assert sorted(da) == sorted(db) == ["drift", "pixels"] and np.array_equal(da["pixels"], db["pixels"])
                assert _same(da["drift"], db["drift"])


def test_run_positions_with_an_empty_position_and_a_large_object(tmp_path, engine):
    """Batches whose frames are not alike: one position without any object (its count is 0 in the object table the runner
    builds from the segmenter's counts), one with an object wider than the LDS-resident window (the per-object kernels take
    their global-scratch variants, and neither the family fan-out nor the side-by-side colocalisation launch is taken), among
    ordinary ones — against single calls, table for table."""
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    shape = (224, 256)
    fovs = [synth.make_fov(2, 60 + i, shape=shape, n_channels=2, n_target=8) for i in range(4)]
    rng = np.random.default_rng(9)
    empty = dict(pixels=rng.integers(90, 140, (2, 1, *shape)).astype(np.uint16), nuclei=np.zeros(shape, np.uint16))
    yy, xx = np.mgrid[0 : shape[0], 0 : shape[1]]
    big_lab = ((yy - 110) ** 2 + (xx - 128) ** 2 <= 50**2).astype(np.uint16)
    big = dict(pixels=(rng.integers(90, 140, (2, 1, *shape)) + 400 * big_lab).astype(np.uint16), nuclei=big_lab)

    def run(order, batch_size, out):
        override = _keyed_override(order)

        def pipes():  # (a pipeline dict is consumed by its run: init_step pops image_kwargs, as the reference does)
            made = []
            for f in order:
                p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1],
                                         features_to_extract=("sizeshape", "intensity", "texture", "radial_distribution", "zernike"))
                p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
                p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
                made.append(p)
            return made

        names = [f"Q{i:02d}__1" for i in range(len(order))]
        single = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=out / "single")[0] for p, nm in zip(pipes(), names)]
        got = run_positions(pipes(), names, out / "batched", batch_size=batch_size)
        return single, [g[0] for g in got]

    for k, (order, bs) in enumerate((([fovs[0], empty, fovs[1]], 3), ([fovs[2], big, fovs[3], empty], 4), ([empty], 1))):
        single, got = run(order, bs, tmp_path / f"case{k}")
        for i, (a, b) in enumerate(zip(got, single)):
            assert a.schema.equals(b.schema) and a.num_rows == b.num_rows, (k, i, a.num_rows, b.num_rows)
            for c in a.column_names:
                x, y = a[c].to_numpy(zero_copy_only=False), b[c].to_numpy(zero_copy_only=False)
                if k == 1 and x.dtype.kind == "f":
                    # the large object of this batch selects 256-thread workgroups (and global scratch) for every object of
                    # the batch; alone, the ordinary positions run with one wave per object: the floating-point reductions
                    # (second moments, Haralick sums) then add in another order — last bits, not values
                    scale = float(np.nanmax(np.abs(y))) if y.size and np.isfinite(y).any() else 0.0  # (central moments cancel to ~0)
                    assert np.allclose(x, y, rtol=1e-9, atol=1e-12 + 1e-9 * scale, equal_nan=True), (k, i, c)
                else:
                    assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (k, i, c)
    assert any(g.num_rows == 0 for g in got)


def test_run_positions_from_other_threads_and_two_at_once(tmp_path, engine):
    """A caller that is not the main thread (its own context, aliby_amd/_lib.py), and two callers at once (the second waits:
    the calls of a process share segmenters, arenas and interpreter settings) — both get the tables single calls produce."""
    import threading

    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    fovs = [synth.make_fov(2, 80 + i, shape=(224, 256), n_channels=2, n_target=9) for i in range(6)]
    override = _keyed_override(fovs)

    def pipes(sel):
        made = []
        for i in sel:
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("sizeshape", "intensity"))
            p["steps"]["tile"]["image_kwargs"] = {"source": fovs[i]["pixels"][None]}
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            made.append(p)
        return made

    want = [run_pipeline_and_post(pipeline=p, pipeline_name=f"S{i}", output_path=tmp_path / "single")[0] for i, p in enumerate(pipes(range(6)))]
    got, errors = {}, []

    def call(tag, sel):
        try:
            got[tag] = run_positions(pipes(sel), [f"{tag}{i}" for i in sel], tmp_path / tag, batch_size=2)
        except Exception as e:  # noqa: BLE001
            errors.append((tag, repr(e)))

    def single(tag, sel):  # the reference's own entry point from a third thread, while the other two are at it
        try:
            got[tag] = [run_pipeline_and_post(pipeline=p, pipeline_name=f"{tag}{i}", output_path=tmp_path / tag) for i, p in zip(sel, pipes(sel))]
        except Exception as e:  # noqa: BLE001
            errors.append((tag, repr(e)))

    threads = [threading.Thread(target=call, args=("A", [0, 1, 2])), threading.Thread(target=call, args=("B", [3, 4, 5])),
               threading.Thread(target=single, args=("C", [1, 4]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors and set(got) == {"A", "B", "C"}, errors
    for tag, sel in (("A", [0, 1, 2]), ("B", [3, 4, 5]), ("C", [1, 4])):
        for res, i in zip(got[tag], sel):
            assert res[0].schema.equals(want[i].schema) and res[0].num_rows == want[i].num_rows > 0
            for c in want[i].column_names:  # (column by column: three normalised moments are NaN by definition)
                x, y = res[0][c].to_numpy(zero_copy_only=False), want[i][c].to_numpy(zero_copy_only=False)
                assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (tag, i, c)


def test_run_positions_with_positions_of_different_shapes_in_one_batch(tmp_path, engine):
    """Positions whose frames differ in size share a batch's segmentation where they can and fall back to the per-position engine
    for the steps that need one block: same tables as single calls."""
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post
    from aliby_amd.pipe_builder import build_pipeline_steps

    fovs = [synth.make_fov(2, 90, shape=(224, 256), n_channels=2, n_target=9), synth.make_fov(2, 91, shape=(192, 224), n_channels=2, n_target=7),
            synth.make_fov(2, 92, shape=(224, 256), n_channels=2, n_target=8), synth.make_fov(2, 93, shape=(160, 320), n_channels=2, n_target=6)]
    override = _keyed_override(fovs)

    def pipes():
        made = []
        for f in fovs:
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("sizeshape", "intensity"))
            p["steps"]["tile"]["image_kwargs"] = {"source": f["pixels"][None]}
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            made.append(p)
        return made

    names = [f"M{i}" for i in range(len(fovs))]
    want = [run_pipeline_and_post(pipeline=p, pipeline_name=nm, output_path=tmp_path / "single")[0] for p, nm in zip(pipes(), names)]
    from aliby_amd import runner

    stats = {}
    got = runner.run_positions(pipes(), names, tmp_path / "batched", batch_size=4, stats=stats)
    assert stats["batches"] == 3  # array sources say their shape: [M0, M2] share a batch, M1 and M3 run alone
    for i, (res, w) in enumerate(zip(got, want)):
        assert res[0].schema.equals(w.schema) and res[0].num_rows == w.num_rows > 0
        for c in w.column_names:
            x, y = res[0][c].to_numpy(zero_copy_only=False), w[c].to_numpy(zero_copy_only=False)
            assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (i, c)
    # sources that do not say their shape (TIFF files here) land in one batch: the segmenter then takes them one by one
    paths = []
    for i, f in enumerate(fovs[:2]):
        for c in range(2):
            synth.write_tiff(tmp_path / f"img__{i}__{c}.tif", f["pixels"][c, 0])
        paths.append([str(tmp_path / f"img__{i}__{c}.tif") for c in range(2)])

    def file_pipes():
        made = pipes()[:2]
        for p, pp in zip(made, paths):
            p["steps"]["tile"]["image_kwargs"] = {"source": {"key": Path(pp[0]).stem, "path": pp}, "regex": r".*img__([0-9])__([0-9])\.tif",
                                                  "capture_order": "FC"}
        return made

    got_f = runner.run_positions(file_pipes(), ["F0", "F1"], tmp_path / "files", batch_size=4, stats=stats)
    assert stats["batches"] == 1
    for i in range(2):
        for c in want[i].column_names:
            x, y = got_f[i][0][c].to_numpy(zero_copy_only=False), want[i][c].to_numpy(zero_copy_only=False)
            assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), ("files", i, c)


def test_run_positions_recovers_after_a_failing_position(tmp_path, engine):
    """A position whose image cannot be read fails the call with the reader's error; the next call of the process works (the
    device lock is free, the collector is back on, the arenas are usable)."""
    import gc

    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe_builder import build_pipeline_steps

    fovs = [synth.make_fov(2, 95 + i, shape=(224, 256), n_channels=2, n_target=8) for i in range(3)]
    override = _keyed_override(fovs)

    def pipes(bad=None):
        made = []
        for i, f in enumerate(fovs):
            p = build_pipeline_steps(channels_to_segment={"nuclei": 0}, channels_to_extract=[0, 1], features_to_extract=("sizeshape",))
            p["steps"]["tile"]["image_kwargs"] = ({"source": str(tmp_path / "missing.tif"), "capture_order": "CYX"} if i == bad
                                                  else {"source": f["pixels"][None]})
            p["steps"]["segment_nuclei"]["segmenter_kwargs"]["setup_params"] = dict(flows_override=override)
            made.append(p)
        return made

    names = ["E0", "E1", "E2"]
    with pytest.raises(Exception) as err:
        run_positions(pipes(bad=1), names, tmp_path / "bad", batch_size=2)
    assert "missing.tif" in str(err.value), err.value
    assert gc.isenabled() and gc.get_freeze_count() == 0
    got = run_positions(pipes(), names, tmp_path / "good", batch_size=2)
    assert [g[0].num_rows > 0 for g in got] == [True, True, True]


def test_run_positions_monotile_timelapse_matches_single_calls(tmp_path, engine):
    """Positions with three time points (Z = 3, one channel, monotile, masks saved every time point, history trimmed by `retain`)
    through the position-batched runner against one run_pipeline_and_post per position: tables, metadata_tp, saved masks."""
    from aliby_amd.parallel import run_positions
    from aliby_amd.pipe import run_pipeline_and_post

    T, P = 3, 3
    stacks, keyed = [], []
    for p in range(P):
        fovs = [synth.make_fov(4, 10 * p + t, shape=(160, 192), n_channels=1, n_z=3, n_target=6 + t + p) for t in range(T)]
        stacks.append(np.stack([f["pixels"] for f in fovs]))  # [T,1,3,Y,X]
        keyed += [dict(pixels=f["pixels"], nuclei=f["nuclei"]) for f in fovs]
    override = _keyed_override(keyed)  # (keyed by the projected plane: any order of calls, any batch)
    tree = {"None": {"None": ["sizeshape"]}, 0: {"max": ["intensity"]}}

    def pipes():
        return [{
            "ntps": T,
            "steps": {
                "tile": {"image_kwargs": {"source": stacks[p]}, "tile_size": None},
                "segment_cells": {"segmenter_kwargs": {"kind": "cellpose", "setup_params": {"flows_override": override}}, "channel_to_segment": 0},
                "extract_cells": {"tree": tree},
            },
            "passed_data": {"extract_cells": [("masks", "segment_cells"), ("pixels", "tile")]},
            "passed_methods": {"segment_cells": ("tile", "get_fczyx")},
            "save": ("segment_cells",), "save_interval": 1, "retain": {"tile": 1},
        } for p in range(P)]

    names = [f"T{p}" for p in range(P)]
    want = [run_pipeline_and_post(pipeline=pl, pipeline_name=nm, output_path=tmp_path / "single")[0] for pl, nm in zip(pipes(), names)]
    got = run_positions(pipes(), names, tmp_path / "batched", batch_size=2)
    for p, (res, w) in enumerate(zip(got, want)):
        assert res[0].schema.equals(w.schema) and res[0].num_rows == w.num_rows > 0
        assert sorted(set(res[0]["metadata_tp"].to_pylist())) == list(range(T))
        for c in w.column_names:
            x, y = res[0][c].to_numpy(zero_copy_only=False), w[c].to_numpy(zero_copy_only=False)
            assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), (p, c)
        for t in range(T):
            a = np.load(tmp_path / "batched" / "steps" / names[p] / "segment_cells" / f"{t:04d}.npz")["arr_0"]
            b = np.load(tmp_path / "single" / "steps" / names[p] / "segment_cells" / f"{t:04d}.npz")["arr_0"]
            assert np.array_equal(a, b), (p, t)
