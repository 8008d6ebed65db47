"""bench.py --dump-outputs: what the last timed step computed lands as float32 / float64 .npy files within the size cap, and
the same outputs give the same files (a larger output is sampled with a fixed seed).  A feature column that is NaN for every
object (undefined by definition) is left out and the kept column indices are written beside the rows."""

import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def _fake(n_fov, n_obj, c1, c2, side):
    rng = np.random.default_rng(7)
    host = np.zeros(n_obj, dtype=[("tile", "<i4"), ("label", "<i4")])
    host["tile"] = np.sort(rng.integers(0, n_fov, n_obj))
    host["label"] = np.arange(n_obj) % 250 + 1
    table = SimpleNamespace(n_obj=n_obj, host=host)
    rows = (rng.standard_normal((n_obj, c1)), rng.standard_normal((n_obj, c2)))
    rows[0][:, 1] = np.nan  # NaN for every object, like the normalised moments of order < 2
    labels = torch.from_numpy(rng.integers(0, 300, (n_fov, side, side)).astype(np.int32))
    return rows, table, labels


def _load(d):
    return {p.stem: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_small_output_is_written_whole(tmp_path):
    rows, table, labels = _fake(3, 40, 5, 2, 32)
    info = bench.dump_outputs(tmp_path, rows, table, labels)
    got = _load(tmp_path)
    assert info["rows_written"] == 40 and info["mask_fovs"] == [0, 1, 2]
    assert info["all_nan_columns_left_out"] == {"features_mono": [1], "features_multi": []}
    np.testing.assert_array_equal(got["features_mono_columns"], [0, 2, 3, 4])
    np.testing.assert_array_equal(got["features_mono"], rows[0][:, [0, 2, 3, 4]])
    np.testing.assert_array_equal(got["features_multi_columns"], [0, 1])
    np.testing.assert_array_equal(got["features_multi"], rows[1])
    np.testing.assert_array_equal(got["masks"], labels.numpy().astype(np.float32))
    np.testing.assert_array_equal(got["object_label"], table.host["label"])
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert all(np.isfinite(a).all() for a in got.values())


def test_a_nan_of_one_object_is_kept(tmp_path):
    rows, table, labels = _fake(2, 30, 4, 2, 16)
    rows[0][7, 2] = np.nan  # undefined for this object only: written as it is
    bench.dump_outputs(tmp_path, rows, table, labels)
    got = _load(tmp_path)
    np.testing.assert_array_equal(got["features_mono_columns"], [0, 2, 3])
    np.testing.assert_array_equal(got["features_mono"], rows[0][:, [0, 2, 3]])
    assert np.isnan(got["features_mono"][7, 1]) and np.isnan(got["features_mono"]).sum() == 1


def test_large_output_is_a_fixed_sample_within_the_cap(tmp_path):
    rows, table, labels = _fake(16, 20000, 420, 40, 512)  # ~74 MB of rows + 16 MB of planes
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(a, rows, table, labels)
    bench.dump_outputs(b, rows, table, labels)
    ga, gb = _load(a), _load(b)
    assert sum(p.stat().st_size for p in a.glob("*.npy")) <= bench.DUMP_BYTES
    assert ga.keys() == gb.keys()
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k])
    idx = ga["row_index"].astype(np.int64)
    assert 0 < len(idx) < 20000 and np.all(np.diff(idx) > 0)
    cols = ga["features_mono_columns"].astype(np.int64)
    assert 1 not in cols and len(cols) == 419
    np.testing.assert_array_equal(ga["features_mono"], rows[0][idx][:, cols])
    assert all(np.isfinite(x).all() for x in ga.values())
    np.testing.assert_array_equal(ga["object_tile"], table.host["tile"][idx])
    fovs = ga["mask_fov"].astype(np.int64)
    assert len(fovs) == bench.DUMP_MASK_FOVS
    np.testing.assert_array_equal(ga["masks"], labels.numpy()[fovs].astype(np.float32))
