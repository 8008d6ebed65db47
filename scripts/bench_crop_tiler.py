"""
Times the crop tiler's three kernels (aliby_amd/csrc/tile_crop.hip) with device events on one 5 x 1 x 2160 x 2160 uint16 frame,
tile size 224, clip_outliers + standard_scale: histogram, statistics, tile pass (float32 and float64) and the whole call, once on
random pixels and once on a narrow-range frame (values within 2 000 grey levels: the contended case of the histogram).  Beside
them the same work in NumPy on the host: the reference's arithmetic per voxel (np.percentile, np.mean, np.std) and
tests/crop_tiler_ref.py (through the histogram).  Prints one JSON line per frame.

    python scripts/bench_crop_tiler.py [--reps 50] [--windows 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def numpy_per_voxel(pix, ts):
    """clip_outliers -> standard_scale -> tiles, per voxel, as the reference computes them"""
    axes = (-3, -2, -1)
    pmax, pmin = np.percentile(pix, 99.5, axis=axes), np.percentile(pix, 0.5, axis=axes)
    x = np.clip((pix.T - pmin) / (pmax - pmin), 0, 1).T
    x = ((x.T - np.mean(x, axis=axes)) / np.std(x, axis=axes)).T
    C, Z, Y, X = x.shape
    return np.stack([x[:, :, i:i + ts, j:j + ts] for i in range(0, Y - ts + 1, ts) for j in range(0, X - ts + 1, ts)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    import torch

    from aliby_amd import _lib
    from aliby_amd.extraction.engine import FeatureEngine, _ptr, _stream_ptr
    from tests import crop_tiler_ref as cr

    assert torch.cuda.is_available(), "needs the GPU: there is no fallback to time"
    eng = FeatureEngine(0)
    lib, ctx = eng.lib, eng.ctx.handle
    C, Z, Y, X, ts, flags = 5, 1, 2160, 2160, 224, _lib.CROP_CLIP | _lib.CROP_STD
    n, T = Z * Y * X, (Y // ts) * (X // ts)
    rng = np.random.default_rng(5)
    frames = {"random": rng.integers(0, 65536, (C, Z, Y, X)).astype(np.uint16),
              "narrow": (1000 + rng.integers(0, 2000, (C, Z, Y, X))).astype(np.uint16)}
    for name, px in frames.items():
        dev = torch.from_numpy(px).cuda()
        hist = torch.empty((C, 65536), dtype=torch.int32, device="cuda")
        stats = torch.empty((C, 4), dtype=torch.float64, device="cuda")
        out32 = torch.empty((T, C, Z, ts, ts), dtype=torch.float32, device="cuda")
        out64 = torch.empty((T, C, Z, ts, ts), dtype=torch.float64, device="cuda")
        s = _stream_ptr()
        calls = {
            "histogram": lambda: lib.aliby_crop_hist_u16(ctx, _ptr(dev), C, n, _ptr(hist), s),
            "statistics": lambda: lib.aliby_crop_stats(ctx, _ptr(hist), C, n, flags, 0.5, _ptr(stats), s),
            "tiles_f32": lambda: lib.aliby_crop_cut_u16(ctx, _ptr(dev), C, Z, Y, X, ts, flags, _ptr(stats), _ptr(out32), _lib.F32, s),
            "tiles_f64": lambda: lib.aliby_crop_cut_u16(ctx, _ptr(dev), C, Z, Y, X, ts, flags, _ptr(stats), _ptr(out64), _lib.F64, s),
            "whole_call_f32": lambda: lib.aliby_crop_tiles_u16(ctx, _ptr(dev), C, Z, Y, X, ts, flags, 0.5, _ptr(out32), _lib.F32,
                                                               _ptr(stats), s),
        }
        result = {"frame": name, "shape": [C, Z, Y, X], "tile_size": ts, "reps": args.reps}
        for what, call in calls.items():
            for _ in range(3):
                _lib.check(call())
            torch.cuda.synchronize()
            per_call = []
            for _ in range(args.windows):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    call()
                b.record()
                torch.cuda.synchronize()
                per_call.append(a.elapsed_time(b) * 1e3 / args.reps)
            result[what + "_us"] = {"median": round(float(np.median(per_call)), 2), "min": round(min(per_call), 2),
                                    "max": round(max(per_call), 2)}
        # the same numbers as the restatement's, at the size timed
        t0 = time.perf_counter()
        frame, want_stats = cr.normalise(px, True, False, True)
        want = cr.cut(frame, ts)
        result["numpy_restatement_s"] = round(time.perf_counter() - t0, 3)
        got = out64.cpu().numpy()
        result["rel_err_tiles_f64"] = cr.rel_err(got, want)
        result["rel_err_stats"] = cr.rel_err(stats.cpu().numpy(), want_stats)
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), np.stack([cr.histogram(px[c]) for c in range(C)]))
        assert np.array_equal(out32.cpu().numpy(), got.astype(np.float32))
        t0 = time.perf_counter()
        per_voxel = numpy_per_voxel(px, ts)
        result["numpy_per_voxel_s"] = round(time.perf_counter() - t0, 3)
        result["rel_err_restatement_vs_per_voxel"] = cr.rel_err(want, per_voxel)
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
