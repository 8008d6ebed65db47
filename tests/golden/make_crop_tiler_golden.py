"""
Generates tests/golden/reference_crop_tiler.npz: what the reference's own CropTiler (src/aliby/tile/tiler.py) returns from
get_fczyx(0) on the seeded scenes of tests/crop_tiler_ref.py (scenes()), over the eight on/off combinations of clip_outliers,
convert_8bit and standard_scale.  Needs a checkout of the reference:

    python tests/golden/make_crop_tiler_golden.py --reference <reference checkout>

tiler.py is loaded on its own with importlib.  Of its imports only NumPy is used by CropTiler; for those that are not installed
(dask.array, skimage.registration, agora.abc, aliby.tile.process_traps, aliby.tile.tiles) an empty stand-in module is placed in
sys.modules first, whose attributes are empty classes.  Only numbers travel: one array per "<scene>/<combination>"; the inputs
are rebuilt from their seeds.
"""
import argparse
import importlib
import importlib.util
import sys
import types
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]


class _Any(type):
    """An empty class whose every attribute is another one: good as a base class and inside an annotation."""

    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any(name, (), {})


class _StandIn(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Any(name, (), {})


def load_reference(checkout: Path):
    for name in ("dask", "dask.array", "skimage", "skimage.registration", "agora", "agora.abc", "aliby", "aliby.tile",
                 "aliby.tile.process_traps", "aliby.tile.tiles"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _StandIn(name)
    spec = importlib.util.spec_from_file_location("reference_tiler", checkout / "src" / "aliby" / "tile" / "tiler.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=Path, required=True)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from tests import crop_tiler_ref as cr

    ref = load_reference(args.reference)
    out = {}
    for name, s in cr.scenes().items():
        for clip, bit8, std in cr.COMBOS:
            tiler = ref.CropTiler(s["pixels"][None], s["ts"], standard_scale=std, convert_8bit=bit8, clip_outliers=clip)
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")  # the constant channel: 0 / 0, and NaN cast to uint8
                tiles = tiler.get_fczyx(0)
            out[f"{name}/{cr.combo_name(clip, bit8, std)}"] = tiles
            print(name, cr.combo_name(clip, bit8, std), tiles.shape, tiles.dtype)
    np.savez_compressed(HERE / "reference_crop_tiler.npz", **out)
    print((HERE / "reference_crop_tiler.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
