"""
Generates tests/golden/reference_nuc_conv_3d.json: what the reference's own nuc_conv_3d
(src/extraction/core/functions/custom/localisation.py) returns on the seeded inputs of tests/localisation3d_ref.py (scenes()).
Needs a checkout of the reference:

    python tests/golden/make_localisation3d_golden.py --reference <reference checkout>

The module imports scikit-image, which it uses in small_peaks_conv only; where scikit-image is not installed an empty stand-in
module of that name is placed in sys.modules first.  Only numbers travel: {scene: [value per (tile, label) row]}, NaN written as
the string "nan"; the inputs are rebuilt from their seeds.
"""
import argparse
import importlib.util
import json
import sys
import types
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]


def load_reference(checkout: Path):
    try:
        import skimage  # noqa: F401
    except ImportError:
        sys.modules["skimage"] = types.ModuleType("skimage")
    path = checkout / "src" / "extraction" / "core" / "functions" / "custom" / "localisation.py"
    spec = importlib.util.spec_from_file_location("reference_localisation", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=Path, required=True)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from tests import localisation3d_ref as lr

    ref = load_reference(args.reference)
    out = {}
    for name, s in lr.scenes().items():
        vals = []
        for f, l in lr.rows(s):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")  # the empty mask: "Mean of empty slice"
                v = float(ref.nuc_conv_3d(s["labels"][f] == l, np.array(s["stack"][f, s["channel"]]), **s["kwargs"]))
            vals.append(v if np.isfinite(v) else repr(v))
        out[name] = vals
        print(name, len(vals))
    (HERE / "reference_nuc_conv_3d.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
