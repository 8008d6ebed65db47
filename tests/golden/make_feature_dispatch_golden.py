"""
Writes tests/golden/feature_dispatch_trace.json: what `families.evaluate` decides for every case of tests/dispatch_recorder.py,
recorded through its recording engine (no GPU).  The committed file was written at the commit BEFORE `evaluate` was split into
`plan` and its executors, so tests/test_cpu_feature_dispatch.py holds the split to the dispatch it replaced.  Rewrite it only when a
change is meant to alter which launches happen, and say so in that commit.

    python tests/golden/make_feature_dispatch_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import dispatch_recorder as dr  # noqa: E402


def main():
    undo = []

    def setattr_(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    trace = {name: dr.run_case(case, setattr_) for name, case in dr.cases().items()}
    for obj, name, value in reversed(undo):
        setattr(obj, name, value)
    out = Path(__file__).with_name("feature_dispatch_trace.json")
    lines = [f"{json.dumps(name)}: {json.dumps(t, separators=(',', ':'), sort_keys=True)}" for name, t in trace.items()]
    out.write_text("{\n" + ",\n".join(lines) + "\n}\n")  # one case per line
    n_ok = sum("raises" not in t for t in trace.values())
    print(f"{out.name}: {len(trace)} cases ({n_ok} complete, {len(trace) - n_ok} refused), {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
