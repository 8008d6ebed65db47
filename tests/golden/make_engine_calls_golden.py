"""
Writes tests/golden/engine_call_trace.json: what `FeatureEngine` hands to the C library for every case of
tests/engine_call_recorder.py, recorded through its stand-in library (no GPU).  The committed file was written at the commit
BEFORE the engine's launches were put on one path, so tests/test_cpu_engine_calls.py holds that path, and the shared argument
checks, to the calls they replaced.  Rewrite it only when a change is meant to alter what reaches C, and say so in that commit.

    python tests/golden/make_engine_calls_golden.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import engine_call_recorder as er  # noqa: E402


def main():
    undo = []

    def setattr_(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    trace = {name: er.run_case(fn, setattr_) for name, fn in er.cases().items()}
    for obj, name, value in reversed(undo):
        setattr(obj, name, value)
    out = Path(__file__).with_name("engine_call_trace.json")
    lines = [f"{json.dumps(name)}: {json.dumps(t, separators=(',', ':'), sort_keys=True)}" for name, t in trace.items()]
    out.write_text("{\n" + ",\n".join(lines) + "\n}\n")  # one case per line
    n_ok = sum("raises" not in t for t in trace.values())
    n_calls = sum(1 for t in trace.values() for name, _ in t["events"] if name.startswith("aliby_"))
    print(f"{out.name}: {len(trace)} cases ({n_ok} complete, {len(trace) - n_ok} refused), {n_calls} C calls, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
