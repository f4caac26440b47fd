#!/usr/bin/env python3
"""tests/golden/parity_bounds.json from a parity log of the GPU tests.

  EKF_PARITY_LOG=gpurun_out/parity_log.jsonl python -m pytest tests -m gpu      (on the MI355X box)
  python tools/update_parity_bounds.py gpurun_out/parity_log.jsonl              (here)
  python tools/update_parity_bounds.py --add LOG     (the log of new tests alone: adds their sites, moves no recorded one)

Per call site of tests/helpers.bound() (test node id + label) the MAXIMUM error measured in that run is recorded;
bound() then holds the site to 10x that value (see its docstring).  The log itself is kept under profiles/ so the
numbers can be audited."""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    add = "--add" in sys.argv[1:]
    sys.argv = [a for a in sys.argv if a != "--add"]
    log = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gpurun_out", "parity_log.jsonl")
    path = os.path.join(ROOT, "tests", "golden", "parity_bounds.json")
    measured = collections.OrderedDict()
    for line in open(log):
        r = json.loads(line)
        measured[r["site"]] = max(measured.get(r["site"], 0.0), r["value"])
    if add:
        # the log of a run of new tests only: their sites join the file, every recorded site keeps its value
        out = json.load(open(path), object_pairs_hook=collections.OrderedDict)
        new = [k for k in measured if k not in out["sites"]]
        for k in new:
            out["sites"][k] = measured[k]
        json.dump(out, open(path, "w"), indent=1)
        print(f"{len(new)} new call sites ({len(measured) - len(new)} already recorded, left alone) -> {path}")
        return
    out = {"generated_by": "tools/update_parity_bounds.py", "source_log": os.path.relpath(log, ROOT),
           "rule": "bound = min(ceiling in the test, max(10 x measured, floor)), floor 3e-7 (fp32 sites) / 1e-14 (fp64 sites)",
           "sites": measured}
    json.dump(out, open(path, "w"), indent=1)
    print(f"{len(measured)} call sites -> {path}")


if __name__ == "__main__":
    main()
