"""Fixture for the host side of the thin-convolution family (tests/golden/thin_plan.json): for every row of
tests/thin_plan_cases.py what the seven size and route queries return, and the return code of the fourteen launch entry
points (as given, with a short and a null workspace, with each required pointer null).  Run it on a machine WITHOUT a
device: the descriptors carry dummy pointers, and an accepted one must come back REHR_EHIP instead of being launched.

The file pins what the library did BEFORE the host code of the family was merged into direct_shared.h.  It is a record
of that library, not of the current one: regenerate it only against a build of the commit whose behaviour is meant to
be kept, and only to add rows.

    REHRSEG_HIP_LIB=/path/to/that/librehrseg_hip.so python tools/gen_golden_thin_plan.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rehrseg_amd import lib as L  # noqa: E402
from thin_plan_cases import ROWS, launch_codes, queries  # noqa: E402


def main():
    import torch
    assert not torch.cuda.is_available(), "dummy pointers: record the launch codes where nothing can be launched"
    lib = L.load()
    rec = {name: {"queries": queries(lib, args), "launch": launch_codes(lib, args)} for name, args in ROWS}
    assert len(rec) == len(ROWS), "row names must be unique"
    path = os.path.join(ROOT, "tests", "golden", "thin_plan.json")
    with open(path, "w") as f:   # one line per row
        f.write('{"rows": {\n')
        f.write(",\n".join(f" {json.dumps(name)}: {json.dumps(r)}" for name, r in rec.items()))
        f.write("\n}}\n")
    print("wrote", path, len(rec), "rows from", L.LIB_PATH)


if __name__ == "__main__":
    main()
