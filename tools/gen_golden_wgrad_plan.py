"""Fixture for the weight-gradient planners (tests/golden/wgrad_plan.json): what rehr_wgrad_workspace_bytes,
rehr_wgrad_uses_winograd and rehr_wgrad_bf16_workspace_bytes return for every row of tests/wgrad_plan_cases.py.  The
three are pure host code, so this runs without a device.

The file pins the plans (route, tiles, splits: together they fix the workspace size) that the library had BEFORE the
host code of the weight-gradient family was merged into shared helpers.  It is a record of that library, not of the
current one: regenerate it only against a build of the commit whose plans are meant to be kept, and only to add rows.

    REHRSEG_HIP_LIB=/path/to/that/librehrseg_hip.so python tools/gen_golden_wgrad_plan.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rehrseg_amd import lib as L  # noqa: E402
from wgrad_plan_cases import ROWS, desc  # noqa: E402


def main():
    lib = L.load()
    rec = {}
    for name, args in ROWS:
        d = desc(**args)
        rec[name] = {"f32_bytes": int(lib.rehr_wgrad_workspace_bytes(C.byref(d))),
                     "uses_winograd": int(lib.rehr_wgrad_uses_winograd(C.byref(d))),
                     "bf16_bytes": int(lib.rehr_wgrad_bf16_workspace_bytes(C.byref(d)))}
    assert len(rec) == len(ROWS), "row names must be unique"
    path = os.path.join(ROOT, "tests", "golden", "wgrad_plan.json")
    with open(path, "w") as f:
        json.dump({"rows": rec}, f, indent=1)
        f.write("\n")
    print("wrote", path, len(rec), "rows from", L.LIB_PATH)


if __name__ == "__main__":
    main()
