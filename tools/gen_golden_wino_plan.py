"""Fixture for the host side of the fp32 Winograd forward / input-gradient family (tests/golden/wino_plan.json): for every
row of tests/wino_plan_cases.py what rehr_gather_gemm_wino_bytes returns under each debug-flag setting, and the return
code of rehr_gather_gemm_f32 / rehr_gather_gemm_multi_f32 (plain and with REHR_GG_WS_ONLY) with the queried scratch, with
one byte less, with a null and with a misaligned scratch; for the multi-part rows the same with every part's scratch sized by the formula
(parts that have no route of their own are what tells the all-or-none entries from the per-part loop).
Run it on a machine WITHOUT a device: the descriptors carry dummy pointers, and a launch must come back REHR_EHIP.

The file pins what the library did BEFORE the family's host code was merged into wino_shared.h and the route decided in
one place.  It is a record of that library, not of the current one: regenerate it only against a build of the commit whose
behaviour is meant to be kept, and only to add rows.  (Only the three recorded entry points are bound, so a library of an
older ABI version loads.)

    REHRSEG_HIP_LIB=/path/to/that/librehrseg_hip.so python tools/gen_golden_wino_plan.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from wino_plan_cases import MULTI, ROWS, bind, bytes_by_flag, launch_codes, multi_codes  # noqa: E402


def main():
    import torch
    assert not torch.cuda.is_available(), "dummy pointers: record the launch codes where nothing can be launched"
    path = os.environ.get("REHRSEG_HIP_LIB")
    lib = bind(path)
    rows = {name: {"bytes": bytes_by_flag(lib, args), "launch": launch_codes(lib, args)} for name, args, _, _ in ROWS}
    multi = {name: multi_codes(lib, parts) for name, parts, _ in MULTI}
    assert len(rows) == len(ROWS) and len(multi) == len(MULTI), "row names must be unique"
    out = os.path.join(ROOT, "tests", "golden", "wino_plan.json")
    with open(out, "w") as f:   # one line per row
        f.write('{"rows": {\n')
        f.write(",\n".join(f" {json.dumps(name)}: {json.dumps(r)}" for name, r in rows.items()))
        f.write('\n},\n"multi": {\n')
        f.write(",\n".join(f" {json.dumps(name)}: {json.dumps(r)}" for name, r in multi.items()))
        f.write("\n}}\n")
    print("wrote", out, len(rows), "+", len(multi), "rows from", path or "the in-tree library")


if __name__ == "__main__":
    main()
