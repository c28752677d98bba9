"""Fixture for the host side of the direct gather-GEMM kernels (tests/golden/direct_plan.json): for every row of
tests/direct_plan_cases.py the return codes of rehr_gather_gemm_f32 / rehr_gather_gemm_multi_f32 / rehr_gather_gemm_bf16 /
rehr_gather_gemm_multi_bf16 under debug_flags 0, REHR_DBG_GG_NO_HALO and REHR_DBG_GG_NO_TCONV_KS, and for every multi-part
row those of the two multi entry points.
Run it on a machine WITHOUT a device: the descriptors carry dummy pointers, and a launch must come back REHR_EHIP.

The file pins what the library did BEFORE the host code of the halo kernels and tconv_ks was merged into halo_shared.h
and the route decided in one place.  It is a record of that library, not of the current one: regenerate it only against
a build of the commit whose behaviour is meant to be kept, and only to add rows.  (Only the four recorded entry points
are bound, so a library of an older ABI version loads.)

    REHRSEG_HIP_LIB=/path/to/that/librehrseg_hip.so python tools/gen_golden_direct_plan.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from direct_plan_cases import MULTI, ROWS, bind, multi_codes, row_codes  # noqa: E402


def main():
    import torch
    assert not torch.cuda.is_available(), "dummy pointers: record the launch codes where nothing can be launched"
    path = os.environ.get("REHRSEG_HIP_LIB")
    lib = bind(path)
    rows = {r[0]: row_codes(lib, r[1]) for r in ROWS}
    multi = {m[0]: multi_codes(lib, m[1]) for m in MULTI}
    assert len(rows) == len(ROWS) and len(multi) == len(MULTI), "row names must be unique"
    out = os.path.join(ROOT, "tests", "golden", "direct_plan.json")
    with open(out, "w") as f:   # one line per row
        f.write('{"rows": {\n')
        f.write(",\n".join(f" {json.dumps(name)}: {json.dumps(r)}" for name, r in rows.items()))
        f.write('\n},\n"multi": {\n')
        f.write(",\n".join(f" {json.dumps(name)}: {json.dumps(r)}" for name, r in multi.items()))
        f.write("\n}}\n")
    print("wrote", out, len(rows), "+", len(multi), "rows from", path or "the in-tree library")


if __name__ == "__main__":
    main()
