"""Fixture for the host side of the pipeline kernels (tests/golden/pipeline_host.json): what the five workspace size
queries and the 23 launch entry points of seg_eval, sr_volume, stage1_volume, sr_metrics, seg_surface, seg_components,
intensity_norm and sr_losses return for every row of tests/pipeline_host_cases.py.  Runs only on a machine without a
device: an accepted call then returns REHR_EHIP, so nothing is launched on the table's dummy pointers.

The file pins the argument checks, their order and the workspace sizes that the library had BEFORE the host code of
these files moved onto csrc/host_util.h.  It is a record of that library, not of the current one: regenerate it only
against a build of the commit whose behaviour is meant to be kept, and only to add rows.

    REHRSEG_HIP_LIB=/path/to/that/librehrseg_hip.so python tools/gen_golden_pipeline_host.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rehrseg_amd import lib as L  # noqa: E402
import pipeline_host_cases as T  # noqa: E402


def main():
    import torch
    if torch.cuda.is_available():
        sys.exit("a device is present: the launch rows would run kernels on dummy pointers")
    rec = T.record(L.load(), launches=True)
    bad = T.table_condition(rec["launches"])
    if bad:
        sys.exit("the table does not meet its condition on this library:\n  " + "\n  ".join(bad))
    path = os.path.join(ROOT, "tests", "golden", "pipeline_host.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path, len(rec["queries"]), "queries and", len(rec["launches"]), "launch rows from", L.LIB_PATH)


if __name__ == "__main__":
    main()
