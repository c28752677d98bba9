"""The host side of the pipeline kernels is pinned without a device: the five workspace size queries and, for the 23
launch entry points of seg_eval, sr_volume, stage1_volume, sr_metrics, seg_surface, seg_components, intensity_norm and
sr_losses, which calls are accepted and which code a refused one gets -- so also the order of the checks.
tests/golden/pipeline_host.json holds what the library answered before its host code moved onto csrc/host_util.h."""
import json
import os

import pytest

from rehrseg_amd import lib as L
import pipeline_host_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_host.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_reaches_every_entry_point_and_error_code(golden):
    """The recorded values themselves show that the table is not one-sided: every launch entry point has a row that
    was accepted (REHR_EHIP: no device) and one that was REHR_EINVAL, every one that documents an extent limit a
    REHR_ENOSUP, and there are at least 150 rows."""
    assert T.table_condition(golden["launches"]) == []
    q = golden["queries"]
    assert set(q) == {T.query_name(e, a) for e, a in T.QUERIES}
    for entry in {e for e, _ in T.QUERIES}:
        codes = [v for k, v in q.items() if k.startswith(entry + "(")]
        assert T.EINVAL in codes or entry == "rehr_seg_cc_workspace_bytes", entry   # that one answers ENOSUP alone
        assert T.ENOSUP in codes and sum(c > 0 for c in codes) >= 6, entry


def test_recorded_sizes_follow_the_documented_layouts(golden):
    """The fixture against the layouts of include/rehrseg_hip.h, at the sizes whose segments need padding."""
    q = golden["queries"]
    assert q["rehr_seg_surface_workspace_bytes(3, 5, 7)"] == T.surface_bytes(105) == 4096 + 2 * 848 + 112
    assert q["rehr_seg_cc_workspace_bytes(3, 5, 7)"] == T.cc_bytes(105) == 64 + 4 * 432
    assert q["rehr_order_stats_workspace_bytes(3, 3)"] == T.order_bytes(3, 3) == 144 + 16 + 9216
    assert q["rehr_sr_metrics_workspace_bytes(2, 3, 12, 13)"] == T.tile_bytes(6, 6)
    assert q["rehr_structure_loss_workspace_bytes(2, 2, 3, 12, 13)"] == T.tile_bytes(12, 4)


def test_size_queries_equal_the_record(golden):
    got = T.record(L.load(), launches=False)["queries"]
    assert got == golden["queries"], {k: (v, golden["queries"][k]) for k, v in got.items() if v != golden["queries"][k]}


def test_launch_checks_equal_the_record(golden):
    """Runs only where there is no device: an accepted call then meets "no device", not a launch on dummy pointers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted call cannot be launched")
    got = T.record(L.load(), launches=True)["launches"]
    want = golden["launches"]
    assert got == want, {k: (v, want[k]) for k, v in got.items() if v != want[k]}
