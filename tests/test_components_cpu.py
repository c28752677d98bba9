"""Connected components and lesion-wise scores without a GPU: the public functions over the CPU statement of the
kernels (tests/components_emu.py) against the scipy oracle (tests/components_oracle.py), the dict's NaN / 0.0
conventions, the tuple layout of _evaluate_case for the four surface x components combinations, the printed lines of
evaluate_cases(components=True), and the four new C-ABI symbols with their argument checks."""
import math

import numpy as np
import pytest
import torch

import components_oracle as co
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import seg_utils as su
from test_eval_cpu import G

NEW_SYMBOLS = ("rehr_seg_cc_workspace_bytes", "rehr_seg_cc_roots_i32", "rehr_seg_cc_lesion_i64",
               "rehr_seg_cc_compact_i32")
EINVAL, ENOSUP = -1, -2
KEYS = {"n_pred", "n_gt", "tp_pred", "tp_gt", "fp", "fn", "largest_pred", "largest_gt", "precision", "recall", "f1",
        "dice_largest", "dice_largest_terms"}
CPU_CASES = ("noise_0.1", "noise_0.3", "checkerboard", "corners", "edges", "no_wrap", "late_join_mirror", "empty",
             "one_row", "one_column", "lesions_pred")


@pytest.fixture
def components_emu():
    import components_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


@pytest.mark.parametrize("connectivity", co.CONNECTIVITIES)
@pytest.mark.parametrize("name", CPU_CASES)
def test_public_functions_meet_the_oracle(components_emu, name, connectivity):
    m, g, want = co.case(name), co.partner(name), co.expected(name, connectivity)
    labels, n = su.connected_components(m, connectivity, device="cpu")
    assert labels.dtype == torch.int32 and tuple(labels.shape) == m.shape and type(n) is int
    assert n == want["n"] and np.array_equal(labels.numpy(), want["labels"])
    keep = su.keep_largest_component(m, connectivity, device="cpu")
    assert keep.dtype == torch.uint8 and np.array_equal(keep.numpy(), want["keep"])
    got = su.lesion_metrics(m, g, connectivity, device="cpu")
    assert co.same_dict(got, want["dict"]), (got, want["dict"])


def test_oracle_counts_of_the_cases():
    """What the issue states about the cases, from scipy alone."""
    assert [co.expected("checkerboard", c)["n"] for c in co.CONNECTIVITIES] == [120, 1, 1]
    assert [co.expected("corners", c)["n"] for c in co.CONNECTIVITIES] == [2, 2, 1]
    assert [co.expected("edges", c)["n"] for c in co.CONNECTIVITIES] == [2, 1, 1]
    assert [co.expected("no_wrap", c)["n"] for c in co.CONNECTIVITIES] == [4, 4, 4]
    assert co.expected("noise_0.1", 6)["n"] == 571 and co.n_largest_ties(co.case("noise_0.1"), 6) == 3
    assert co.expected("noise_0.1", 6)["eight"][4] == 7
    assert co.expected("snake", 6)["n"] == 1 and co.case("snake").sum() > 5 * 9 * 67 // 4
    for name in ("late_join", "late_join_mirror"):
        m = co.case(name).copy()
        assert [co.expected(name, c)["n"] for c in co.CONNECTIVITIES] == [1, 1, 1]
        m[0 if name == "late_join_mirror" else -1, 0 if name == "late_join_mirror" else -1, 1::2] = False
        assert co.labels(m, 26)[1] == 34
    d = co.expected("lesions_pred", 26)["dict"]
    assert d["n_gt"] >= 5 and 0 < d["tp_gt"] < d["n_gt"] and d["fp"] >= 1 and d["tp_pred"] != d["tp_gt"]
    # the largest predicted component is not the one with the most ground-truth overlap
    P, Gt = co.case("lesions_pred"), co.case("lesions_gt")
    lab, n = co.labels(P, 26)
    overlap = [int(((lab == k) & Gt).sum()) for k in range(1, n + 1)]
    assert d["dice_largest_terms"][0] < max(overlap)


def test_labels_follow_the_roots_not_scipy():
    m = co.case("noise_0.3")
    for c in co.CONNECTIVITIES:
        r, (lab, n) = co.roots(m, c), co.labels(m, c)
        uniq = np.unique(r[r >= 0])
        assert n == len(uniq) and np.array_equal(lab[r >= 0], np.searchsorted(uniq, r[r >= 0]) + 1)
        assert (lab[r < 0] == 0).all() and (r.ravel()[uniq] == uniq).all()
        assert (r[m] <= np.flatnonzero(m.ravel())).all()


def test_dict_conventions(components_emu):
    z = np.zeros((3, 6, 7), np.uint8)
    a, b = z.copy(), z.copy()
    a[0, 1:3, 1:3] = 1
    b[2, 4:6, 4:7] = 1
    d = su.lesion_metrics(z, b, device="cpu")                  # empty prediction
    assert (d["n_pred"], d["n_gt"], d["tp_gt"], d["fn"]) == (0, 1, 0, 1)
    assert math.isnan(d["precision"]) and d["recall"] == 0.0 and math.isnan(d["f1"])
    assert d["largest_pred"] == 0 and d["dice_largest_terms"] == (0, 0, 6)
    d = su.lesion_metrics(a, z, device="cpu")                  # empty label
    assert (d["n_pred"], d["n_gt"], d["fp"]) == (1, 0, 1)
    assert d["precision"] == 0.0 and math.isnan(d["recall"]) and math.isnan(d["f1"])
    d = su.lesion_metrics(z, z, device="cpu")                  # both empty
    assert math.isnan(d["precision"]) and math.isnan(d["recall"]) and math.isnan(d["f1"]) and d["dice_largest"] == 1.0
    d = su.lesion_metrics(a, b, device="cpu")                  # no overlap at all
    assert d["precision"] == 0.0 and d["recall"] == 0.0 and d["f1"] == 0.0 and (d["fp"], d["fn"]) == (1, 1)
    assert set(d) == KEYS
    assert all(type(d[k]) is int for k in ("n_pred", "n_gt", "tp_pred", "tp_gt", "fp", "fn", "largest_pred",
                                           "largest_gt"))
    assert all(type(d[k]) is float for k in ("precision", "recall", "f1", "dice_largest"))
    d = su.lesion_metrics(a, a, device="cpu")
    assert d["precision"] == 1.0 and d["recall"] == 1.0 and d["f1"] == 1.0 and d["dice_largest_terms"] == (4, 4, 4)
    # any dtype, (1, D, H, W), tensors; non-zero is foreground
    want = su.lesion_metrics(a, b, device="cpu")
    for conv in (lambda t: t.astype(np.float32) * 2.5, lambda t: torch.from_numpy(t)[None],
                 lambda t: torch.from_numpy(t.astype(np.int64) * 3)):
        assert co.same_dict(su.lesion_metrics(conv(a), conv(b), device="cpu"), want)
    assert tuple(su.keep_largest_component(torch.from_numpy(a)[None], device="cpu").shape) == (1, 3, 6, 7)
    assert not su.keep_largest_component(z, device="cpu").any()


def test_arguments_are_validated_on_the_host(components_emu):
    from rehrseg_amd import hip_backend as hb
    a = np.ones((2, 3, 4), np.uint8)
    with pytest.raises(ValueError):
        su.lesion_metrics(a, a[:, :, :-1], device="cpu")
    with pytest.raises(ValueError):
        su.connected_components(a[0, 0], device="cpu")
    with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
        hb.seg_cc_check_extent((1 << 10, 1 << 10, (1 << 10) + 1))
    with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
        hb.seg_cc_check_extent((4, 0, 4))
    assert hb.seg_cc_check_extent((1024, 1024, 1024)) == (1024, 1024, 1024)
    z = torch.zeros((2, 3, 4), dtype=torch.uint8)
    with pytest.raises(L.RehrsegHipError, match="no CPU fallback"):
        hb.seg_cc_roots(z, 26)
    with pytest.raises(L.RehrsegHipError, match="no CPU fallback"):
        hb.seg_cc_lesion(z.int(), z.int(), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(L.RehrsegHipError, match="no CPU fallback"):
        hb.seg_cc_compact(z.int(), torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("case", ("thin", "multi"))
def test_evaluate_case_tuple_layout(components_emu, case):
    from toy_models import ToySegNet
    sep = int(G["sep"])
    img, label = G[f"{case}_img"].astype(np.float32), G[f"{case}_label"].astype(np.float32)
    patch = list(G[f"{case}_patch"])
    sp = (4.0, 0.75, 0.5)
    args = (ToySegNet(sep=sep), img, label, sep, patch, True, "cpu")
    plain = su._evaluate_case(*args)
    surf = su._evaluate_case(*args, True, sp)
    comp = su._evaluate_case(*args, components=True, connectivity=6)
    both = su._evaluate_case(*args, True, sp, True, 6)
    assert (len(plain), len(surf), len(comp), len(both)) == (5, 6, 6, 7)
    for out in (surf, comp, both):
        assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1]) and torch.equal(out[2], plain[2])
        assert out[3] == plain[3] and out[4] == plain[4]
    assert np.array_equal(plain[0], G[f"{case}_pred_lr"]) and plain[3] == G[f"{case}_dice_lr"]
    assert set(surf[5]) == {"hd", "hd95", "assd", "n_pred", "n_gt"} and both[5] == surf[5]
    want = co.lesion_dict(co.eight(plain[0], plain[2][0].numpy(), 6))
    assert co.same_dict(comp[5], want) and co.same_dict(both[6], want)
    assert want["n_pred"] > 0 and want["n_gt"] > 0
    # the public function drops the Dice terms; the default connectivity is 26
    public = su.evaluate_case(*args[:5], get_HR_results=True, device="cpu", components=True)
    assert len(public) == 5 and co.same_dict(public[4], co.lesion_dict(co.eight(plain[0], plain[2][0].numpy(), 26)))
    public = su.evaluate_case(*args[:5], get_HR_results=True, device="cpu", surface=True, spacing=sp, components=True)
    assert len(public) == 6 and public[4] == surf[5] and set(public[5]) == KEYS
    assert len(su.evaluate_case(*args[:5], get_HR_results=True, device="cpu")) == 4


def test_evaluate_cases_lesion_summary(components_emu, capsys):
    from rehrseg_amd.train_steps import evaluate_cases
    from toy_models import ToySegNet
    net = ToySegNet(sep=1)
    cases = [("thin", G["thin_img"], G["thin_label"]), ("multi", G["multi_img"], G["multi_label"]),
             ("empty", G["thin_img"], np.zeros_like(G["thin_label"]))]
    plain = evaluate_cases(net, cases, [16, 16, 8], device="cpu")
    text_plain = capsys.readouterr().out
    again = evaluate_cases(net, cases, [16, 16, 8], device="cpu", components=False)
    assert capsys.readouterr().out == text_plain and again == plain
    assert "Lesion" not in text_plain and "largest" not in text_plain
    plain_lines = text_plain.splitlines()
    assert [l.split(":")[0] for l in plain_lines] == ["Subject thin", "Subject multi", "Subject empty", "Global dice",
                                                       "Average dice", "Std dice", "Max dice", "Min dice"]
    mean = evaluate_cases(net, cases, [16, 16, 8], device="cpu", components=True, connectivity=18)
    lines = capsys.readouterr().out.splitlines()
    assert mean == plain
    outs = [su.evaluate_case(net, img, lab, 1, [8, 16, 16], device="cpu") for _, img, lab in cases]
    want = [co.lesion_dict(co.eight(o[0], np.asarray(lab)[0], 18)) for o, (_, _, lab) in zip(outs, cases)]
    for line, p, w in zip(lines[:3], plain_lines[:3], want):
        assert line == p + f" | Lesions: {w['tp_gt']}/{w['n_gt']} found, {w['fp']} false"
    assert lines[3:8] == plain_lines[3:]
    tot = {k: sum(w[k] for w in want) for k in ("n_pred", "n_gt", "tp_pred", "tp_gt", "fp", "fn")}
    micro = co.lesion_dict([tot["n_pred"], tot["n_gt"], tot["tp_pred"], tot["tp_gt"], 0, 0, 0, 0])
    largest = sum(w["dice_largest"] for w in want) / 3
    assert lines[8:] == [
        f"Lesions: {tot['tp_gt']}/{tot['n_gt']} found, {tot['fn']} missed; {tot['n_pred']} predicted, {tot['fp']} false",
        f"Lesion precision: {micro['precision']}", f"Lesion recall: {micro['recall']}", f"Lesion F1: {micro['f1']}",
        f"Average dice: {plain} | largest component only: {largest}",
        f"Keep largest component: {'yes (raises' if largest > plain else 'no (does not raise'} the mean Dice)"]
    # with the surface numbers as well: the lesion part follows the surface part, on the lines and in the summary
    evaluate_cases(net, cases, [16, 16, 8], device="cpu", surface=True, components=True, connectivity=18)
    both = capsys.readouterr().out.splitlines()
    assert " | HD95: " in both[0] and both[0].index(" | HD95: ") < both[0].index(" | Lesions: ")
    assert both[0].endswith(lines[0].split(" | ", 1)[1]) and both[-6:] == lines[-6:]


def test_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols()
    assert set(declared) == set(L.PROTOTYPES)
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    assert L.ABI_VERSION == 6 and lib.rehr_abi_version() == 6


def test_entry_points_reject_malformed_arguments_without_launching():
    """Every call below is malformed in exactly the way its row says; the other pointers are dummy addresses that
    nothing on the host dereferences, and no call reaches a launch."""
    lib = L.load()
    q = lib.rehr_seg_cc_workspace_bytes
    assert q(0, 4, 4) == ENOSUP and q(4, -1, 4) == ENOSUP and q(4, 4, 0) == ENOSUP
    assert q(1024, 1024, 1025) == ENOSUP and q(1 << 30, 2, 1) == ENOSUP and q(1 << 20, 1 << 20, 1 << 20) == ENOSUP
    assert q(1024, 1024, 1024) == 64 + 16 * (1 << 30) and q(1, 1, 1 << 30) > 0 and q(6, 20, 67) >= 64 + 16 * 6 * 20 * 67
    p = [0x10000, 0x20000, 0x30000]                              # mask, roots, workspace
    big = 1 << 40

    def roots(ptrs=p, dims=(4, 5, 6), conn=26, ws=big):
        return lib.rehr_seg_cc_roots_i32(ptrs[0], *dims, conn, ptrs[1], ptrs[2], ws, None)

    for k in range(3):
        assert roots(ptrs=[None if i == k else v for i, v in enumerate(p)]) == EINVAL, k
    for conn in (7, 0, 8, 27, -6):
        assert roots(conn=conn) == EINVAL, conn
    for dims in ((0, 5, 6), (4, -5, 6), (4, 5, 0), (1024, 1024, 1025)):
        assert roots(dims=dims) == ENOSUP, dims
    assert roots(ws=q(4, 5, 6) - 1) == EINVAL and roots(ptrs=[p[0], 0x20002, p[2]]) == EINVAL

    r = [0x10000, 0x20000, 0x30000, 0x40000]                     # roots_pred, roots_gt, out, workspace

    def lesion(ptrs=r, n=120, ws=big):
        return lib.rehr_seg_cc_lesion_i64(ptrs[0], ptrs[1], n, ptrs[2], ptrs[3], ws, None)

    for k in range(4):
        assert lesion(ptrs=[None if i == k else v for i, v in enumerate(r)]) == EINVAL, k
    assert lesion(n=0) == ENOSUP and lesion(n=(1 << 30) + 1) == ENOSUP
    assert lesion(ws=64 + 16 * 120 - 1) == EINVAL and lesion(ptrs=r[:3] + [0x40008]) == EINVAL
    assert lesion(ptrs=r[:2] + [0x30004, r[3]]) == EINVAL

    c = [0x10000, 0x20000, 0x30000, 0x40000]                     # roots, rank, labels, count

    def compact(ptrs=c, n=120):
        return lib.rehr_seg_cc_compact_i32(ptrs[0], n, ptrs[1], ptrs[2], ptrs[3], None)

    for k in range(4):
        assert compact(ptrs=[None if i == k else v for i, v in enumerate(c)]) == EINVAL, k
    assert compact(n=0) == ENOSUP and compact(n=(1 << 30) + 1) == ENOSUP
    assert compact(ptrs=c[:3] + [0x40004]) == EINVAL
