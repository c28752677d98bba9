"""Boundary metrics without a GPU: the pinned case of DESIGN section 3.15 through surface_distance_metrics over the CPU
statement of its kernels (tests/surface_emu.py), the brute-force oracle against scipy, the host logic of
evaluate_case(surface=True) / evaluate_cases(surface=True) on the toy network of tests/golden/eval_case.npz, and the
three new C-ABI symbols with their argument checks."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import surface_oracle as so
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import seg_utils as su
from test_eval_cpu import G

NEW_SYMBOLS = ("rehr_seg_surface_workspace_bytes", "rehr_seg_surface_dist_f32", "rehr_seg_surface_reduce_f64")
EINVAL, ENOSUP = -1, -2
KEYS = ("hd", "hd95", "assd")


@pytest.fixture
def surface_emu():
    import surface_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


def _same(got, want, tol=1e-12):
    assert got["n_pred"] == want["n_pred"] and got["n_gt"] == want["n_gt"], (got, want)
    for k in KEYS:
        if math.isnan(want[k]):
            assert math.isnan(got[k]), (k, got)
        else:
            assert abs(got[k] - want[k]) <= tol * max(1.0, abs(want[k])), (k, got[k], want[k])


def test_pinned_case_through_the_public_function(surface_emu):
    P, Gt, sp, want = so.pinned_case()
    got = su.surface_distance_metrics(P, Gt, sp, device="cpu")
    assert set(got) == {"hd", "hd95", "assd", "n_pred", "n_gt"}
    assert all(isinstance(got[k], float) for k in KEYS) and isinstance(got["n_pred"], int)
    _same(got, want)
    _same(so.metrics(P, Gt, sp), want)
    # any dtype, (1, D, H, W), tensors; non-zero is foreground
    for conv in (lambda a: a.astype(np.float32) * 2.5, lambda a: torch.from_numpy(a)[None],
                 lambda a: torch.from_numpy(a.astype(np.int64) * 3)):
        _same(su.surface_distance_metrics(conv(P), conv(Gt), sp, device="cpu"), want)


def test_empty_masks_give_nan_and_counts(surface_emu):
    P, Gt, sp, want = so.pinned_case()
    got = su.surface_distance_metrics(np.zeros_like(P), Gt, sp, device="cpu")
    assert got["n_pred"] == 0 and got["n_gt"] == want["n_gt"] and all(math.isnan(got[k]) for k in KEYS)
    got = su.surface_distance_metrics(P, np.zeros_like(P), sp, device="cpu")
    assert got["n_pred"] == want["n_pred"] and got["n_gt"] == 0 and all(math.isnan(got[k]) for k in KEYS)
    same = su.surface_distance_metrics(P, P, sp, device="cpu")
    assert same["hd"] == 0.0 and same["hd95"] == 0.0 and same["assd"] == 0.0


def test_spacing_and_extent_are_validated_on_the_host(surface_emu):
    P, Gt, _, _ = so.pinned_case()
    for bad in ((1, 1), (1, 0, 1), (1, -2, 1), (float("nan"), 1, 1), (1, 1, float("inf"))):
        with pytest.raises(ValueError):
            su.surface_distance_metrics(P, Gt, bad, device="cpu")
    with pytest.raises(ValueError):
        su.surface_distance_metrics(P, Gt[:, :, :-1], device="cpu")
    big = np.zeros((1, 1, 2049), np.uint8)
    with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
        su.surface_distance_metrics(big, big, device="cpu")


def test_oracle_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    P, Gt, sp, _ = so.pinned_case()
    rng = np.random.RandomState(7)
    cases = [(P, Gt, sp), (rng.rand(6, 20, 24) < 0.3, rng.rand(6, 20, 24) < 0.3, (4.0, 0.75, 0.5)),
             (so.ellipsoid((1, 33, 40), (0, 15, 20), (1, 9, 13)), so.ellipsoid((1, 33, 40), (0, 18, 17), (1, 11, 8)),
              (3.0, 1.25, 1.0))]
    st = ndi.generate_binary_structure(3, 1)
    for A, B, spacing in cases:
        sa, sb = so.surface(A), so.surface(B)
        assert np.array_equal(sa, A ^ ndi.binary_erosion(A, st)) and np.array_equal(sb, B ^ ndi.binary_erosion(B, st))
        to_b = ndi.distance_transform_edt(~sb, sampling=spacing)[sa]
        to_a = ndi.distance_transform_edt(~sa, sampling=spacing)[sb]
        m = so.metrics(A, B, spacing)
        assert np.array_equal(m["s_pg"], np.sort(to_b)) and np.array_equal(m["s_gp"], np.sort(to_a))
        assert m["hd"] == max(to_b.max(), to_a.max())
        assert m["hd95"] == np.percentile(np.concatenate([to_b, to_a]), 95)
        assert m["assd"] == (to_b.mean() + to_a.mean()) / 2


@pytest.mark.parametrize("case", ("thin", "multi"))
def test_evaluate_case_surface_on_the_toy_network(surface_emu, case):
    from toy_models import ToySegNet
    sep = int(G["sep"])
    img, label = G[f"{case}_img"].astype(np.float32), G[f"{case}_label"].astype(np.float32)
    patch = list(G[f"{case}_patch"])
    sp = (4.0, 0.75, 0.5)
    plain = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, patch, get_HR_results=True, device="cpu")
    out = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, patch, get_HR_results=True, device="cpu",
                           surface=True, spacing=sp)
    assert len(plain) == 4 and len(out) == 5
    assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1]) and out[3] == plain[3]
    assert torch.equal(out[2], plain[2])
    assert np.array_equal(out[0], G[f"{case}_pred_lr"]) and out[3] == G[f"{case}_dice_lr"]
    _same(out[4], so.metrics(out[0], out[2][0].numpy(), sp))
    assert out[4]["n_pred"] > 0 and out[4]["n_gt"] > 0
    # arrays carry no spacing: (1, 1, 1)
    unit = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, patch, device="cpu", surface=True)
    _same(unit[4], so.metrics(out[0], out[2][0].numpy()))


def test_evaluate_cases_surface_summary(surface_emu, capsys):
    from rehrseg_amd.train_steps import evaluate_cases
    from toy_models import ToySegNet
    net = ToySegNet(sep=1)
    cases = [("thin", G["thin_img"], G["thin_label"]), ("multi", G["multi_img"], G["multi_label"]),
             ("empty", G["thin_img"], np.zeros_like(G["thin_label"]))]
    plain = evaluate_cases(net, cases, [16, 16, 8], device="cpu")
    text_plain = capsys.readouterr().out
    sp = (5.0, 0.5, 0.5)
    mean = evaluate_cases(net, cases, [16, 16, 8], device="cpu", surface=True, spacing=sp)
    text = capsys.readouterr().out
    assert mean == plain
    assert "HD95" not in text_plain and "ASSD" not in text_plain
    want = [so.metrics(su.evaluate_case(net, img, lab, 1, [8, 16, 16], device="cpu")[0], np.asarray(lab)[0], sp)
            for _, img, lab in cases]
    subj = [line for line in text.splitlines() if line.startswith("Subject ")]
    assert len(subj) == 3
    for line, w, p in zip(subj, want, [l for l in text_plain.splitlines() if l.startswith("Subject ")]):
        assert line.startswith(p + " | HD95: ")
        hd95, assd = (float(v.split(": ")[1]) for v in line.split(" | ")[1:])
        for got, k in ((hd95, "hd95"), (assd, "assd")):
            assert (math.isnan(got) and math.isnan(w[k])) or abs(got - w[k]) <= 1e-12 * max(1.0, w[k])
    finite = [w for w in want if not math.isnan(w["hd95"])]
    assert len(finite) == 2
    val = {line.split(": ")[0]: line.split(": ")[1] for line in text.splitlines() if ": " in line}
    for k, label in (("hd95", "HD95"), ("assd", "ASSD")):
        v = [w[k] for w in finite]
        assert abs(float(val[f"Average {label}"]) - sum(v) / 2) <= 1e-12 * max(v)
        assert abs(float(val[f"Std {label}"]) - np.std(v)) <= 1e-12 * max(v)
        assert abs(float(val[f"Max {label}"]) - max(v)) <= 1e-12 * max(v)
        assert abs(float(val[f"Min {label}"]) - min(v)) <= 1e-12 * max(v)
    assert val["Empty-surface cases"] == "1 of 3"
    # the summary of the plain run is a prefix, line for line apart from the subject lines
    rest = [l for l in text.splitlines() if not l.startswith("Subject ")]
    assert rest[:5] == [l for l in text_plain.splitlines() if not l.startswith("Subject ")]


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.PROTOTYPES and hasattr(lib, s), s
    assert L.ABI_VERSION == 6 and lib.rehr_abi_version() == 6


def test_workspace_query():
    lib = L.load()
    q = lib.rehr_seg_surface_workspace_bytes
    assert q(0, 4, 4) == EINVAL and q(4, -1, 4) == EINVAL and q(4, 4, 0) == EINVAL
    assert q(2049, 1, 1) == ENOSUP and q(1, 1, 2049) == ENOSUP and q(2048, 2048, 2048) == ENOSUP
    assert q(1024, 1024, 1024) > 0 and q(2048, 1, 1) > 0
    n = 6 * 20 * 24
    assert q(6, 20, 24) >= 17 * n and q(1, 1, 1) >= 4096


def test_entry_points_reject_malformed_arguments_without_launching():
    """Every call below is malformed in exactly the way its row says; the other pointers are dummy addresses that
    nothing on the host dereferences, and no call reaches a launch."""
    lib = L.load()
    dist_fn, red_fn = lib.rehr_seg_surface_dist_f32, lib.rehr_seg_surface_reduce_f64
    p = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]      # pred, gt, dist, counts, workspace
    big = 1 << 40

    def dist(ptrs=p, dims=(4, 5, 6), sp=(1.0, 1.0, 1.0), ws=big):
        return dist_fn(ptrs[0], ptrs[1], *dims, *sp, ptrs[2], ptrs[3], ptrs[4], ws, None)

    for k in range(5):
        assert dist(ptrs=[None if i == k else v for i, v in enumerate(p)]) == EINVAL, k
    for dims in ((0, 5, 6), (4, -5, 6), (4, 5, 0)):
        assert dist(dims=dims) == EINVAL, dims
    for dims in ((2049, 1, 1), (1, 2049, 1), (1, 1, 2049), (2048, 2048, 2048)):
        assert dist(dims=dims) == ENOSUP, dims
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for k in range(3):
            sp = [1.0, 1.0, 1.0]
            sp[k] = bad
            assert dist(sp=sp) == EINVAL, sp
    need = lib.rehr_seg_surface_workspace_bytes(4, 5, 6)
    assert dist(ws=need - 1) == EINVAL and dist(ws=0) == EINVAL
    assert dist(ptrs=p[:4] + [0x50008]) == EINVAL                     # workspace not 16-byte aligned
    assert dist(ptrs=p[:3] + [0x40004, p[4]]) == EINVAL               # counts not 8-byte aligned

    q = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]      # dist, sorted, counts, out, workspace

    def red(ptrs=q, n=120, ws=4096):
        return red_fn(ptrs[0], ptrs[1], ptrs[2], n, ptrs[3], ptrs[4], ws, None)

    for k in range(5):
        assert red(ptrs=[None if i == k else v for i, v in enumerate(q)]) == EINVAL, k
    assert red(n=0) == EINVAL and red(n=-3) == EINVAL
    assert red(n=(1 << 30) + 1) == ENOSUP
    assert red(ws=4095) == EINVAL
    assert red(ptrs=q[:3] + [0x40004, q[4]]) == EINVAL                # out not 8-byte aligned


def test_backend_wrappers_refuse_cpu_tensors_and_large_extents():
    from rehrseg_amd import hip_backend as hb
    z = torch.zeros((2, 3, 4), dtype=torch.uint8)
    with pytest.raises(L.RehrsegHipError, match="no CPU fallback"):
        hb.seg_surface_distances(z, z, (1.0, 1.0, 1.0), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
        hb.seg_surface_check_extent((1, 2049, 1))
    assert hb.seg_surface_check_extent((1024, 1024, 1024)) == (1024, 1024, 1024)
    hdr = open(L.HEADER_PATH).read()
    assert f"#define REHR_SEG_SURFACE_MAX_AXIS {hb.SEG_SURFACE_MAX_AXIS}\n" in hdr
