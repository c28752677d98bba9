"""Stage-2 validation without a GPU: the drop-in import line of train_all.py:29, calculate_dice and pad_nd_image, the
SimpleITK requirement of file paths, the three new C-ABI symbols, and the host logic of evaluate_case over the CPU
emulation of its kernels (tests/eval_emu.py) against the reference's own outputs (tests/golden/eval_case.npz, written
by tools/gen_golden_eval.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import seg_utils as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "eval_case.npz"))
CASES = ("thin", "multi")
NEW_SYMBOLS = ("rehr_tta_gather_f32", "rehr_tta_blend_f16acc", "rehr_seg_eval_finalize_f16")


def test_train_all_import_line_resolves_in_clean_interpreter(tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from utils.seg_utils import zscore_normalization, BCEDiceLoss, _build_loss, evaluate_case, calculate_dice\n"
            "import rehrseg_amd.utils.seg_utils as real\n"
            "assert evaluate_case is real.evaluate_case and calculate_dice is real.calculate_dice\n"
            "assert zscore_normalization is real.zscore_normalization and _build_loss is real._build_loss\n"
            "print('ok')\n") % os.path.join(ROOT, "rehrseg_amd")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_calculate_dice_reproduces_the_reference():
    a, b = G["dice_a"], G["dice_b"]
    assert su.calculate_dice(a, b) == G["dice_u8"]
    assert su.calculate_dice(a, b.astype(np.float32)) == G["dice_f32"]
    assert su.calculate_dice(a * 0, b * 0, smooth=1.0) == G["dice_smooth"]
    for c in CASES:
        assert su.calculate_dice(G[f"{c}_pred_lr"], G[f"{c}_label"]) == G[f"{c}_dice_lr"]


def test_dice_from_counts_equals_calculate_dice():
    a, b = G["dice_a"], G["dice_b"]
    terms = (int((a * b).sum()), int(a.sum()), int(b.sum()))
    assert su._dice_from_counts(*terms) == su.calculate_dice(a, b)


@pytest.mark.parametrize("shape,new", [((1, 5, 24, 13), [8, 16, 16]), ((2, 9, 7), [4, 12, 7]),
                                       ((1, 3, 4, 5), [2, 2, 2])])
def test_pad_nd_image_round_trips(shape, new):
    x = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape) + 1
    for img, kw in ((x, {"value": 0}), (x.numpy(), {"constant_values": 0})):   # F.pad's / np.pad's keyword
        res, sl = su.pad_nd_image(img, new, "constant", kw, True, None)
        want = [max(s, n) for s, n in zip(shape, [shape[0]] * (len(shape) - len(new)) + list(new))]
        assert list(res.shape) == want
        back = res[sl]
        assert tuple(back.shape) == tuple(shape) and (np.asarray(back) == np.asarray(img)).all()
        assert float(np.asarray(res).sum()) == float(np.asarray(img).sum())     # the rest is the constant 0
        for s, n, w in zip(sl, shape, want):
            assert s.start == (w - n) // 2 and s.stop - s.start == n
    assert su.pad_nd_image(x, list(shape[1:])) is x                               # nothing to pad


def test_file_paths_need_simpleitk(tmp_path):
    try:
        import SimpleITK  # noqa: F401
    except ImportError:
        pass
    else:
        pytest.skip("SimpleITK is installed")
    with pytest.raises(ImportError, match="SimpleITK"):
        su.preprocess_image(str(tmp_path / "case_0000.nii.gz"))
    with pytest.raises(ImportError, match="SimpleITK"):
        su.evaluate_case(torch.nn.Identity(), str(tmp_path / "a.nii.gz"), str(tmp_path / "b.nii.gz"), 1, [4, 4, 4],
                         device="cpu")


def test_preprocess_image_zscores_on_the_host():
    raw = G["multi_img"].astype(np.float32)
    data, props = su.preprocess_image(raw)
    ref = raw.copy()
    ref -= ref.mean()
    ref /= max(ref.std(), 1e-8)
    assert data.dtype == torch.float32 and tuple(data.shape) == raw.shape and props == {}
    assert np.array_equal(data.numpy(), ref)
    lab, _ = su.preprocess_image(torch.from_numpy(G["multi_label"]), apply_norm=False)
    assert np.array_equal(lab.numpy(), G["multi_lr_label"])


def test_slice_separation_must_be_integral():
    with pytest.raises(ValueError):
        su.evaluate_case(torch.nn.Identity(), G["thin_img"], G["thin_label"], 2.5, [8, 16, 16], device="cpu")


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.PROTOTYPES and hasattr(lib, s), s
    assert lib.rehr_abi_version() == L.ABI_VERSION


def test_new_entry_points_reject_malformed_arguments_without_launching():
    import ctypes
    lib = L.load()
    assert lib.rehr_tta_gather_f32(None, None, 4, 4, 4, 0, 0, 0, 0, 0, 0, 2, 2, 2, None) == -1
    strides = (ctypes.c_int64 * 5)(8, 1, 1, 1, 1)
    assert lib.rehr_tta_blend_f16acc(None, strides, 2, 1, 1, 1, None, None, None, 1, 1, 1, 0, 0, 0, None) == -1
    assert lib.rehr_seg_eval_finalize_f16(None, None, 1, 1, 1, 0, 0, 0, 1, 1, 1, None, None, None, None) == -1


@pytest.fixture
def eval_emu():
    import eval_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


@pytest.mark.parametrize("case", CASES)
def test_evaluate_case_host_logic_matches_reference_fixture(eval_emu, case):
    from toy_models import ToySegNet
    sep = int(G["sep"])
    img, label = G[f"{case}_img"].astype(np.float32), G[f"{case}_label"].astype(np.float32)
    pred_lr, pred_hr, lr_label, dice = su.evaluate_case(ToySegNet(sep=sep), img, label, float(sep),
                                                        list(G[f"{case}_patch"]), get_HR_results=True, device="cpu")
    assert pred_lr.dtype == np.uint8 and np.array_equal(pred_lr, G[f"{case}_pred_lr"])
    assert pred_hr.dtype == np.uint8 and np.array_equal(pred_hr, G[f"{case}_pred_hr"])
    assert isinstance(lr_label, torch.Tensor) and lr_label.dtype == torch.float32
    assert np.array_equal(lr_label.numpy(), G[f"{case}_lr_label"])
    assert isinstance(dice, np.float64) and dice == G[f"{case}_dice_lr"]
    lr_only = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, list(G[f"{case}_patch"]), device="cpu")
    assert lr_only[1] is lr_only[0] and np.array_equal(lr_only[0], pred_lr) and lr_only[3] == dice


def test_fused_predictor_emulation_matches_existing_predictor(eval_emu):
    """The tile loop's host logic (gather geometry, blend offsets, HR depth) and the kernels' rounding contract
    against the unchanged torch predictor on the CPU, bit for bit."""
    from toy_models import ToySegNet
    net = ToySegNet(sep=2)
    data = su.preprocess_image(G["multi_img"].astype(np.float32))[0]
    patch = [int(p) for p in G["multi_patch"]]
    sl = su._internal_get_sliding_window_slicers(data.shape[1:], patch_size=patch)
    for out_idx, sep, gauss in ((0, 1, True), (1, 2, False)):
        ps = [patch[0] * sep, patch[1], patch[2]] if out_idx else patch
        want = su._internal_predict_sliding_window_return_logits(data.clone(), sl, net, False, out_idx, sep, ps,
                                                                 use_gaussian=gauss, deep_supervision=False)
        got = su._fused_predict_sliding_window_return_logits(data.clone(), sl, net, out_idx, sep, ps,
                                                             use_gaussian=gauss, deep_supervision=False)
        assert got.dtype == torch.half and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_evaluate_cases_global_dice_from_summed_terms(eval_emu, capsys):
    from rehrseg_amd.train_steps import evaluate_cases
    from toy_models import ToySegNet
    net = ToySegNet(sep=1)
    cases = [("thin", G["thin_img"], G["thin_label"]), ("multi", G["multi_img"], G["multi_label"]),
             ("thin_flipped", G["thin_img"][:, :, ::-1].copy(), G["thin_label"][:, :, ::-1].copy())]
    mean = evaluate_cases(net, cases, [16, 16, 8], device="cpu")
    out = capsys.readouterr().out
    assert "Average dice" in out and out.count("Subject ") == 3
    per = [float(line.split(": ")[1]) for line in out.splitlines() if line.startswith("Subject ")]
    assert abs(mean - sum(per) / 3) < 1e-12
    maps = [su.evaluate_case(net, img, lab, 1, [8, 16, 16], device="cpu")[0] for _, img, lab in cases]
    glob = float(next(line for line in out.splitlines() if line.startswith("Global dice")).split(": ")[1])
    assert glob == su.calculate_dice(np.concatenate([m.ravel() for m in maps]),
                                     np.concatenate([c[2].ravel() for c in cases]))
