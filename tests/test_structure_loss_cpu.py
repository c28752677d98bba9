"""Stage-1 structure losses without a GPU: the three new C-ABI symbols and their argument checks, the launch layer's and
the module's refusals, the CPU statement of both kernels (tests/structure_loss_emu.py) through models.losses and
autograd against the fp64 oracle (tests/structure_loss_cases.py, where the bars are derived), the two functions under
the reference's names, and the drop-in import."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import structure_loss_cases as lc
from rehrseg_amd import lib as L
from rehrseg_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rehr_structure_loss_workspace_bytes", "rehr_structure_loss_fwd_f32", "rehr_structure_loss_bwd_f32")


@pytest.fixture
def lemu():
    import structure_loss_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


def _run(loss_fn, p, t, go=None):
    """loss_fn(input, target) through autograd on CPU tensors -> (value, gradient as numpy)."""
    x = torch.from_numpy(np.array(p)).requires_grad_()
    loss = loss_fn(x, torch.from_numpy(np.array(t)))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss if go is None else loss * go).backward()
    return float(loss.detach()), x.grad.numpy()


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.PROTOTYPES and hasattr(lib, s), s
    assert L.ABI_VERSION == 6 and lib.rehr_abi_version() == 6      # new entry points, no signature changed


def test_workspace_query():
    q = L.load().rehr_structure_loss_workspace_bytes
    assert q(1, 1, 1, 11, 11) == 32 and q(1, 1, 1, 1, 5) == 32       # four doubles per tile, also below the SSIM window
    assert q(2, 3, 4, 128, 128) == 2 * q(1, 3, 4, 128, 128) == 6 * q(1, 1, 4, 128, 128) == 24 * q(1, 1, 1, 128, 128)
    assert q(1, 1, 1, 33, 32) == 2 * q(1, 1, 1, 32, 32) == q(1, 1, 1, 32, 33)
    for bad in ((0, 1, 1, 11, 11), (1, 0, 1, 11, 11), (1, 1, 0, 11, 11), (1, 1, 1, 0, 11), (1, 1, 1, 11, -1)):
        assert q(*bad) == -1, bad


def test_malformed_arguments_are_rejected_before_any_launch():
    """Host addresses that no kernel dereferences: every call returns before a launch."""
    lib = L.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    st = (ctypes.c_int64 * 5)(121, 121, 121, 11, 1)
    neg = (ctypes.c_int64 * 5)(121, 121, 121, -11, 1)
    zero = (ctypes.c_int64 * 5)(121, 121, 121, 0, 1)
    need = lib.rehr_structure_loss_workspace_bytes(1, 1, 1, 11, 11)
    nan, inf = float("nan"), float("inf")

    def fwd(x=p, xs=st, t=p, ts=st, dims=(1, 1, 1, 11, 11), w=(1.0, 0.0, 1.0, 1.0), rng=1.0, stats=p, loss=p, fields=p,
            ws=p, nbytes=need):
        return lib.rehr_structure_loss_fwd_f32(x, xs, t, ts, *dims, *w, rng, stats, loss, fields, ws, nbytes, None)

    def bwd(x=p, xs=st, t=p, ts=st, dims=(1, 1, 1, 11, 11), w=(1.0, 0.0, 1.0, 1.0), fields=p, go=p, dx=p, ds=st):
        return lib.rehr_structure_loss_bwd_f32(x, xs, t, ts, *dims, *w, fields, go, dx, ds, None)

    for call in (fwd, bwd):
        assert call(x=None) == -1 and call(xs=None) == -1 and call(t=None) == -1 and call(ts=None) == -1
        assert call(xs=neg) == -1 and call(ts=neg) == -1
        for dims in ((0, 1, 1, 11, 11), (1, 0, 1, 11, 11), (1, 1, 0, 11, 11), (1, 1, 1, 0, 11), (1, 1, 1, 11, -3)):
            assert call(dims=dims) == -1, dims
        for w in ((nan, 0, 0, 0), (0, inf, 0, 0), (0, 0, nan, 0), (0, 0, 0, -inf)):
            assert call(w=w) == -1, w
        # the SSIM window does not fit: unsupported, but only when the term is asked for
        assert call(dims=(1, 1, 1, 10, 11)) == -2 and call(dims=(1, 1, 1, 11, 10)) == -2
        assert call(dims=(1, 1, 1, 1, 5)) == -2
    assert fwd(stats=None) == -1 and fwd(loss=None) == -1 and fwd(ws=None) == -1
    assert fwd(rng=0.0) == -1 and fwd(rng=-1.0) == -1 and fwd(rng=nan) == -1
    assert fwd(nbytes=need - 1) == -1 and fwd(dims=(2, 1, 1, 11, 11)) == -1
    assert fwd(ws=ctypes.c_void_p(p.value + 4)) == -1 and fwd(loss=ctypes.c_void_p(p.value + 2)) == -1
    assert bwd(go=None) == -1 and bwd(dx=None) == -1 and bwd(ds=None) == -1 and bwd(ds=neg) == -1
    assert bwd(fields=None) == -1                                     # the SSIM term's gradient needs the forward's fields
    assert bwd(ds=zero) == -1                                         # two pixels of d input at one address


def test_launch_layer_and_module_refusals(lemu):
    from rehrseg_amd import hip_backend as hb
    from rehrseg_amd.models.losses import StructureLoss
    w = (1.0, 0.0, 0.0, 1.0)
    x = torch.zeros(1, 1, 1, 11, 11)
    with pytest.raises(L.RehrsegHipError, match="device tensor"):
        hb.structure_loss_fwd(x, x, w)
    with pytest.raises(L.RehrsegHipError, match="device tensor"):
        hb.structure_loss_bwd(x, x, w, None, torch.ones(1))
    meta = torch.zeros(1, 1, 1, 11, 11, device="meta")

    class Dev(torch.Tensor):
        """A meta tensor that claims to live on the device: reaches the checks behind `is_cuda`, never a launch."""
        is_cuda = True

    def dev(t):
        return t.as_subclass(Dev)

    for bad in (meta.half(), meta.double(), meta.bfloat16()):
        with pytest.raises(L.RehrsegHipError, match="float32"):
            hb.structure_loss_fwd(dev(bad), dev(meta), w)
        with pytest.raises(L.RehrsegHipError, match="float32"):
            hb.structure_loss_fwd(dev(meta), dev(bad), w)
    with pytest.raises(L.RehrsegHipError, match="one shape"):
        hb.structure_loss_fwd(dev(meta), dev(torch.zeros(1, 1, 1, 11, 12, device="meta")), w)
    with pytest.raises(L.RehrsegHipError, match="one shape"):
        hb.structure_loss_fwd(dev(meta[0, 0]), dev(meta[0, 0]), w)
    with pytest.raises(L.RehrsegHipError, match="four weights"):
        hb.structure_loss_fwd(dev(meta), dev(meta), (1.0, 0.0))
    # the module: a target that asks for a gradient, and a slice the SSIM window does not fit
    with pytest.raises(ValueError, match="target"):
        StructureLoss()(x, x.clone().requires_grad_())
    with pytest.raises(ValueError, match="H, W >= 11"):
        StructureLoss(ssim=1.0)(torch.zeros(1, 1, 1, 10, 12), torch.zeros(1, 1, 1, 10, 12))
    assert float(StructureLoss(ssim=0.0, sobel=1.0)(torch.zeros(1, 1, 1, 10, 12), torch.zeros(1, 1, 1, 10, 12))) == 0.0


def test_module_refuses_host_tensors_on_the_product_backend():
    from rehrseg_amd.models.losses import StructureLoss, l1_sobel_loss
    x = torch.zeros(1, 1, 1, 11, 11)
    with pytest.raises(L.RehrsegHipError):
        StructureLoss(l1=1.0, ssim=1.0)(x, x)
    with pytest.raises(L.RehrsegHipError):
        l1_sobel_loss(x, x)


@pytest.mark.parametrize("term", list(lc.TERMS))
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", lc.KINDS)
def test_cpu_statement_against_the_oracle(lemu, kind, shape, term):
    from rehrseg_amd.models.losses import StructureLoss
    p, t, rng, ref = lc.reference(kind, shape, term)
    l1, l2, ssim, sobel = lc.TERMS[term]
    value, grad = _run(StructureLoss(l1, l2, ssim, sobel, data_range=rng), p, t)
    lc.check(f"emu {kind} {shape} {term}", value, grad, p, t, lc.TERMS[term], rng, ref)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_cpu_statement_one_row_slices_and_four_dimensions(lemu, kind):
    from rehrseg_amd.models.losses import StructureLoss
    w = (1.0, 0.5, 0.0, 1.3)
    p, t, rng = lc.make_case(kind, lc.ROW_SHAPE)
    value, grad = _run(StructureLoss(*w, data_range=rng), p, t)
    lc.check(f"emu {kind} {lc.ROW_SHAPE}", value, grad, p, t, w, rng)
    # (N, C, H, W) is (N, C, 1, H, W)
    p, t, rng, ref = lc.reference(kind, (1, 2, 2, 45, 37), "all")
    v5, g5 = _run(StructureLoss(*lc.TERMS["all"], data_range=rng), p[:, :, :1], t[:, :, :1])
    v4, g4 = _run(StructureLoss(*lc.TERMS["all"], data_range=rng), p[:, :, 0], t[:, :, 0])
    assert v4 == v5 and g4.shape == (1, 2, 45, 37) and np.array_equal(g4, g5[:, :, 0])


def test_reference_named_functions_and_their_argument_order(lemu):
    from rehrseg_amd.models import losses
    p, t, rng = lc.make_case("a", (1, 2, 2, 45, 37))
    for fn, w in ((losses.l1_sobel_loss, (1.0, 0.0, 0.0, 1.0)), (losses.l2_sobel_loss, (0.0, 1.0, 0.0, 1.0))):
        value, grad = _run(lambda x, y: fn(y, x), p, t)                 # (y_true, y_pred): the gradient goes to y_pred
        lc.check(f"emu {fn.__name__}", value, grad, p, t, w, rng)
        v2, g2 = _run(losses.StructureLoss(*w), p, t)
        assert v2 == value and np.array_equal(g2, grad)
        y_true = torch.from_numpy(np.array(t)).requires_grad_()
        with pytest.raises(ValueError, match="target"):
            fn(y_true, torch.from_numpy(np.array(p)))


def test_a_weight_of_zero_leaves_the_other_terms_unchanged(lemu):
    p, t, rng = lc.make_case("b", (2, 1, 3, 12, 43))
    pt, tt = torch.from_numpy(p), torch.from_numpy(t)
    full = (1.0, 0.5, 0.7, 1.3)
    _, stats, fields = lemu.structure_loss_fwd(pt, tt, full, rng)
    gfull = lemu.structure_loss_bwd(pt, tt, full, fields, torch.ones(1)).numpy().astype(np.float64)
    gsum = np.zeros_like(gfull)
    V, M = p.size, 2 * 3 * 2 * 33
    for k in range(4):
        w = tuple(v if i == k else 0.0 for i, v in enumerate(full))
        loss, s, f = lemu.structure_loss_fwd(pt, tt, w, rng)
        assert torch.equal(s[:, k], stats[:, k]) and not s[:, [i for i in range(4) if i != k]].any()
        assert (f is not None) == (k == 2) and (f is None or torch.equal(f, fields))
        want = w[k] * (1 - float(s[:, k].sum()) / M) if k == 2 else w[k] * float(s[:, k].sum()) / V
        assert float(loss) == pytest.approx(want, rel=1e-6)
        gsum += lemu.structure_loss_bwd(pt, tt, w, f, torch.ones(1)).numpy()
    # the four gradients add up to the fused one: each is rounded to fp32 once, the fused sum four times
    assert np.abs(gsum - gfull).max() <= 8 * 2.0 ** -24 * np.abs(gfull).max()
    assert lemu.structure_loss_fwd(pt, tt, full, rng, need_grad=False)[2] is None


@pytest.mark.parametrize("kind", lc.KINDS)
def test_identical_images_give_exactly_zero(lemu, kind):
    from rehrseg_amd.models.losses import StructureLoss
    _, t, rng = lc.make_case(kind, (1, 2, 2, 45, 37))
    value, grad = _run(StructureLoss(1.0, 0.5, 0.7, 1.3, data_range=rng), t, t)
    assert value == 0.0 and np.isfinite(grad).all()


def test_grad_output_scales_the_gradient(lemu):
    from rehrseg_amd.models.losses import StructureLoss
    p, t, rng = lc.make_case("a", (2, 1, 3, 12, 43))
    fn = StructureLoss(1.0, 0.5, 0.7, 1.3)
    _, g1 = _run(fn, p, t)
    _, g3 = _run(fn, p, t, go=-3.0)
    assert np.abs(g3 - np.float32(-3.0) * g1).max() <= 2.0 ** -23 * np.abs(g3).max()


def test_models_losses_resolves_through_the_drop_in_alias():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from models.losses import l1_sobel_loss, l2_sobel_loss, StructureLoss\n"
            "import rehrseg_amd.models.losses as real\n"
            "assert l1_sobel_loss is real.l1_sobel_loss and StructureLoss is real.StructureLoss\n"
            "try:\n"
            "    import models.wdsr\n"
            "except ImportError:\n"
            "    pass\n"
            "else:\n"
            "    raise SystemExit('models.wdsr should not resolve')\n"
            "print('LOSSES_OK')\n" % os.path.join(ROOT, "rehrseg_amd"))
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LOSSES_OK" in r.stdout, r.stdout + r.stderr
