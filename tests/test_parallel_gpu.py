"""PatchParallel on the device (single rank): the weight-gradient kernels write straight into the flat gradient
buffer; the result must equal plain autograd accumulation, also over two accumulated backward passes."""
import socket

import pytest
import torch

from oracle.detinit import det_tensor
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D
from rehrseg_amd.parallel import PatchParallel

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _model(dev):
    m = UNet_3D_3D(2, "unet_18", 4, 4)
    m.load_state_dict({k: det_tensor(k, tuple(v.shape)) for k, v in m.state_dict().items()})
    return m.to(dev)


def test_direct_gradient_writes_equal_autograd_accumulation():
    from rehrseg_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 2, 4, 32, 32, generator=g).to(dev)
    ref = _model(dev)
    for _ in range(2):                                   # two accumulated backward passes
        ref(x.clone()).abs().mean().backward()
    want = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}

    m = _model(dev)
    pp = PatchParallel(m)
    n_direct = sum(1 for p in m.parameters() if p.data_ptr() in ops._direct_grad)
    assert n_direct >= 20
    pp.zero_grad()
    for _ in range(2):
        m(x.clone()).abs().mean().backward()
    assert len(pp._written) >= 20                        # the conv weights really took the direct path
    pp.reduce_gradients()
    for n, p in m.named_parameters():
        if n not in want:
            continue
        scale = float(want[n].abs().max()) + 1e-30
        assert float((p.grad - want[n]).abs().max()) <= 2e-5 * scale, n
    # a new step starts from zero again
    pp.zero_grad()
    m(x.clone()).abs().mean().backward()
    for n, p in m.named_parameters():
        if n not in want:
            continue
        scale = float(want[n].abs().max()) + 1e-30
        assert float((p.grad - want[n] / 2).abs().max()) <= 2e-5 * scale, n


OVERLAP_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, {root!r})
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)          # RCCL communicator first, then the kernels
from oracle.detinit import det_tensor
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D
from rehrseg_amd.parallel import PatchParallel
dev = torch.device("cuda:0")
def model():
    m = UNet_3D_3D(2, "unet_18", 4, 4)
    m.load_state_dict({{k: det_tensor(k, tuple(v.shape)) for k, v in m.state_dict().items()}})
    return m.to(dev)
g = torch.Generator().manual_seed(2)
x = torch.rand(2, 2, 4, 32, 32, generator=g).to(dev)
ref = model()
ref(x.clone()).abs().mean().backward()
want = {{n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}}
m = model()
pp = PatchParallel(m, bucket_mb=8, force_overlap=True)         # ~12 buckets, launched from hooks during backward
assert pp.overlap and pp.exchange and len(pp.buckets) >= 8
worst, launched_in_backward, written = 0.0, [], []
for step in range(3):
    if step == 1:
        torch.optim.SGD(m.parameters(), lr=0.0).zero_grad()     # plain zero_grad(set_to_none=True) in between
    else:
        pp.zero_grad()
    m(x.clone()).abs().mean().backward()
    launched_in_backward.append(sum(pp._launched))
    written.append(len(pp._written))
    pp.reduce_gradients()
    for n, p in m.named_parameters():
        if n in want:
            worst = max(worst, float((p.grad - want[n]).abs().max()) / (float(want[n].abs().max()) + 1e-30))
        else:
            assert float(p.grad.abs().max()) == 0.0, n          # parameters outside the graph: zeros
torch.cuda.synchronize()
print("RESULT " + json.dumps({{"worst": worst, "launched": launched_in_backward, "written": written,
                              "buckets": len(pp.buckets)}}))
dist.destroy_process_group()
"""


def test_hook_launched_buckets_with_direct_writes_under_rccl_world1(tmp_path):
    """The multi-rank code path on the device: post-accumulate hooks + direct weight-gradient writes launch the
    bucket all-reduces (RCCL, world-1 group) DURING backward; the result equals plain autograd.  Fresh
    interpreter: the communicator is created before any kernel of the library runs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, "-c", OVERLAP_SCRIPT.format(root=root)], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["worst"] <= 2e-5, res
    # every bucket whose parameters all received a gradient went out from a hook before reduce_gradients
    assert min(res["launched"]) >= res["buckets"] - 2, res
    assert res["written"][0] >= 20 and res["written"][1] == 0 and res["written"][2] >= 20, res


TWO_RANK_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, {root!r})
import torch
import torch.distributed as dist
rank = int(os.environ["RANK"])
torch.cuda.set_device(0)                                        # both ranks share the one device of the box
dist.init_process_group("gloo", rank=rank, world_size=2)        # gloo moves device tensors through the host
from oracle.detinit import det_tensor
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D
from rehrseg_amd.parallel import PatchParallel
dev = torch.device("cuda:0")
def model():
    m = UNet_3D_3D(2, "unet_18", 4, 4)
    m.load_state_dict({{k: det_tensor(k, tuple(v.shape)) for k, v in m.state_dict().items()}})
    return m.to(dev)
xs = [torch.rand(2, 2, 4, 32, 32, generator=torch.Generator().manual_seed(20 + r)).to(dev) for r in range(2)]
# what the exchange must produce: the mean over the two ranks' patches of the single-rank gradients
want = None
for r in range(2):
    ref = model()
    ref(xs[r].clone()).abs().mean().backward()
    g = {{n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}}
    want = g if want is None else {{n: (want[n] + g[n]) / 2 for n in g}}
    del ref
m = model()
pp = PatchParallel(m, bucket_mb=8)                              # world 2: hooks launch the buckets during backward
assert pp.world == 2 and pp.overlap and pp.exchange and len(pp.buckets) >= 8 and pp.wgrad_stream() is not None
worst, launched, written = 0.0, [], []
for step in range(3):
    pp.zero_grad()
    m(xs[rank].clone()).abs().mean().backward()
    launched.append(sum(pp._launched))
    written.append(len(pp._written))
    pp.reduce_gradients()
    for n, p in m.named_parameters():
        if n in want:
            worst = max(worst, float((p.grad - want[n]).abs().max()) / (float(want[n].abs().max()) + 1e-30))
torch.cuda.synchronize()
if rank == 0:
    print("RESULT " + json.dumps({{"worst": worst, "launched": launched, "written": written, "buckets": len(pp.buckets)}}))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_exchange_on_the_device(tmp_path):
    """The N > 1 path with the real kernels: two ranks (sharing the box's one GPU; gloo carries the device buffers) run
    different patches through PatchParallel -- direct weight-gradient writes on the side stream, hand-over of the small
    gradients, hook-launched bucket exchanges issued from the side stream, division by the world size -- and every
    gradient must equal the mean of the two single-rank gradients."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "two_ranks.py"
    script.write_text(TWO_RANK_SCRIPT.format(root=root))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(script)], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["worst"] <= 2e-5, res
    assert min(res["launched"]) >= res["buckets"] - 2, res
    assert min(res["written"]) >= 20, res


def test_side_stream_weight_gradients_change_nothing():
    """PatchParallel(wgrad_stream=True): the direct-route weight-gradient kernels run on a second HIP stream while the
    main stream continues with the input-gradient chain.  Same kernels on the same operands, so the gradients must
    equal the single-stream ones.

    Gradients are compared on ONE recorded graph, backpropagated once per stream setting: two separate forward passes
    are not bit-identical (the SEGating means are fp64 atomics rounded to fp32: last-bit differences), and a
    pre-activation that sits within rounding of zero then flips its ReLU mask -- one voxel of one channel, which moves
    that channel's weight gradient by ~1e-3 of the tensor's largest element (tools/check_determinism.py shows the two
    modes; measured in round 3 when this test compared separate runs and failed one time in six).  On a shared graph
    the masks are shared and what is left is the summation order of the backward's own fp64 atomics: a few 1e-7.
    Also: a second accumulated backward pass (autograd accumulates into directly written slots), and three optimizer
    steps with each setting (parameters: loose bar, separate forwards).  A race would show as O(1) errors."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 2, 4, 48, 40, generator=g).to(dev)

    def rel(a, b):
        per = {n: float((a[n] - b[n]).abs().max()) / (float(a[n].abs().max()) + 1e-30) for n in a}
        worst = max(per, key=per.get)
        return per[worst], (worst, float(a[worst].abs().max()))

    def grads(m):
        return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}

    # ---- one graph, three backward passes: single stream, side stream, single stream again (the yardstick)
    m = _model(dev)
    pp = PatchParallel(m, wgrad_stream=True)
    assert pp.wgrad_stream() is not None
    loss = m(x.clone()).abs().mean()
    uses = dict(pp._uses)                                     # the forward's use counts (reduce_gradients ends a step
    got = {}                                                  # and clears them: re-armed for every pass over the graph)
    for tag, side in (("single", False), ("side", True), ("again", False)):
        pp.set_wgrad_stream(side)
        assert (pp.wgrad_stream() is not None) == side
        pp._uses = dict(uses)
        pp.zero_grad()
        loss.backward(retain_graph=True)
        assert len(pp._written) >= 20                         # the direct route (the one that uses the side stream)
        pp.join_side()
        torch.cuda.synchronize()
        got[tag] = grads(m)
        loss.backward(retain_graph=True)                      # accumulated on top (autograd's accumulation route)
        pp.reduce_gradients()
        torch.cuda.synchronize()
        got[tag + "+acc"] = grads(m)
    for k in ("", "+acc"):
        repro, _ = rel(got["single" + k], got["again" + k])
        d, where = rel(got["single" + k], got["side" + k])
        print("side stream vs single stream, gradients" + k, d, "run-to-run", repro, where)
        assert d <= max(2e-6, 4 * repro), (k, d, repro, where)
    for n, t in got["single+acc"].items():                    # (and the accumulation really doubled them)
        assert float((t - 2 * got["single"][n]).abs().max()) <= 1e-5 * (float(t.abs().max()) + 1e-30), n
    pp.close()
    del loss, got

    # ---- three optimizer steps with each setting: the parameters agree (separate forwards: mask flips allowed for)
    res = {}
    for side in (False, True):
        m = _model(dev)
        pp = PatchParallel(m, wgrad_stream=side)
        opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
        for _ in range(3):
            pp.zero_grad()
            m(x.clone()).abs().mean().backward()
            pp.reduce_gradients()
            opt.step()
        torch.cuda.synchronize()
        res[side] = {n: p.detach().clone() for n, p in m.named_parameters()}
        pp.close()
    d, where = rel(res[False], res[True])
    print("side stream vs single stream, parameters after 3 steps", d, where)
    assert d <= 1e-4, (d, where)
