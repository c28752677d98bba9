"""Boundary metrics on the MI355X (csrc/seg_surface.hip) against the brute-force fp64 oracle (tests/surface_oracle.py):
the surface counts exactly, every directed distance element by element after sorting, and hd, hd95, assd.

The bar, derived and not measured.  A distance is sqrtf of a sum of three fp32 terms (d * s)^2.  Each term takes a
product and a square, i.e. a relative error of at most 3 roundings of 2^-24 (the product's enters twice); the two
additions of non-negative numbers add one rounding each, so the squared distance is within 5 * 2^-24; the square root
halves that and the device sqrtf adds at most one ulp, 2 * 2^-24 relative: 4.5 * 2^-24.  The bar is 6 * 2^-24 relative
for every distance; hd is one of them, hd95 a convex combination of two and assd an fp64 mean, so the same bar holds
for the three metrics.  A zero distance has no rounding at all and must be exactly zero.  The spacings are exactly
representable in fp32, so the oracle and the kernels see the same values."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

import surface_oracle as so
from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L
from rehrseg_amd.utils import seg_utils as su

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = so.TOL
KEYS = ("hd", "hd95", "assd")


def _boxes():
    P, G = np.zeros((6, 20, 24), bool), np.zeros((6, 20, 24), bool)
    P[0:3, 0:7, 17:24] = True
    G[3:6, 12:20, 0:5] = True
    return P, G


def _points():
    P, G = np.zeros((6, 20, 24), bool), np.zeros((6, 20, 24), bool)
    P[2, 5, 5] = True
    G[4, 15, 20] = G[0, 0, 0] = True
    return P, G


def _noise():
    rng = np.random.RandomState(11)
    return rng.rand(6, 20, 24) < 0.3, rng.rand(6, 20, 24) < 0.3


def _case(name):
    if name == "ellipsoids":
        P, G, sp, _ = so.pinned_case()
        return P, G, sp
    if name == "boxes":
        return _boxes() + ((5.0, 0.5, 0.75),)
    if name == "points":
        return _points() + ((1.25, 1.0, 3.0),)
    if name == "noise":
        return _noise() + ((5.0, 0.5, 0.75),)
    if name == "long_lines":       # longer than one 64-wide step in H and W; W odd, no multiple of 4
        return (so.ellipsoid((5, 70, 67), (2, 30, 31), (2.4, 25, 28)),
                so.ellipsoid((5, 70, 67), (2.5, 40, 36), (1.8, 27, 22)), (4.0, 0.75, 0.75))
    if name == "one_slice":
        return (so.ellipsoid((1, 33, 40), (0, 15, 20), (1, 9, 13)), so.ellipsoid((1, 33, 40), (0, 18, 17), (1, 11, 8)),
                (3.0, 1.25, 1.0))
    if name == "same":
        P = so.pinned_case()[0]
        return P, P.copy(), (5.0, 0.5, 0.75)
    if name == "pred_empty":
        G = so.pinned_case()[1]
        return np.zeros_like(G), G, (5.0, 0.5, 0.75)
    if name == "both_empty":
        z = np.zeros((6, 20, 24), bool)
        return z, z.copy(), (1.0, 1.0, 1.0)
    if name == "lattice":          # the stage-2 lattice: a few 10^4 surface voxels each
        return (so.ellipsoid((16, 320, 384), (7.5, 150, 180), (6, 60, 80)),
                so.ellipsoid((16, 320, 384), (9, 170, 200), (5.5, 70, 70)), (5.0, 0.5, 0.5))
    raise KeyError(name)


SMALL = ("ellipsoids", "boxes", "points", "noise", "long_lines", "one_slice", "same", "pred_empty", "both_empty")


@functools.lru_cache(maxsize=None)
def _oracle(name):
    P, G, sp = _case(name)
    return so.metrics(P, G, sp, device=DEV if name == "lattice" else None)


def _run(P, G, sp):
    """The two backend calls and torch's sort between them, as seg_utils composes them; returns the distance buffer
    (2, N) and the five int64 on the host."""
    pred = torch.from_numpy(P.astype(np.uint8)).to(DEV)
    gt = torch.from_numpy(G.astype(np.uint8)).to(DEV)
    out = torch.zeros(5, dtype=torch.int64, device=DEV)
    dist, ws = hb.seg_surface_distances(pred, gt, sp, out[3:5])
    hb.seg_surface_reduce(dist, torch.sort(dist.view(-1)).values, out[3:5], out[0:3], ws)
    return dist.cpu(), out.cpu()


def _check_distances(got32, want, what):
    got = np.sort(got32[np.isfinite(got32)].astype(np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if len(want) == 0:
        return
    err = np.abs(got - want)
    worst = float((err / np.maximum(want, 1e-300)).max() / 2.0 ** -24)
    print(f"{what}: {len(want)} distances, worst relative error {worst:.3f} * 2^-24, {int((want == 0).sum())} zeros")
    assert (got[want == 0] == 0).all(), what
    assert (err <= TOL * want).all(), (what, worst)


def _check_metrics(got, want, what):
    assert got["n_pred"] == want["n_pred"] and got["n_gt"] == want["n_gt"], (what, got, want)
    for k in KEYS:
        if math.isnan(want[k]):
            assert math.isnan(got[k]), (what, k, got[k])
        else:
            print(f"{what} {k}: {got[k]!r} (oracle {want[k]!r})")
            assert abs(got[k] - want[k]) <= TOL * want[k], (what, k, got[k], want[k])


def _check_case(name):
    P, G, sp = _case(name)
    want = _oracle(name)
    dist, out = _run(P, G, sp)
    d = dist.numpy()
    # the buffer is finite exactly at the surface voxels of its own map (when the other surface is not empty)
    if want["n_pred"] and want["n_gt"]:
        assert np.array_equal(np.isfinite(d[0]).reshape(P.shape), so.surface(P))
        assert np.array_equal(np.isfinite(d[1]).reshape(P.shape), so.surface(G))
    else:
        assert not np.isfinite(d).any()
    _check_distances(d[0], want["s_pg"], f"{name} pred->gt")
    _check_distances(d[1], want["s_gp"], f"{name} gt->pred")
    got = su._surface_result(out.numpy())
    _check_metrics(got, want, name)
    public = su.surface_distance_metrics(P, G, sp, device=DEV)
    assert {k: public[k] for k in ("n_pred", "n_gt")} == {k: got[k] for k in ("n_pred", "n_gt")}
    for k in KEYS:
        assert public[k] == got[k] or (math.isnan(public[k]) and math.isnan(got[k])), (name, k)
    return got, want


@pytest.mark.parametrize("name", SMALL)
def test_small_cases_meet_the_oracle(name):
    got, want = _check_case(name)
    if name == "ellipsoids":
        pinned = so.pinned_case()[3]
        assert (want["n_pred"], want["n_gt"]) == (238, 250)
        for k in KEYS:
            assert abs(want[k] - pinned[k]) <= 1e-12 and abs(got[k] - pinned[k]) <= TOL * pinned[k]
    if name == "boxes":
        assert abs(want["hd"] - 21.542109924517607) <= 1e-12 and abs(want["hd95"] - 20.661757274067785) <= 1e-12
    if name == "points":
        assert want["n_pred"] + want["n_gt"] == 3                   # the percentile interpolates
    if name == "noise":
        zeros = int((want["s_pg"] == 0).sum()) + int((want["s_gp"] == 0).sum())
        assert zeros > 0.2 * (want["n_pred"] + want["n_gt"])
    if name == "same":
        assert got["hd"] == 0.0 and got["hd95"] == 0.0 and got["assd"] == 0.0 and got["n_pred"] == got["n_gt"] > 0
    if name == "pred_empty":
        assert got["n_pred"] == 0 and got["n_gt"] == 250 and all(math.isnan(got[k]) for k in KEYS)
    if name == "both_empty":
        assert got["n_pred"] == 0 and got["n_gt"] == 0 and all(math.isnan(got[k]) for k in KEYS)


def test_stage2_lattice_case_meets_the_oracle():
    got, want = _check_case("lattice")
    assert 2e4 < want["n_pred"] < 1e5 and 2e4 < want["n_gt"] < 1e5


@pytest.mark.parametrize("name", ("noise", "lattice"))
def test_two_runs_give_the_same_bits(name):
    P, G, sp = _case(name)
    d1, o1 = _run(P, G, sp)
    d2, o2 = _run(P, G, sp)
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32)) and torch.equal(o1, o2)


def test_unsupported_extent_raises_without_a_launch():
    big = torch.zeros((1, 2049, 2), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
            su.surface_distance_metrics(big, big, device=DEV)
        with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
            hb.seg_surface_distances(big, big, (1.0, 1.0, 1.0), torch.zeros(2, dtype=torch.int64, device=DEV))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    lib = L.load()
    assert lib.rehr_seg_surface_workspace_bytes(1, 2049, 2) == -2
    assert lib.rehr_seg_surface_dist_f32(big.data_ptr(), big.data_ptr(), 1, 2049, 2, 1.0, 1.0, 1.0, big.data_ptr(),
                                         big.data_ptr(), big.data_ptr(), 1 << 40, None) == -2
    with pytest.raises(ValueError):
        su.surface_distance_metrics(big[:, :8], big[:, :8], (1.0, 0.0, 1.0), device=DEV)


class DevToy(torch.nn.Module):
    """A position- and orientation-sensitive toy network built from device ops only (no host tensors, no syncs)."""

    def __init__(self, sep=2, scale=1.0):
        super().__init__()
        self.sep, self.scale = sep, scale

    def forward(self, x):
        sh = torch.roll(x, shifts=(1, 2), dims=(3, 4))
        lr = torch.cat([x * 0.5 + sh * 0.25, -x * 0.75 + sh * sh * 0.125 - 0.1], 1) * self.scale
        return lr, torch.repeat_interleave(lr, self.sep, dim=2) * 1.5


def _count_syncs(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return out, [w for w in rec if "called a synchronizing" in str(w.message)]


def test_evaluate_case_with_surface_makes_one_host_sync():
    model = DevToy(sep=4)
    g = np.random.RandomState(3)
    img = g.randint(0, 256, size=(1, 10, 70, 80)).astype(np.float32)
    lab = (g.rand(1, 10, 70, 80) < 0.4).astype(np.float32)
    sp = (4.0, 0.75, 0.5)
    args = (model, img, lab, 4, [8, 32, 32], True, DEV)
    run = lambda: su._evaluate_case(*args, surface=True, spacing=sp)  # noqa: E731
    first = run()                                                      # warm-up: cached Gaussian, sort's workspace
    torch.cuda.synchronize()
    out, syncs = _count_syncs(run)
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    plain = su._evaluate_case(*args)
    assert len(plain) == 5 and len(out) == 6
    assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1]) and torch.equal(out[2], plain[2])
    assert out[3] == plain[3] and out[4] == plain[4] and out[5] == first[5]
    want = so.metrics(out[0], lab[0], sp)
    _check_metrics(out[5], want, "evaluate_case")
    public = su.evaluate_case(model, img, lab, 4, [8, 32, 32], device=DEV, surface=True, spacing=sp)
    assert len(public) == 5 and public[4] == out[5]


def test_surface_distance_metrics_makes_one_host_sync():
    P, G, sp = _case("ellipsoids")
    pred, gt = torch.from_numpy(P).to(DEV), torch.from_numpy(G).to(DEV)
    su.surface_distance_metrics(pred, gt, sp)
    torch.cuda.synchronize()
    out, syncs = _count_syncs(lambda: su.surface_distance_metrics(pred, gt, sp))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    _check_metrics(out, _oracle("ellipsoids"), "device tensors")
